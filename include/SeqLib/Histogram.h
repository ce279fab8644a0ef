// Histogram.h -- SeqLib::Bin and SeqLib::Histogram for the MI355X drop-in: evenly spaced bins with inclusive bounds, as BamStats keeps them.  Host only; it links
// nothing.  The reference class is src/non_api/Histogram.{h,cpp}; the bin layout of Histogram(start, end, width) (Histogram.cpp:14-48) and toFileString's format
// (:64-73) are kept, and three things that are broken there are put right and named:
//   the constructor    the reference tests `end >= start` and so throws for every valid argument; here std::invalid_argument when end <= start, as its header says
//   retrieveBinID      the reference returns m_bins.size(), one past the last bin, for a value in the last bin; here the last bin is the last bin
//   out of range       the reference calls exit(1) (a 300 bp read in BamStats' len histogram); here a value below the first bound counts in NumBelow(), one above
//                      the last in NumAbove(), no bin is touched, and retrieveBinID returns npos
// toFileString of an empty histogram is the empty string (the reference's pop_back() on an empty string is undefined).  Counts are uint64 (getCount() included).
// Not carried: Initialize (quantile bins from a span vector), toCSV, the interval-tree typedefs.
#pragma once
#include <cstddef>
#include <cstdint>
#include <ostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace SeqLib {

class Histogram;

class Bin {
    friend class Histogram;
public:
    Bin() = default;                                   // no count, the range [0, 1]
    uint64_t getCount() const { return n_; }
    int32_t First() const { return lo_; }
    int32_t Second() const { return hi_; }
    bool contains(const int32_t &elem) const { return lo_ <= elem && elem <= hi_; }
    bool operator<(const Bin &o) const { return std::make_pair(lo_, hi_) < std::make_pair(o.lo_, o.hi_); }          // by lower bound, then by upper
    Bin &operator++() { n_ += 1; return *this; }
    Bin &operator--() { if (n_ > 0) n_ -= 1; return *this; }          // an empty bin stays empty
    friend std::ostream &operator<<(std::ostream &out, const Bin &b) { out << b.lo_ << ',' << b.hi_ << ',' << b.n_; return out; }          // "first,second,count"
private:
    Bin(int32_t lo, int32_t hi) : lo_(lo), hi_(hi) {}
    int32_t lo_ = 0, hi_ = 1;
    uint64_t n_ = 0;
};

class Histogram {
public:
    static const size_t npos = (size_t)-1;
    std::vector<Bin> m_bins;

    Histogram() {}
    // n = (end - start) / width + 1 bins; bin k is [start + k * width, start + (k + 1) * width - 1], the last one ends at `end` (st_layout, st_bin_lo and st_bin_hi of
    // seqlib_amd/csrc/dev_stats.h state the same rule for the kernels)
    Histogram(const int32_t &start, const int32_t &end, const uint32_t &width) : start_(start), width_(width)
    {
        if (end <= start) throw std::invalid_argument("SeqLib::Histogram - the range is empty: end " + std::to_string(end) + " is not above start " + std::to_string(start));
        if (width == 0) throw std::invalid_argument("SeqLib::Histogram - a bin width of 0");
        const int64_t n = ((int64_t)end - start) / width_ + 1;
        m_bins.reserve((size_t)n);
        for (int64_t k = 0; k < n; ++k) m_bins.push_back(Bin((int32_t)(start_ + k * width_), k == n - 1 ? end : (int32_t)(start_ + (k + 1) * width_ - 1)));
    }

    // the bin of elem, or npos outside [first bound, last bound]
    size_t retrieveBinID(const int32_t &elem) const
    {
        if (m_bins.empty() || elem < m_bins.front().lo_ || elem > m_bins.back().hi_) return npos;
        return (size_t)(((int64_t)elem - start_) / width_);          // elem <= end: at most the last bin
    }
    void addElem(const int32_t &elem) { addCount(elem, 1); }
    void removeElem(const int32_t &elem)
    {
        const size_t i = retrieveBinID(elem);
        if (i != npos) --m_bins[i];
        else if (m_bins.empty() || elem < m_bins.front().lo_) { if (below_) --below_; }
        else if (above_) --above_;
    }
    // n elements of value elem (new)
    void addCount(int64_t elem, uint64_t n)
    {
        if (m_bins.empty() || elem < m_bins.front().lo_) below_ += n;
        else if (elem > m_bins.back().hi_) above_ += n;
        else m_bins[(size_t)((elem - start_) / width_)].n_ += n;
    }
    // n elements into bin i, and into the two counts outside (new: what a GPU-side histogram hands over)
    void addToBin(size_t i, uint64_t n) { m_bins.at(i).n_ += n; }
    void addOutside(uint64_t below, uint64_t above) { below_ += below; above_ += above; }

    uint64_t NumBelow() const { return below_; }
    uint64_t NumAbove() const { return above_; }
    uint64_t totalCount() const { uint64_t t = 0; for (const Bin &b : m_bins) t += b.getCount(); return t; }
    uint64_t binCount(size_t i) const { return m_bins[i].getCount(); }
    size_t numBins() const { return m_bins.size(); }

    // the non-empty bins as first_second_count joined by ','
    std::string toFileString() const
    {
        std::string out;
        for (const Bin &b : m_bins) {
            if (!b.n_) continue;
            if (!out.empty()) out += ',';
            out += std::to_string(b.lo_) + "_" + std::to_string(b.hi_) + "_" + std::to_string(b.n_);
        }
        return out;
    }
    // a line per bin
    friend std::ostream &operator<<(std::ostream &out, const Histogram &h)
    {
        for (size_t k = 0; k < h.m_bins.size(); ++k) out << h.m_bins[k] << '\n';
        return out.flush();
    }

private:
    int64_t start_ = 0, width_ = 1;
    uint64_t below_ = 0, above_ = 0;
};

}  // namespace SeqLib
