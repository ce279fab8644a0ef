// BamStats.h -- SeqLib::BamReadGroup and SeqLib::BamStats for the MI355X drop-in: per-read-group counters and histograms of a BAM's records, counted in HBM
// behind include/seqlib_amd_stats.h.  The reference classes are src/non_api/BamStats.{h,cpp}; they are orphaned there (they call BamRecord::MeanPhred() and an int
// GetIntTag(tag) that no longer exist, over a Histogram whose constructor throws for every valid argument), so the interface, the output format and addRead's
// arithmetic (BamStats.cpp:45-109) are kept and the rest is defined by seqlib_amd_stats.h, which lists every rule.  In short: the group is RG:Z, else "QNAMED_" +
// the name up to its first ':' (else "NA"); six counters and six histograms per group; kept quirk: `supp` counts flag 0x100 (SecondaryFlag under that name).
// Deviations: a value outside a histogram counts in its NumBelow() / NumAbove() where the reference exits; a record without an integer NM adds nothing to nm and
// counts in "nm_missing"; groups print in order of first appearance where the reference's unordered_map gives none; an empty histogram prints an empty field.
//   addRead(BamRecord&)     one record, on the host through slx_stats_record -- the body the kernels compile -- with no GPU, as ReadFilter::isValid does
//   addReads(BamReader&)    (new, the reason for the GPU) drains a reader batch by batch from HBM to HBM; SetRegions and SetReadFilter are honoured, a record
//                           served once per region it overlaps counts once per region
//   addBatch(slx_rec_batch) (new) the records alignToBam's builder left in HBM
// Host-added and GPU-added reads land in the same object: groups first seen by addRead come first in their order, groups first seen on the GPU behind them in
// theirs.  SetExcludeFlags / SetMinMapq act on addReads and addBatch only (addRead tests nothing, as in the reference).  A C-ABI failure is a std::runtime_error.
#pragma once
#include <cstdint>
#include <cstring>
#include <ostream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamRecord.h"
#include "SeqLib/Histogram.h"
#include "seqlib_amd_rec.h"
#include "seqlib_amd_stats.h"

namespace SeqLib {

namespace detail {
static const char *const stats_counter_names[14] = {"reads", "supp", "qcfail", "duplicate", "unmap", "mate_unmap", "supplementary", "paired", "proper_pair", "read1", "read2", "reverse",
                                                    "bases", "nm_missing"};
static const uint32_t stats_counter_bits[12] = {0, 0x100, 0x200, 0x400, 0x4, 0x8, 0x800, 0x1, 0x2, 0x40, 0x80, 0x10};          // reads: every record
inline void stats_check(int rc, const char *who) { if (rc != SLX_OK) throw std::runtime_error(std::string(who) + " - " + slx_last_error()); }
inline slx_stats_rec stats_record(BamRecord &r, const char *who)
{
    if (!r.raw()) throw std::invalid_argument(std::string(who) + " - empty BamRecord");
    const std::vector<uint8_t> p = packed_record(r.raw());
    slx_stats_rec v;
    stats_check(slx_stats_record(p.data(), (int64_t)p.size(), &v), who);
    return v;
}
}  // namespace detail

class BamReadGroup {
    friend class BamStats;
public:
    BamReadGroup() : BamReadGroup(std::string()) {}
    explicit BamReadGroup(const std::string &name, int32_t len_max = 250, int32_t isize_max = 2000) : m_name(name)
    {
        h_[SLX_STATS_MAPQ] = Histogram(0, 100, 1); h_[SLX_STATS_NM] = Histogram(0, 100, 1); h_[SLX_STATS_ISIZE] = Histogram(-2, isize_max, 10);
        h_[SLX_STATS_CLIP] = Histogram(0, 100, 5); h_[SLX_STATS_PHRED] = Histogram(0, 100, 1); h_[SLX_STATS_LEN] = Histogram(0, len_max, 1);
    }
    // the record's counts into this group, whatever its own group is
    void addRead(BamRecord &r) { add(detail::stats_record(r, "BamReadGroup::addRead")); }
    const std::string &Name() const { return m_name; }
    // "reads", "supp", "qcfail", "duplicate", "unmap", "mate_unmap" and the new ones of seqlib_amd_stats.h
    uint64_t Counter(const std::string &name) const
    {
        for (int i = 0; i < 14; ++i) if (name == detail::stats_counter_names[i]) return c_[i];
        throw std::invalid_argument("BamReadGroup::Counter - unknown counter '" + name + "'");
    }
    // SLX_STATS_MAPQ .. SLX_STATS_LEN
    const Histogram &Hist(int which) const
    {
        if (which < 0 || which >= SLX_STATS_N_HIST) throw std::invalid_argument("BamReadGroup::Hist - unknown histogram");
        return h_[which];
    }
    friend std::ostream &operator<<(std::ostream &out, const BamReadGroup &g)
    {
        out << g.m_name << "\t" << g.c_[0] << "\t" << g.c_[1] << "\t" << g.c_[4] << "\t" << g.c_[5] << "\t" << g.c_[2] << "\t" << g.c_[3];          // reads supp unmap mate_unmap qcfail duplicate
        for (const Histogram &h : g.h_) out << "\t" << h.toFileString();
        return out;
    }

private:
    void add(const slx_stats_rec &v)
    {
        ++c_[0];
        for (int i = 1; i < 12; ++i) if (v.flag & detail::stats_counter_bits[i]) ++c_[i];
        if (v.value[SLX_STATS_LEN] > 0) c_[12] += (uint64_t)v.value[SLX_STATS_LEN];
        if (!v.has_nm) ++c_[13];
        for (int h = 0; h < SLX_STATS_N_HIST; ++h) if (h != SLX_STATS_NM || v.has_nm) h_[h].addCount(v.value[h], 1);
    }
    void merge(const BamReadGroup &o)
    {
        for (int i = 0; i < 14; ++i) c_[i] += o.c_[i];
        for (int h = 0; h < SLX_STATS_N_HIST; ++h) {
            if (h_[h].numBins() != o.h_[h].numBins()) throw std::runtime_error("BamStats - the bin layouts differ");
            for (size_t k = 0; k < o.h_[h].numBins(); ++k) h_[h].addToBin(k, o.h_[h].binCount(k));
            h_[h].addOutside(o.h_[h].NumBelow(), o.h_[h].NumAbove());
        }
    }
    uint64_t c_[14] = {};
    Histogram h_[SLX_STATS_N_HIST];
    std::string m_name;
};

class BamStats {
public:
    BamStats() = default;
    BamStats(const BamStats &) = delete;
    BamStats &operator=(const BamStats &) = delete;
    ~BamStats() { if (st_) slx_stats_free(st_); }

    // BamStats.cpp:86-109: the record's group, made on first appearance, takes it.  On the host.
    void addRead(BamRecord &r)
    {
        const slx_stats_rec v = detail::stats_record(r, "BamStats::addRead");
        host_group(std::string(v.group, (size_t)v.group_len)).add(v);
    }
    // every record the reader still has, batch by batch, from HBM to HBM; returns how many were handed over
    size_t addReads(BamReader &rd)
    {
        if (!rd.rd_) throw std::runtime_error("BamStats::addReads - the reader is not open");
        need();
        size_t n = 0;
        while (rd.advance()) {
            const slx_bam_batch &b = rd.batch_;
            const int64_t k = b.n_records - (int64_t)rd.cur_;
            check(slx_stats_add_device(st_, b.d_stream, b.n_bytes, (const uint64_t *)b.d_rec_off + rd.cur_, k));
            rd.cur_ = (size_t)b.n_records;
            n += (size_t)k;
        }
        return n;
    }
    // the records a builder left in HBM (slx_rec_build*, BWAAligner::alignToBam)
    void addBatch(const slx_rec_batch &b)
    {
        need();
        check(slx_stats_add_device(st_, b.d_stream, b.n_bytes, b.d_rec_off, b.n_records));
    }

    void SetExcludeFlags(uint32_t f) { SetKnob("exclude_flags", f); }
    void SetMinMapq(int q) { SetKnob("min_mapq", q); }
    // a key of slx_stats_set; "len_max" and "isize_max" before the first read only
    void SetKnob(const char *key, int64_t v)
    {
        need();
        const bool is_len = !std::strcmp(key, "len_max"), is_isize = !std::strcmp(key, "isize_max");
        if ((is_len || is_isize) && !host_.empty()) throw std::runtime_error(std::string("BamStats - ") + key + " after the first read");
        check(slx_stats_set(st_, key, v));
        if (is_len) len_max_ = (int32_t)v;
        if (is_isize) isize_max_ = (int32_t)v;
    }
    int64_t Counter(const char *name) const { return st_ ? slx_stats_counter(st_, name) : -1; }

    // this += o, groups matched by name
    void Merge(BamStats &o)
    {
        if (&o == this) throw std::invalid_argument("BamStats::Merge - an object into itself");
        if (len_max_ != o.len_max_ || isize_max_ != o.isize_max_) throw std::runtime_error("BamStats::Merge - the bin layouts differ");
        for (const BamReadGroup &g : o.host_) host_group(g.m_name).merge(g);
        if (o.st_ && slx_stats_n_groups(o.st_) > 0) { need(); check(slx_stats_merge(st_, o.st_)); }
    }
    void clear()
    {
        host_.clear(); index_.clear();
        if (st_) check(slx_stats_clear(st_));
    }

    // the groups with the host's and the GPU's counts summed
    std::vector<BamReadGroup> Groups() const
    {
        std::vector<BamReadGroup> out = host_;
        if (!st_) return out;
        std::unordered_map<std::string, size_t> at = index_;
        const int64_t n = slx_stats_n_groups(st_);
        std::vector<uint64_t> bins;
        for (int64_t i = 0; i < n; ++i) {
            const char *nm = slx_stats_group_name(st_, i);
            if (!nm) throw std::runtime_error("BamStats - a group without a name");
            auto it = at.find(nm);
            if (it == at.end()) { it = at.emplace(nm, out.size()).first; out.push_back(BamReadGroup(nm, len_max_, isize_max_)); }
            BamReadGroup &g = out[it->second];
            for (int k = 0; k < 14; ++k) {
                const int64_t v = slx_stats_counter_of(st_, i, detail::stats_counter_names[k]);
                if (v < 0) check((int)v);
                g.c_[k] += (uint64_t)v;
            }
            for (int h = 0; h < SLX_STATS_N_HIST; ++h) {
                bins.assign(g.h_[h].numBins(), 0);
                uint64_t below = 0, above = 0;
                check(slx_stats_hist(st_, i, h, bins.data(), (int64_t)bins.size(), &below, &above));
                for (size_t k = 0; k < bins.size(); ++k) g.h_[h].addToBin(k, bins[k]);
                g.h_[h].addOutside(below, above);
            }
        }
        return out;
    }
    size_t NumGroups() const { return Groups().size(); }
    BamReadGroup Group(const std::string &name) const
    {
        for (const BamReadGroup &g : Groups()) if (g.m_name == name) return g;
        throw std::out_of_range("BamStats::Group - no group '" + name + "'");
    }
    // BamStats.cpp:21-26: the header line, then a line per group
    friend std::ostream &operator<<(std::ostream &out, const BamStats &s)
    {
        out << "ReadGroup\tReadCount\tSupplementary\tUnmapped\tMateUnmapped\tQCFailed\tDuplicate\tMappingQuality\tNM\tInsertSize\tClippedBases\tMeanPhredScore\tReadLength" << std::endl;
        for (const BamReadGroup &g : s.Groups()) out << g << std::endl;
        return out;
    }

private:
    void check(int rc) const { detail::stats_check(rc, "BamStats"); }
    void need() { if (!st_) check(slx_stats_create(-1, &st_)); }
    BamReadGroup &host_group(const std::string &name)
    {
        auto it = index_.find(name);
        if (it == index_.end()) { it = index_.emplace(name, host_.size()).first; host_.push_back(BamReadGroup(name, len_max_, isize_max_)); }
        return host_[it->second];
    }
    slx_stats *st_ = nullptr;
    int32_t len_max_ = 250, isize_max_ = 2000;
    std::vector<BamReadGroup> host_;
    std::unordered_map<std::string, size_t> index_;
};

}  // namespace SeqLib
