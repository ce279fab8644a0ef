// GenomicRegionCollection.h -- SeqLib::GenomicRegionCollection<T> and GRC for the MI355X drop-in: the whole surface of the reference's
// SeqLib/GenomicRegionCollection.h:32-344 with SeqLib/GenomicRegionCollection.cpp, header-only over the C-ABI of include/seqlib_amd_grc.h.  There is no pointer
// tree: CreateTreeMap builds a sorted index (slx_grc; in HBM when there is a GPU, host-only otherwise) and "the tree" below means that object.
// Two tiers.  As it stands the header needs nothing but GenomicRegion.h and declares what needs no library: the container, the tiling constructors, Concat, Pad,
// Shuffle, TotalWidth, Rewind, empty, AsBEDString, operator<<, CoordinateSort, SortAndStretchLeft / Right.  With SEQLIB_GRC_QUERIES defined for the whole build
// (-DSEQLIB_GRC_QUERIES: BamReader.h includes this header, so a #define has to stand before the first include) it also declares everything that needs
// libseqlib_amd.so, zlib or BamRecord.h: CreateTreeMap, the queries, MergeOverlappingIntervals, NumTree, ReadBED / ReadVCF, the file and BamRecordVector
// constructors, OverlapReads / CountReads / SubjectCounts / OverlapBatch.  Without the macro a use of those does not compile (no stub that answers nothing).
// The object's layout is the same in both tiers.
//   host only, as in the reference   the container (add, size, [], at, begin / end, clear, IsEmpty, empty), Concat, Pad, Shuffle, TotalWidth, Rewind, NumTree,
//                                    AsBEDString, operator<<, CoordinateSort (stable here), SortAndStretchLeft / Right, both tiling constructors, the
//                                    BamRecordVector and the file constructors, ReadBED / ReadVCF (plain or gzip through zlib; a gz error gives false with a
//                                    message where the reference calls exit())
//   single queries, on the host      FindOverlaps(gr), FindOverlappedIntervals, CountOverlaps, CountContained, OverlapSameInterval, FindOverlapWidth: answered
//                                    by slx_grc_query_host from the index's host mirror, no GPU round trip per call; they work without a GPU
//   batches, on the GPU              FindOverlaps(subject, query_id, subject_id), Intersection (slx_grc_overlaps on the subject's index),
//                                    MergeOverlappingIntervals (slx_grc_merged), and new next to the reference: OverlapReads / CountReads / SubjectCounts over the
//                                    batches a BamReader serves (SetRegions and SetReadFilter are honoured: only NextBatch's batches are consumed) and OverlapBatch
//                                    for a slx_bam_batch / slx_rec_batch.  std::runtime_error carries a C-ABI failure (SLX_ENODEVICE without a GPU: no CPU fallback)
// Differences on purpose: the hits of a query come by ascending (pos1, pos2, id), not in the tree's traversal order; the collection join looks
// the query's chr up in the SUBJECT's index (the reference compares the subject's iterator with its own tree's end(), GenomicRegionCollection.cpp:650);
// CountContained, declared but never defined in the reference, is defined by TIntervalTree::findContained's rule (IntervalTree.h:224); an interval with
// pos2 < pos1 is std::invalid_argument; at() throws std::out_of_range where the reference throws the int 20; the vector is held by value, so a copy of a
// collection owns its intervals (the index, immutable once built, is shared).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <functional>
#include <iostream>
#include <memory>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "SeqLib/BamHeader.h"
#include "SeqLib/GenomicRegion.h"
#ifdef SEQLIB_GRC_QUERIES
#include <zlib.h>
#include "SeqLib/BamRecord.h"
#include "seqlib_amd_grc.h"
#endif

namespace SeqLib {

typedef std::pair<size_t, size_t> OverlapResult;

template <typename T = GenomicRegion> class GenomicRegionCollection {
    template <typename K> friend class GenomicRegionCollection;
public:
    typedef typename std::vector<T>::iterator iterator;
    typedef typename std::vector<T>::const_iterator const_iterator;

    GenomicRegionCollection() = default;
    explicit GenomicRegionCollection(const std::vector<T> &vec) : v_(vec) {}
    explicit GenomicRegionCollection(const T &gr) : v_(1, gr), m_sorted(true) {}
#ifdef SEQLIB_GRC_QUERIES
    // (ChrID, Position, PositionEnd) of every record: BamRecord::AsGenomicRegion
    explicit GenomicRegionCollection(const BamRecordVector &brv)
    {
        for (BamRecordVector::const_iterator i = brv.begin(); i != brv.end(); ++i) v_.push_back(T(i->ChrID(), i->Position(), i->PositionEnd()));
    }
#endif
    // gr in bins of `width` that overlap by `ovlp`, and a last piece up to gr.pos2 (GenomicRegionCollection.cpp:358-397)
    GenomicRegionCollection(int width, int ovlp, const T &gr)
    {
        if (width <= ovlp) throw std::invalid_argument("Width should be > ovlp");
        if (width >= gr.Width()) { v_.push_back(gr); return; }
        int32_t start = gr.pos1, end = gr.pos1 + width;
        if (end > gr.pos2) { std::cerr << "GenomicRegionCollection constructor: GenomicRegion is smaller than bin width" << std::endl; return; }
        while (end <= gr.pos2) {
            v_.push_back(T(gr.chr, start, end));
            end += width - ovlp;
            start += width - ovlp;
        }
        if (v_.back().pos2 != gr.pos2) v_.push_back(T(gr.chr, v_.back().pos2 - ovlp, gr.pos2));
        m_sorted = true;
    }
    // every sequence of h tiled the same way, from 0 to its length; no last piece (GenomicRegionCollection.cpp:20-66)
    GenomicRegionCollection(int width, int ovlp, const HeaderSequenceVector &h)
    {
        if (width <= ovlp) throw std::invalid_argument("Width should be > ovlp");
        int32_t chr = 0;
        for (HeaderSequenceVector::const_iterator i = h.begin(); i != h.end(); ++i, ++chr) {
            T gr;
            gr.chr = chr; gr.pos1 = 0; gr.pos2 = (int32_t)i->Length;
            if (width >= gr.Width()) { v_.push_back(gr); continue; }
            int32_t start = gr.pos1, end = gr.pos1 + width;
            if (end > gr.pos2) { std::cerr << "GenomicRegionCollection constructor: GenomicRegion is smaller than bin width" << std::endl; return; }
            while (end <= gr.pos2) {
                T tg;
                tg.chr = gr.chr; tg.pos1 = start; tg.pos2 = end;
                v_.push_back(tg);
                end += width - ovlp;
                start += width - ovlp;
            }
        }
    }
#ifdef SEQLIB_GRC_QUERIES
    // contains ':' -> one samtools-style region; contains ".vcf" -> ReadVCF; anything else (".bed" or not) -> ReadBED
    GenomicRegionCollection(const std::string &file, const BamHeader &hdr)
    {
        if (file.find(":") != std::string::npos) { m_sorted = true; v_.push_back(T(file, hdr)); return; }
        if (file.find(".bed") == std::string::npos && file.find(".vcf") != std::string::npos) ReadVCF(file, hdr);
        else ReadBED(file, hdr);
    }

    // chr, pos1, pos2 of every line without a '#'; entries whose chr the header does not know are dropped.  Plain or gzip'd.
    bool ReadBED(const std::string &file, const BamHeader &hdr)
    {
        m_sorted = false; idx_ = 0;
        return read_lines(file, "BED", [&](const std::string &line) {
            if (line.find("#") != std::string::npos) return;
            std::istringstream iss(line);
            std::string chr, pos1, pos2;
            if (!(iss >> chr >> pos1 >> pos2)) return;
            T gr(chr, pos1, pos2, hdr);
            if (gr.chr >= 0) v_.push_back(gr);
        });
    }
    // chr and pos of every line that does not start with '#', width 1
    bool ReadVCF(const std::string &file, const BamHeader &hdr)
    {
        m_sorted = false; idx_ = 0;
        return read_lines(file, "VCF", [&](const std::string &line) {
            if (line.empty() || line[0] == '#') return;
            std::istringstream iss(line);
            std::string chr, pos;
            if (!(iss >> chr >> pos)) return;
            T gr;
            try { gr = T(chr, pos, pos, hdr); }
            catch (...) { std::cerr << "...Could not parse pos: " << pos << std::endl << std::endl << "...on line " << line << std::endl; }
            if (gr.chr >= 0) v_.push_back(gr);
        });
    }

#endif
    void Shuffle()
    {
        static thread_local std::mt19937 rng(std::random_device{}());
        std::shuffle(v_.begin(), v_.end(), rng);
    }
    // by (chr, pos1, pos2), stable
    void CoordinateSort()
    {
        std::stable_sort(v_.begin(), v_.end());
        m_sorted = true;
    }
#ifdef SEQLIB_GRC_QUERIES
    // Sorts unless marked sorted (add does not clear the mark, as in the reference), then builds the index: in HBM when there is a GPU, host-only otherwise.
    void CreateTreeMap()
    {
        tree_.reset();
        if (v_.empty()) return;
        if (!m_sorted) CoordinateSort();
        tree_ = make_tree(v_);
    }
    // The minimal set of intervals: touching ones merge ([4,6] and [6,8]).  A merged interval is its first member (by sorted order) with the run's largest pos2.
    void MergeOverlappingIntervals()
    {
        if (v_.empty()) { tree_.reset(); return; }
        const std::shared_ptr<void> held = make_tree(v_);
        slx_grc *g = static_cast<slx_grc *>(held.get());
        std::vector<slx_grc_iv> m(v_.size());
        std::vector<int32_t> perm(v_.size());
        int64_t n = 0;
        check(slx_grc_merged(g, m.data(), (int64_t)m.size(), &n), "MergeOverlappingIntervals");
        check(slx_grc_sorted(g, nullptr, perm.data(), nullptr, nullptr), "MergeOverlappingIntervals");
        std::vector<T> out;
        out.reserve((size_t)n);
        int64_t k = -1;
        for (size_t i = 0; i < perm.size(); ++i) {          // a run's first member is the first sorted entry past the run before it
            const T &e = v_[(size_t)perm[i]];
            if (k >= 0 && e.chr == m[(size_t)k].chr && e.pos1 <= m[(size_t)k].pos2) continue;
            ++k;
            out.push_back(e);
            out.back().pos2 = m[(size_t)k].pos2;
        }
        v_.swap(out);
        tree_.reset();
    }

#endif
    size_t size() const { return v_.size(); }
    void add(const T &g) { v_.push_back(g); idx_ = 0; }
    bool IsEmpty() const { return v_.empty(); }
    bool empty() const { return v_.empty(); }
    void clear() { v_.clear(); tree_.reset(); idx_ = 0; }
#ifdef SEQLIB_GRC_QUERIES
    // the chr values the index holds (the reference's number of per-chromosome trees); 0 before CreateTreeMap
    int NumTree() const { return tree_ ? (int)slx_grc_counter(tree(), "chrs") : 0; }
#endif
    void Rewind() { idx_ = 0; }
    // unchecked, as a vector's; at() throws out_of_range
    const T &operator[](size_t i) const { return v_[i]; }
    T &operator[](size_t i) { return v_[i]; }
    const T &at(size_t i) const
    {
        if (i >= v_.size()) throw std::out_of_range("GenomicRegionCollection::at - index out of range");
        return v_[i];
    }
    iterator begin() { return v_.begin(); }
    iterator end() { return v_.end(); }
    const_iterator begin() const { return v_.begin(); }
    const_iterator end() const { return v_.end(); }
    const std::vector<T> &AsGenomicRegionVector() const { return v_; }

#ifdef SEQLIB_GRC_QUERIES
    // ---- single queries (host)
    // the ids (positions in this collection) of the intervals gr overlaps
    template <class K> std::vector<int> FindOverlappedIntervals(const K &gr, bool ignore_strand) const
    {
        need_tree();
        const Hits h = query(gr, ignore_strand, false);
        return std::vector<int>(h.id.begin(), h.id.end());
    }
    // the overlapping intervals, trimmed to lie inside gr
    template <class K> GenomicRegionCollection<GenomicRegion> FindOverlaps(const K &gr, bool ignore_strand) const
    {
        need_tree();
        GenomicRegionCollection<GenomicRegion> out;
        const Hits h = query(gr, ignore_strand, false);
        for (size_t k = 0; k < h.id.size(); ++k) out.add(GenomicRegion(gr.chr, h.p1[k], h.p2[k]));
        return out;
    }
    // positions of gr covered by the collection
    template <class K> size_t FindOverlapWidth(const K &gr, bool ignore_strand) const
    {
        need_tree();
        return (size_t)query(gr, ignore_strand, false).width;
    }
    size_t CountOverlaps(const T &gr) const
    {
        if (warn_no_tree()) return 0;
        return query(gr, true, false).id.size();
    }
    // intervals of the collection that lie inside gr (IntervalTree.h:224)
    size_t CountContained(const T &gr)
    {
        if (warn_no_tree()) return 0;
        return query(gr, true, true).id.size();
    }
    template <class K> bool OverlapSameInterval(const K &gr1, const K &gr2) const
    {
        if (gr1.chr != gr2.chr) return false;
        if (warn_no_tree()) return false;
        const Hits a = query(gr1, true, false), b = query(gr2, true, false);
        for (int32_t x : a.id)
            if (std::find(b.id.begin(), b.id.end(), x) != b.id.end()) return true;
        return false;
    }

    // ---- batches (GPU)
    // This collection's intervals as queries against subject's index: for every hit the query's and the subject's position (appended), and the subject interval
    // trimmed to the query.  Queries in order, a query's hits by ascending (pos1, pos2, id).
    template <class K>
    GenomicRegionCollection<GenomicRegion> FindOverlaps(const GenomicRegionCollection<K> &subject, std::vector<int32_t> &query_id, std::vector<int32_t> &subject_id, bool ignore_strand) const
    {
        GenomicRegionCollection<GenomicRegion> output;
        if (subject.NumTree() == 0 && subject.size() != 0) {
            std::cerr << "!!!!!! findOverlaps: WARNING: Trying to find overlaps on empty tree. Need to run this->CreateTreeMap() somewhere " << std::endl;
            return output;
        }
        if (!subject.tree_ || v_.empty()) return output;
        if (subject.size() < v_.size() && v_.size() - subject.size() > 20) std::cerr << "findOverlaps warning: Suggest switching query and subject for efficiency." << std::endl;
        const std::vector<slx_grc_iv> q = as_ivs(v_);
        slx_grc_result r;
        check(slx_grc_overlaps(subject.tree(), q.data(), (int64_t)q.size(), ignore_strand ? 1 : 0, &r), "FindOverlaps");
        try {
            for (int64_t k = 0; k < r.n_pairs; ++k) {
                query_id.push_back(r.query_id[k]);
                subject_id.push_back(r.subject_id[k]);
                output.add(GenomicRegion(v_[(size_t)r.query_id[k]].chr, r.pos1[k], r.pos2[k]));
            }
        } catch (...) { slx_grc_result_free(&r); throw; }
        slx_grc_result_free(&r);
        return output;
    }
    template <class K> GenomicRegionCollection<GenomicRegion> Intersection(const GenomicRegionCollection<K> &subject, bool ignore_strand) const
    {
        std::vector<int32_t> sub, que;
        if (subject.size() > size()) return FindOverlaps(subject, que, sub, ignore_strand);
        return subject.FindOverlaps(*this, que, sub, ignore_strand);
    }

    // Every record the reader still has, batch by batch from HBM, against this collection's index: for every hit the record's number (in the order served by this
    // call) and the interval's id; clipped (may be null) takes the interval trimmed to the record's (ChrID, Position, PositionEnd).  Returns the records seen.
    // The per-interval record counts accumulate (SubjectCounts).
    template <class Reader>
    size_t OverlapReads(Reader &rd, std::vector<int64_t> &read_id, std::vector<int32_t> &subject_id, GenomicRegionCollection<GenomicRegion> *clipped = nullptr)
    {
        return drain(rd, &read_id, &subject_id, clipped);
    }
    // the same without the pairs: the counts only
    template <class Reader> size_t CountReads(Reader &rd) { return drain(rd, nullptr, nullptr, nullptr); }
    // one batch in HBM (slx_bam_batch, slx_rec_batch: d_stream, n_bytes, d_rec_off, n_records); read_id counts from first_read
    template <class Batch>
    size_t OverlapBatch(const Batch &b, std::vector<int64_t> *read_id, std::vector<int32_t> *subject_id, GenomicRegionCollection<GenomicRegion> *clipped = nullptr, int64_t first_read = 0)
    {
        need_tree();
        if (!tree_) return 0;
        join_records(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records, first_read, read_id, subject_id, clipped);
        return (size_t)b.n_records;
    }
    // per interval (by position in this collection): the records so far that overlap it
    std::vector<int64_t> SubjectCounts() const
    {
        need_tree();
        std::vector<int64_t> out(tree_ ? v_.size() : 0);
        if (tree_) check(slx_grc_subject_counts(tree(), out.data()), "SubjectCounts");
        return out;
    }
    void ClearCounts() { if (tree_) check(slx_grc_clear_counts(tree()), "ClearCounts"); }
    // knobs and diagnostics of the C-ABI by name (slx_grc_set, slx_grc_counter)
    bool SetKnob(const char *key, int64_t v) { return tree_ && slx_grc_set(tree(), key, v) == SLX_OK; }
    int64_t Counter(const char *name) const { return tree_ ? slx_grc_counter(tree(), name) : -1; }

#endif
    // ---- host only
    int TotalWidth() const
    {
        int wid = 0;
        for (const_iterator i = v_.begin(); i != v_.end(); ++i) wid += i->Width();
        return wid;
    }
    void Pad(int v) { for (iterator i = v_.begin(); i != v_.end(); ++i) i->Pad(v); }
    void Concat(const GenomicRegionCollection<T> &g)
    {
        if (!g.size()) return;
        m_sorted = false;
        v_.insert(v_.end(), g.v_.begin(), g.v_.end());
    }
    std::string AsBEDString(const BamHeader &h) const
    {
        std::stringstream ss;
        for (const_iterator i = v_.begin(); i != v_.end(); ++i) ss << i->ChrName(h) << "\t" << i->pos1 << "\t" << i->pos2 << "\t" << i->strand << std::endl;
        return ss.str();
    }
    // sorted, and every interval stretched right to the one before the next one's start; the last one to max (0: left as it is)
    void SortAndStretchRight(int max)
    {
        if (v_.empty()) return;
        CoordinateSort();
        if (max > 0 && max < v_.back().pos2) throw std::out_of_range("GenomicRegionCollection::SortAndStrech Can't stretch to max, as we are already past max.");
        for (size_t i = 0; i + 1 < v_.size(); ++i) v_[i].pos2 = v_[i + 1].pos1 - 1;
        if (max > 0) v_.back().pos2 = max;
    }
    // sorted, the first one's start set to min (< 0: left as it is) and every other one's to one past the end of the one before.  The reference's check is kept as
    // it is written (GenomicRegionCollection.cpp:110): out_of_range when min lies BEFORE the first start, although its comment says the opposite
    void SortAndStretchLeft(int min)
    {
        if (v_.empty()) return;
        CoordinateSort();
        if (min >= 0 && min < v_.front().pos1) throw std::out_of_range("GenomicRegionCollection::SortAndStrechLeft - Can't stretch to min, as we are already below min");
        if (min >= 0) v_[0].pos1 = min;
        for (size_t i = 1; i < v_.size(); ++i) v_[i].pos1 = v_[i - 1].pos2 + 1;
    }

    // the size, the first three, an ellipsis if there are more than six, the last three
    friend std::ostream &operator<<(std::ostream &os, const GenomicRegionCollection &grc)
    {
        const size_t n = grc.size(), head = std::min<size_t>(3, n);
        os << "GenomicRegionCollection(size=" << n << ")";
        if (n == 0) return os;
        os << " [";
        for (size_t i = 0; i < head; ++i) os << grc.v_[i] << (i + 1 < head ? ", " : "");
        if (n > 2 * head) {
            os << ", ... ";
            for (size_t i = n - head; i < n; ++i) os << grc.v_[i] << (i + 1 < n ? ", " : "");
        } else if (n > head) {
            os << ", ";
            for (size_t i = head; i < n; ++i) os << grc.v_[i] << (i + 1 < n ? ", " : "");
        }
        return os << "]";
    }

private:
#ifdef SEQLIB_GRC_QUERIES
    struct Hits { std::vector<int32_t> id, p1, p2; int64_t width = 0; };

    // SLX_EINVAL is the caller's interval (pos2 < pos1); anything else is the library's or the device's
    static void check(int rc, const char *who)
    {
        if (rc == SLX_OK) return;
        const std::string msg = std::string("GenomicRegionCollection::") + who + " - " + slx_last_error();
        if (rc == SLX_EINVAL) throw std::invalid_argument(msg);
        throw std::runtime_error(msg);
    }
    template <class V> static std::vector<slx_grc_iv> as_ivs(const V &v)
    {
        std::vector<slx_grc_iv> out(v.size());
        for (size_t i = 0; i < v.size(); ++i) { std::memset(&out[i], 0, sizeof out[i]); out[i].chr = v[i].chr; out[i].pos1 = v[i].pos1; out[i].pos2 = v[i].pos2; out[i].strand = v[i].strand; }
        return out;
    }
    slx_grc *tree() const { return static_cast<slx_grc *>(tree_.get()); }
    static std::shared_ptr<void> make_tree(const std::vector<T> &v)
    {
        const std::vector<slx_grc_iv> iv = as_ivs(v);
        slx_grc *g = nullptr;
        check(slx_grc_create(SLX_GRC_AUTO, iv.data(), (int64_t)iv.size(), &g), "CreateTreeMap");
        return std::shared_ptr<void>(g, [](void *p) { slx_grc_free(static_cast<slx_grc *>(p)); });
    }
    void need_tree() const
    {
        if (!tree_ && !v_.empty()) throw std::logic_error("Need to run CreateTreeMap to make the interval tree before doing range queries");
    }
    bool warn_no_tree() const
    {
        if (tree_) return false;
        if (!v_.empty()) std::cerr << "!!!!!! WARNING: Trying to find overlaps on empty tree. Need to run this->CreateTreeMap() somewhere " << std::endl;
        return true;
    }
    template <class K> Hits query(const K &gr, bool ignore_strand, bool contained) const
    {
        Hits h;
        if (!tree_) return h;
        slx_grc_iv q;
        std::memset(&q, 0, sizeof q);
        q.chr = gr.chr; q.pos1 = gr.pos1; q.pos2 = gr.pos2; q.strand = gr.strand;
        int64_t n = 0;
        check(slx_grc_query_host(tree(), &q, ignore_strand ? 1 : 0, contained ? 1 : 0, nullptr, nullptr, nullptr, 0, &n, nullptr), "FindOverlaps");
        h.id.resize((size_t)n); h.p1.resize((size_t)n); h.p2.resize((size_t)n);
        if (n) check(slx_grc_query_host(tree(), &q, ignore_strand ? 1 : 0, contained ? 1 : 0, h.id.data(), h.p1.data(), h.p2.data(), n, &n, &h.width), "FindOverlaps");
        return h;
    }
    bool read_lines(const std::string &file, const char *what, const std::function<void(const std::string &)> &take)
    {
        gzFile fp = file.empty() ? nullptr : file != "-" ? gzopen(file.c_str(), "r") : gzdopen(fileno(stdin), "r");
        if (!fp) { std::cerr << what << " file not readable: " << file << std::endl; return false; }
        std::vector<char> buf(65472);
        std::string line;
        while (gzgets(fp, buf.data(), (int)buf.size())) {
            line += buf.data();
            if (!line.empty() && line.back() != '\n' && !gzeof(fp)) continue;          // a line longer than the buffer: more of it follows
            while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
            take(line);
            line.clear();
        }
        int err = 0;
        const char *msg = gzerror(fp, &err);
        const bool ok = err == Z_OK || err == Z_STREAM_END;
        if (!ok) std::cerr << what << " file " << file << ": " << msg << std::endl;
        gzclose(fp);
        return ok;
    }
    void join_records(const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, int64_t first_read, std::vector<int64_t> *read_id, std::vector<int32_t> *subject_id,
                      GenomicRegionCollection<GenomicRegion> *clipped)
    {
        const bool pairs = read_id || subject_id || clipped;
        if (!pairs) { check(slx_grc_overlaps_device(tree(), d_stream, n_bytes, d_rec_off, n_records, 0, nullptr), "CountReads"); return; }
        slx_grc_result r;
        check(slx_grc_overlaps_device(tree(), d_stream, n_bytes, d_rec_off, n_records, 1, &r), "OverlapReads");
        try {
            for (int64_t k = 0; k < r.n_pairs; ++k) {
                if (read_id) read_id->push_back(first_read + r.query_id[k]);
                if (subject_id) subject_id->push_back(r.subject_id[k]);
                if (clipped) clipped->add(GenomicRegion(v_[(size_t)r.subject_id[k]].chr, r.pos1[k], r.pos2[k]));
            }
        } catch (...) { slx_grc_result_free(&r); throw; }
        slx_grc_result_free(&r);
    }
    template <class Reader>
    size_t drain(Reader &rd, std::vector<int64_t> *read_id, std::vector<int32_t> *subject_id, GenomicRegionCollection<GenomicRegion> *clipped)
    {
        if (!rd.rd_) throw std::runtime_error("GenomicRegionCollection::OverlapReads - the reader is not open");
        need_tree();
        size_t n = 0;
        while (rd.advance()) {
            const int64_t k = rd.batch_.n_records - (int64_t)rd.cur_;
            if (tree_) join_records(rd.batch_.d_stream, rd.batch_.n_bytes, (const uint64_t *)rd.batch_.d_rec_off + rd.cur_, k, (int64_t)n, read_id, subject_id, clipped);
            rd.cur_ = (size_t)rd.batch_.n_records;
            n += (size_t)k;
        }
        return n;
    }

#endif
    std::vector<T> v_;
    bool m_sorted = false;
    size_t idx_ = 0;
    std::shared_ptr<void> tree_;          // the index CreateTreeMap built (an slx_grc); null before, and after clear / MergeOverlappingIntervals.  Held untyped so
                                          // that the object has one layout with and without SEQLIB_GRC_QUERIES
};

typedef GenomicRegionCollection<GenomicRegion> GRC;

}  // namespace SeqLib
