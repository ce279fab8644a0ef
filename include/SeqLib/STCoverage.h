// STCoverage.h -- SeqLib::STCoverage for the MI355X drop-in: per-base depth of coverage, kept in HBM behind include/seqlib_amd_cov.h.
// The reference class is src/non_api/STCoverage.{h,cpp}; it is orphaned there (ToBedgraph prints a vector addRead never fills), so its interface and addRead's
// interval arithmetic (src/non_api/STCoverage.cpp:44-109) are kept and the rest is defined by seqlib_amd_cov.h, which lists every rule with both kept quirks:
//   addRead(r, buff, false)   positions pos + buff .. end - buff, end INCLUDED (one past the last aligned base); addRead(r, *, true) extends over a leading and a
//                             trailing soft clip, looking at the first and the last op only.  No flag is tested, as in the reference.
// The reference's unordered-map storage and its uint16 vector are not carried: depth is one int32 per reference base (12.4 GB of HBM for GRCh38), or per base of
// the window for STCoverage(GenomicRegion).  The window is [pos1, pos2), what BamReader::SetRegion hands down for the same GenomicRegion.
// New next to the reference, and the reason for the GPU: addReads(BamReader&) drains a reader batch by batch without a host round trip (SetRegions and
// SetReadFilter are honoured; a record served once per region it overlaps is counted once per region), addBatch takes the records alignToBam's builder left in
// HBM, SetMode(SLX_COV_ALIGNED) counts what `samtools depth` counts, RegionSums gives per-region sums.  A C-ABI failure is a std::runtime_error.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <unistd.h>
#include <vector>
#include "SeqLib/BamHeader.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/BamRecord.h"
#include "SeqLib/GenomicRegionCollection.h"
#include "seqlib_amd_cov.h"
#include "seqlib_amd_rec.h"

namespace SeqLib {

class STCoverage {
public:
    STCoverage() = default;                                                   // all contigs: SetHeader before the first add (addReads takes the reader's)
    explicit STCoverage(const GenomicRegion &gr) : gr_(gr), windowed_(true)   // one window; without SetHeader the contig is taken to end at the window's end
    {
        if (gr.chr < 0) throw std::invalid_argument("STCoverage - the window names no contig");
    }
    STCoverage(const STCoverage &) = delete;
    STCoverage &operator=(const STCoverage &) = delete;
    ~STCoverage() { if (cov_) slx_cov_free(cov_); }

    // the contigs; what was counted so far goes
    void SetHeader(const BamHeader &h)
    {
        std::vector<int64_t> len;
        std::vector<std::string> names;
        for (int i = 0; i < h.NumSequences(); ++i) { len.push_back(h.GetSequenceLength(i)); names.push_back(h.IDtoName(i)); }
        create(len, &names);
    }
    // SLX_COV_SPAN / SLX_COV_FULL / SLX_COV_ALIGNED for every later add, whatever its full_length says; -1 (the default): full_length decides between SPAN and FULL
    void SetMode(int mode) { flush(); mode_ = mode; }
    void SetMinMapq(int q) { flush(); min_mapq_ = q; }
    void SetExcludeFlags(uint32_t f) { flush(); exclude_ = f; }                // default 0: the reference's addRead tests no flag
    void SetCountDeletions(bool on) { flush(); count_del_ = on; }
    void SetKnob(const char *key, int64_t v) { need(); check(slx_cov_set(cov_, key, v)); }
    int64_t Counter(const char *name) const { return cov_ ? slx_cov_counter(cov_, name) : -1; }

    void clear()
    {
        stream_.clear(); off_.assign(1, 0);
        if (cov_) check(slx_cov_clear(cov_));
    }

    // buffered on the host; goes up through slx_cov_add_host when the buffer is full and before any read
    void addRead(const BamRecord &r, int buff, bool full_length)
    {
        const bam1_t *b = r.raw();
        if (!b) return;
        need();
        if (!stream_.empty() && (buff != buf_buff_ || full_length != buf_full_)) flush();
        buf_buff_ = buff; buf_full_ = full_length;
        put_record(b);
        if (stream_.size() >= STAGE) flush();
    }
    // every record the reader still has, batch by batch, from HBM to HBM; returns how many were handed over
    size_t addReads(BamReader &rd, int buff, bool full_length)
    {
        if (!rd.rd_) throw std::runtime_error("STCoverage::addReads - the reader is not open");
        if (!cov_ && !have_header_) SetHeader(rd.Header());
        flush();
        apply(buff, full_length);
        size_t n = 0;
        while (rd.advance()) {
            const slx_bam_batch &b = rd.batch_;
            const int64_t k = b.n_records - (int64_t)rd.cur_;
            check(slx_cov_add_device(cov_, b.d_stream, b.n_bytes, (const uint64_t *)b.d_rec_off + rd.cur_, k));
            rd.cur_ = (size_t)b.n_records;
            n += (size_t)k;
        }
        return n;
    }
    // the records a builder left in HBM (slx_rec_build*, BWAAligner::alignToBam)
    void addBatch(const slx_rec_batch &b, int buff, bool full_length)
    {
        flush();
        apply(buff, full_length);
        check(slx_cov_add_device(cov_, b.d_stream, b.n_bytes, b.d_rec_off, b.n_records));
    }

    void settleCoverage() { flush(); if (cov_ && n_ref_) check(slx_cov_depth(cov_, 0, 0, 0, nullptr)); }
    int maxCov() { flush(); need(); return (int)value(slx_cov_max(cov_, -1)); }
    int getCoverageAtPosition(int chr, int pos) { flush(); need(); return (int)value(slx_cov_at(cov_, chr, pos)); }
    // depth of [beg, end) of contig chr, 0 outside the contig or window
    std::vector<int32_t> Depth(int chr, int64_t beg, int64_t end)
    {
        flush(); need();
        std::vector<int32_t> v((size_t)(end > beg ? end - beg : 0));
        check(slx_cov_depth(cov_, chr, beg, end > beg ? end : beg, v.data()));
        return v;
    }
    // per region [pos1, pos2) (BamReader::SetRegion's interval): the sum of depth and the positions with depth >= min_depth
    void RegionSums(const GRC &grc, int min_depth, std::vector<int64_t> &sum, std::vector<int64_t> &n_at_least)
    {
        flush(); need();
        std::vector<slx_bam_region> r;
        for (const GenomicRegion &g : grc) r.push_back(slx_bam_region{g.chr, g.pos1, g.pos2});
        sum.assign(r.size(), 0); n_at_least.assign(r.size(), 0);
        check(slx_cov_regions(cov_, r.data(), (int64_t)r.size(), min_depth, sum.data(), n_at_least.data()));
    }
    // bedGraph of every contig (or window): runs of depth > 0, or all runs with include_zero
    void ToBedgraph(const std::string &path, bool include_zero = false) { flush(); need(); check(slx_cov_bedgraph(cov_, -1, include_zero ? 1 : 0, path.c_str())); }
    // The reference's form (it takes a bam_hdr_t*; htslib is not part of this image).  The text is made on the GPU into a temporary file and copied into *o.  The
    // names are those of SetHeader; h is taken when none was set and nothing has been added yet.
    void ToBedgraph(std::ofstream *o, const BamHeader &h)
    {
        if (!o) throw std::invalid_argument("STCoverage::ToBedgraph - null stream");
        if (!cov_ && !have_header_ && !windowed_) SetHeader(h);
        const char *dir = std::getenv("TMPDIR");
        std::string tmp = std::string(dir && *dir ? dir : "/tmp") + "/stcoverage_XXXXXX";
        const int fd = mkstemp(&tmp[0]);
        if (fd < 0) throw std::runtime_error("STCoverage::ToBedgraph - cannot create a temporary file");
        ::close(fd);
        try { ToBedgraph(tmp); } catch (...) { std::remove(tmp.c_str()); throw; }
        {
            std::ifstream in(tmp, std::ios::binary);
            if (in.peek() != std::ifstream::traits_type::eof()) (*o) << in.rdbuf();
        }
        std::remove(tmp.c_str());
    }

private:
    static const size_t STAGE = (size_t)8 << 20;
    void check(int rc) const { if (rc != SLX_OK) throw std::runtime_error(std::string("STCoverage - ") + slx_last_error()); }
    int64_t value(int64_t v) const { if (v < 0) check((int)v); return v; }
    void create(const std::vector<int64_t> &len, const std::vector<std::string> *names)
    {
        stream_.clear(); off_.assign(1, 0);
        if (cov_) { slx_cov_free(cov_); cov_ = nullptr; }
        std::vector<const char *> nm;
        if (names) for (const std::string &s : *names) nm.push_back(s.c_str());
        const slx_bam_region w = {gr_.chr, gr_.pos1, gr_.pos2};
        check(slx_cov_create(-1, (int)len.size(), len.data(), names ? nm.data() : nullptr, windowed_ ? &w : nullptr, &cov_));
        n_ref_ = (int)len.size();
        have_header_ = true;
    }
    // the object, made on first use: of the header, or for a window without one of a contig that ends where the window ends
    void need()
    {
        if (cov_) return;
        if (!windowed_) throw std::runtime_error("STCoverage - SetHeader() before the first read: the contigs are not known");
        std::vector<int64_t> len((size_t)gr_.chr + 1, 0);
        len[(size_t)gr_.chr] = gr_.pos2;
        create(len, nullptr);
    }
    void apply(int buff, bool full_length)
    {
        need();
        check(slx_cov_set(cov_, "mode", mode_ >= 0 ? mode_ : full_length ? SLX_COV_FULL : SLX_COV_SPAN));
        check(slx_cov_set(cov_, "buff", buff));
        check(slx_cov_set(cov_, "min_mapq", min_mapq_));
        check(slx_cov_set(cov_, "exclude_flags", exclude_));
        check(slx_cov_set(cov_, "count_del", count_del_ ? 1 : 0));
    }
    void flush()
    {
        if (off_.size() <= 1) return;
        apply(buf_buff_, buf_full_);
        const int rc = slx_cov_add_host(cov_, stream_.data(), (int64_t)stream_.size(), off_.data(), (int64_t)off_.size() - 1);
        stream_.clear(); off_.assign(1, 0);
        check(rc);
    }
    void put32(uint32_t v) { const char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)}; stream_.append(b, 4); }
    void put_record(const bam1_t *b)          // the record as it stands in a BAM file (the bin is not looked at by the unit)
    {
        const bam1_core_t &c = b->core;
        put32((uint32_t)(32 + b->l_data));
        put32((uint32_t)c.tid); put32((uint32_t)c.pos);
        put32((uint32_t)c.bin << 16 | (uint32_t)c.qual << 8 | (uint32_t)(c.l_qname & 0xff));
        put32((uint32_t)c.flag << 16 | (uint32_t)(c.n_cigar & 0xffff));
        put32((uint32_t)c.l_qseq); put32((uint32_t)c.mtid); put32((uint32_t)c.mpos); put32((uint32_t)c.isize);
        stream_.append((const char *)b->data, (size_t)b->l_data);
        off_.push_back(stream_.size());
    }

    slx_cov *cov_ = nullptr;
    GenomicRegion gr_;
    bool windowed_ = false, have_header_ = false;
    int n_ref_ = 0, mode_ = -1, min_mapq_ = 0;
    uint32_t exclude_ = 0;
    bool count_del_ = false;
    std::string stream_;
    std::vector<uint64_t> off_ = std::vector<uint64_t>(1, 0);
    int buf_buff_ = 0;
    bool buf_full_ = false;
};

}  // namespace SeqLib
