// BamReader.h -- SeqLib::BamReader for the MI355X drop-in: the producer in front of BWAAligner and FermiAssembler.
// Same names, signatures and return conventions as /root/reference/SeqLib/BamReader.h:16-76 and /root/reference/src/BamReader.cpp:10-151 (Open / Close /
// Reset / Next / Header / IsOpen / operator<<; false instead of exceptions, messages on stderr, Header() throws before Open as the reference does).
// The reference hands the file to htslib (hts_open / sam_hdr_read / sam_read1), which is not part of this image: here the BGZF members are inflated,
// CRC-checked and cut into records on the GPU behind include/seqlib_amd_bam.h, a batch of members at a time, and Next() serves records out of the
// current batch.  A record's bam1_t is the 32 fixed bytes plus the variable part exactly as they stand in the file, so BamWriter::WriteRecord writes
// back the bytes that were read.
// Open loads the BAI index beside the file when there is one (<path>.bai, or .bai in place of .bam; src/BamReader.cpp:33), and SetRegion(GenomicRegion) /
// SetRegions(GRC) then make Next, NextBatch and BWAAligner::alignSequences(BamReader&) serve the regions in the order given, a record once per region it
// overlaps (src/BamReader.cpp:64-137: one iterator per region): only the BGZF members the index names are inflated, and the records are tested against the
// region and compacted on the GPU.  The interval handed down is [pos1, pos2), exactly what the reference hands to sam_itr_queryi.
// New next to the reference: GetNextRecord (the README's spelling, README.md:150-181), NextBatch (many records at once through the slab path of
// BamRecord.h), SetBatchBytes, HasIndex, and SetReadFilter / ClearReadFilter: a Filter::ReadFilterCollection evaluated on the GPU, so that Next, NextBatch and
// BWAAligner::alignSequences(BamReader&) see the kept records only -- for the whole file and for regions.
// Open takes SAM text too (plain, gzip'd or bgzip'd; the reference's "BAM/SAM/CRAM", SeqLib/BamReader.h:22-26): slx_sam_sniff tells the two apart, and the lines are
// parsed into BAM records on the GPU behind include/seqlib_amd_sam.h (which lists the grammar and its deviations from htslib).  Everything after Open is the same
// code on both: Next, GetNextRecord, NextBatch, Reset, Header, SetReadFilter, BWAAligner::alignSequences(BamReader&) and alignToBam(BamReader&).  SAM text has no
// index: HasIndex() is false, SetRegion / SetRegions return false with a message.
// Refused loudly: SetRegion / SetRegions with anything but a GenomicRegion / a GRC, CRAM input, "-" (stdin), a second Open.
#pragma once
#include <cstdint>
#include <cstring>
#include <iostream>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>
#include "SeqLib/BamHeader.h"
#include "SeqLib/BamRecord.h"
#include "SeqLib/GenomicRegionCollection.h"
#include "SeqLib/ReadFilter.h"
#include "seqlib_amd_bam.h"
#include "seqlib_amd_filter.h"
#include "seqlib_amd_sam.h"

namespace SeqLib {

class BamReader {
    friend class BWAAligner;
    friend class STCoverage;          // addReads(BamReader&): the batches as they lie in HBM
    friend class BamStats;
    friend class RefGenome;           // NmMd(BamReader&): the same
    friend class RecordEditor;        // Apply(BamReader&): the same
    friend class AssemblyWindows;     // addReads(BamReader&): the same
    friend class DuplicateMarker;     // addReads(BamReader&): the same
    friend class Pileup;              // addReads(BamReader&): the same
    template <typename T> friend class GenomicRegionCollection;          // OverlapReads / CountReads(BamReader&): the same
public:
    BamReader() = default;
    BamReader(const BamReader &) = delete;
    BamReader &operator=(const BamReader &) = delete;
    ~BamReader() { Close(); }

    bool Open(const std::string &path)
    {
        if (rd_) { std::cerr << "BamReader::Open - already open ('" << path_ << "'); Close() first" << std::endl; return false; }
        if (path == "-") { std::cerr << "BamReader::Open - reading from stdin is not available in the MI355X drop-in" << std::endl; return false; }
        path_ = path;
        slx_bam *rd = nullptr;
        const bool sam = slx_sam_sniff(path.c_str()) == 1;          // (anything else, an unreadable file included, is slx_bam_open's to name)
        if ((sam ? slx_sam_open(path.c_str(), -1, &rd) : slx_bam_open(path.c_str(), -1, &rd)) != SLX_OK) {
            std::cerr << "BamReader::Open - failed to open '" << path << "': " << slx_last_error() << std::endl;
            return false;
        }
        rd_ = rd;
        const char *text = nullptr; int64_t l_text = 0; int n_ref = 0;
        slx_bam_header(rd_, &text, &l_text, &n_ref);
        // the dictionary is the binary one; the text is kept when its @SQ lines say the same
        const BamHeader from_text{std::string(text, (size_t)l_text)};
        bool same = from_text.NumSequences() == n_ref;
        HeaderSequenceVector hsv;
        for (int i = 0; i < n_ref; ++i) {
            hsv.push_back(HeaderSequence(slx_bam_ref_name(rd_, i), (uint32_t)slx_bam_ref_len(rd_, i)));
            same = same && from_text.IDtoName(i) == hsv.back().Name && from_text.GetSequenceLength(i) == (int)hsv.back().Length;
        }
        hdr_ = same ? from_text : BamHeader(hsv);
        clear_batch();
        return true;
    }
    void Close()
    {
        if (rd_) slx_bam_close(rd_);
        rd_ = nullptr;
        flt_.reset();
        hdr_ = BamHeader();
        clear_batch();
    }
    void Reset()                     // src/BamReader.cpp:56-62 closes and opens again; the member table and the header are kept here
    {
        if (!rd_) { if (!path_.empty()) Open(path_); return; }
        slx_bam_rewind(rd_);
        clear_batch();
    }
    // false when the reader is not open, has no index or the region names a reference outside the header
    bool SetRegion(const GenomicRegion &gr)
    {
        if (!rd_ || no_index_in_sam("SetRegion") || !HasIndex()) return false;
        const slx_bam_region r = {gr.chr, gr.pos1, gr.pos2};
        return arm(&r, 1);
    }
    bool SetRegions(const GRC &grc)
    {
        if (!rd_ || no_index_in_sam("SetRegions") || !HasIndex() || !grc.size()) return false;
        std::vector<slx_bam_region> r;
        for (const GenomicRegion &g : grc) r.push_back(slx_bam_region{g.chr, g.pos1, g.pos2});
        return arm(r.data(), (int64_t)r.size());
    }
    bool HasIndex() const { return rd_ && slx_bam_has_index(rd_) != 0; }
    bool IsSAM() const { return rd_ && slx_bam_counter(rd_, "sam") == 1; }          // new next to the reference: the open file is SAM text
    template <class Region> bool SetRegion(const Region &)
    {
        std::cerr << "BamReader::SetRegion - region iteration needs a BAI index and GenomicRegion; not available in the MI355X drop-in for this argument type (pass a SeqLib::GenomicRegion)" << std::endl;
        return false;
    }
    template <class Regions> bool SetRegions(const Regions &)
    {
        std::cerr << "BamReader::SetRegions - region iteration needs a BAI index and GenomicRegion; not available in the MI355X drop-in for this argument type (pass a SeqLib::GRC)" << std::endl;
        return false;
    }
    bool SetCramReference(const std::string &) { std::cerr << "BamReader::SetCramReference - CRAM input is not available in the MI355X drop-in" << std::endl; return false; }

    // From the next batch on the reader serves only the records the collection keeps: every batch is evaluated and compacted in HBM (include/seqlib_amd_filter.h).
    // The reader holds the compiled collection; rules added to fc afterwards take effect with the next SetReadFilter.  false when the reader is not open.
    bool SetReadFilter(const Filter::ReadFilterCollection &fc)
    {
        if (!rd_) return false;
        std::shared_ptr<slx_filter> h = fc.Handle();
        if (slx_filter_attach(h.get(), rd_) != SLX_OK) { std::cerr << "BamReader::SetReadFilter - " << slx_last_error() << std::endl; return false; }
        flt_ = h;
        return true;
    }
    void ClearReadFilter()
    {
        if (rd_) slx_filter_attach(nullptr, rd_);
        flt_.reset();
    }

    std::optional<BamRecord> Next()
    {
        if (!rd_ || !advance()) return std::nullopt;
        const uint8_t *p = batch_.stream + batch_.rec_off[cur_++];
        bam1_t *r = bam_init1();
        if (!r) throw std::bad_alloc();
        const size_t l_data = blob_bytes(p);
        r->data = static_cast<uint8_t *>(std::malloc(l_data ? l_data : 1));
        if (!r->data) { bam_destroy1(r); throw std::bad_alloc(); }
        fill(r, p, l_data);
        return BamRecord(r);
    }
    bool GetNextRecord(BamRecord &r)
    {
        std::optional<BamRecord> n = Next();
        if (!n) return false;
        r = std::move(*n);
        return true;
    }
    // up to max_records records appended to out; returns how many.  Large requests carve the records out of slabs (BamRecord.h).
    size_t NextBatch(BamRecordPtrVector &out, size_t max_records)
    {
        size_t got = 0;
        detail::SlabWriter writer;
        const bool slabs = max_records >= 1024;
        while (got < max_records && rd_ && advance()) {
            const size_t take = std::min(max_records - got, (size_t)batch_.n_records - cur_);
            out.reserve(out.size() + take);
            for (size_t i = 0; i < take; ++i) out.push_back(make_ptr(batch_.stream + batch_.rec_off[cur_ + i], slabs ? &writer : nullptr));
            cur_ += take; got += take;
        }
        return got;
    }
    const BamHeader &Header() const
    {
        if (!rd_) throw std::runtime_error("BamReader::Header() called before Open()");
        return hdr_;
    }
    bool IsOpen() const { return rd_ != nullptr; }
    // inflated bytes per batch of members (default 64 MiB)
    void SetBatchBytes(int64_t b) { if (b > 0) batch_bytes_ = b; }
    // diagnostics of the C-ABI by name (slx_bam_counter)
    int64_t Counter(const char *name) const { return rd_ ? slx_bam_counter(rd_, name) : -1; }
    bool SetKnob(const char *key, int64_t v) { return rd_ && slx_bam_set(rd_, key, v) == SLX_OK; }

    friend std::ostream &operator<<(std::ostream &out, const BamReader &b)
    {
        out << ": " << b.path_ << '\n' << " - BamReader - Walking whole genome -\n" << " ------------------------------------";
        return out;
    }

private:
    static uint32_t u32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
    static uint16_t u16(const uint8_t *p) { uint16_t v; std::memcpy(&v, p, 2); return v; }
    static size_t blob_bytes(const uint8_t *p) { return (size_t)u32(p) - 32; }          // (the C-ABI refuses a block_size below the fixed part)
    // p: the record in the stream, its block_size word first; r->data holds l_data bytes
    static void fill(bam1_t *r, const uint8_t *p, size_t l_data)
    {
        bam1_core_t &c = r->core;
        c.tid = (int32_t)u32(p + 4); c.pos = (int32_t)u32(p + 8);
        c.l_qname = p[12]; c.qual = p[13]; c.bin = u16(p + 14); c.n_cigar = u16(p + 16); c.flag = u16(p + 18);
        c.l_qseq = (int32_t)u32(p + 20); c.mtid = (int32_t)u32(p + 24); c.mpos = (int32_t)u32(p + 28); c.isize = (int32_t)u32(p + 32);
        c.l_extranul = 0;
        std::memcpy(r->data, p + 36, l_data);
        r->l_data = (int)l_data; r->m_data = (uint32_t)l_data;
    }
    static BamRecordPtr make_ptr(const uint8_t *p, detail::SlabWriter *sw)
    {
        const size_t l_data = blob_bytes(p);
        if (!sw) {
            bam1_t *r = bam_init1();
            if (!r) throw std::bad_alloc();
            r->data = static_cast<uint8_t *>(std::malloc(l_data ? l_data : 1));
            if (!r->data) { bam_destroy1(r); throw std::bad_alloc(); }
            fill(r, p, l_data);
            return std::make_shared<BamRecord>(r);
        }
        detail::Slab *slab = sw->ensure(l_data + 384);          // the blob + the two shells with their control blocks (as BWAAligner::make_record)
        auto box = std::allocate_shared<Bam1Box>(detail::SlabAlloc<Bam1Box>(slab));
        bam1_t *r = &box->b;
        r->data = static_cast<uint8_t *>(slab->take(l_data ? l_data : 1));
        slab->retain();
        box->slab = slab;
        r->mempolicy = BAM_USER_OWNS_DATA;
        fill(r, p, l_data);
        return std::allocate_shared<BamRecord>(detail::SlabAlloc<BamRecord>(slab), std::shared_ptr<bam1_t>(box, r));
    }
    bool no_index_in_sam(const char *who) const
    {
        if (!IsSAM()) return false;
        std::cerr << "BamReader::" << who << " - '" << path_ << "' is SAM text, which has no index: region iteration is not available on it" << std::endl;
        return true;
    }
    void clear_batch() { std::memset(&batch_, 0, sizeof batch_); cur_ = 0; eof_ = false; }
    bool arm(const slx_bam_region *r, int64_t n)
    {
        if (slx_bam_set_regions(rd_, r, n) != SLX_OK) { std::cerr << "BamReader::SetRegion - " << slx_last_error() << std::endl; return false; }
        clear_batch();
        return true;
    }
    // makes batch_[cur_] a record: fetches the next batch when the current one is used up; false at the end of the file or on an error (message on stderr)
    bool advance()
    {
        if (cur_ < (size_t)batch_.n_records) return true;
        if (eof_) return false;
        return fetch(batch_) && batch_.n_records > 0;
    }
    // the next batch of the C-ABI, for BWAAligner::alignSequences(BamReader&) too
    bool fetch(slx_bam_batch &b)
    {
        cur_ = 0;
        if (slx_bam_next(rd_, batch_bytes_, &b) != SLX_OK) {
            std::cerr << "BamReader::Next - " << slx_last_error() << std::endl;
            std::memset(&batch_, 0, sizeof batch_);
            eof_ = true;
            return false;
        }
        if (b.n_records == 0) eof_ = true;
        return true;
    }

    std::string path_;
    slx_bam *rd_ = nullptr;
    std::shared_ptr<slx_filter> flt_;          // the attached read filter, alive as long as the reader uses it
    BamHeader hdr_;
    slx_bam_batch batch_ = {};
    size_t cur_ = 0;
    bool eof_ = false;
    int64_t batch_bytes_ = (int64_t)64 << 20;
};

}  // namespace SeqLib
