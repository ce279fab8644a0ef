// DuplicateMarker.h -- SeqLib::DuplicateMarker for the MI355X drop-in: marks duplicate reads among BAM records that lie in HBM (slx_dup_*,
// include/seqlib_amd_dup.h, which states the rules).  The reference has no duplicate marker -- its users leave the library for `samtools markdup` or Picard
// between the sort and the index -- so this class is new beside it, in the shape of STCoverage and AssemblyWindows: records go in by reader, by batch or one
// by one, each takes the next input ordinal, Finish() decides every ordinal, and Apply() rewrites bit 0x400 of a batch where it lies.  The marker keeps a
// signature per record and no record, so a file larger than HBM is marked in two passes (MarkFile does both).  BamWriter::MarkDuplicates() is the route for
// records that are on their way into a sorted file.  No CPU fallback: without a GPU the constructor throws.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "SeqLib/BamHeader.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/BamRecord.h"
#include "seqlib_amd_dup.h"
#include "seqlib_amd_rec.h"

namespace SeqLib {

class DuplicateMarker {
public:
    explicit DuplicateMarker(int device = -1) { check(slx_dup_create(device, &d_), "DuplicateMarker"); }
    ~DuplicateMarker() { if (d_) slx_dup_free(d_); }
    DuplicateMarker(const DuplicateMarker &) = delete;
    DuplicateMarker &operator=(const DuplicateMarker &) = delete;

    // the @RG lines of the header name the libraries; before the first record
    void SetHeader(const BamHeader &h)
    {
        const std::string text = h.AsString();
        check(slx_dup_set_header(d_, text.data(), (int64_t)text.size()), "SetHeader");
    }
    void SetKnob(const char *key, int64_t v) { check(slx_dup_set(d_, key, v), "SetKnob"); }
    int64_t Counter(const char *name) const { return slx_dup_counter(d_, name); }

    // Drains the reader batch by batch from HBM (SetRegions and SetReadFilter are honoured; what Next() has handed out of the current batch already is left
    // out; a record served once per region it overlaps is a record each time) -> the records taken
    size_t addReads(BamReader &rd)
    {
        if (!rd.rd_) throw std::runtime_error("DuplicateMarker::addReads - the reader is not open");
        size_t n = 0;
        while (rd.advance()) {
            const slx_bam_batch &b = rd.batch_;
            const uint64_t first = b.rec_off[rd.cur_];          // (the offsets count from the first one given: the stream moves up by as much)
            const int64_t k = b.n_records - (int64_t)rd.cur_;
            check(slx_dup_add_device(d_, (const uint8_t *)b.d_stream + first, b.n_bytes - (int64_t)first, (const uint64_t *)b.d_rec_off + rd.cur_, k), "addReads");
            rd.cur_ = (size_t)b.n_records;
            n += (size_t)k;
        }
        return n;
    }
    // the records a builder left in HBM (slx_rec_build*, BWAAligner::alignToBam)
    void addBatch(const slx_rec_batch &b) { check(slx_dup_add_device(d_, b.d_stream, b.n_bytes, b.d_rec_off, b.n_records), "addBatch"); }
    // one record from the host: uploaded, then the same kernels
    void addRead(const BamRecord &r)
    {
        if (!r.raw()) throw std::invalid_argument("DuplicateMarker::addRead - empty record");
        const std::vector<uint8_t> p = detail::packed_record(r.raw());
        const uint64_t off[2] = {0, (uint64_t)p.size()};
        check(slx_dup_add_host(d_, p.data(), (int64_t)p.size(), off, 1), "addRead");
    }

    // decides every ordinal added so far
    void Finish() { check(slx_dup_finish(d_), "Finish"); flags_.clear(); }
    // bit 0x400 of the batch's eligible records becomes the verdict, in place in HBM; record i of the batch has ordinal first_ordinal + i
    void Apply(const slx_rec_batch &b, int64_t first_ordinal) { check(slx_dup_apply_device(d_, (void *)b.d_stream, b.n_bytes, b.d_rec_off, b.n_records, first_ordinal, nullptr), "Apply"); }
    void Apply(void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records, int64_t first_ordinal)
    {
        check(slx_dup_apply_device(d_, d_stream, n_bytes, d_rec_off, n_records, first_ordinal, nullptr), "Apply");
    }
    // after Finish(): whether the record with this input ordinal is a duplicate (an ignored record never is)
    bool IsDuplicate(size_t ordinal)
    {
        if (flags_.empty()) {
            flags_.assign((size_t)slx_dup_counter(d_, "records") + 1, 0);
            check(slx_dup_flags_to_host(d_, flags_.data(), (int64_t)flags_.size()), "IsDuplicate");
        }
        if (ordinal + 1 >= flags_.size()) throw std::out_of_range("DuplicateMarker::IsDuplicate - no such ordinal");
        return flags_[ordinal] == 1;
    }
    size_t NumRecords() const { return (size_t)slx_dup_counter(d_, "records"); }

    // file to file: the header, the records and their order unchanged but for bit 0x400; the marker must be empty and holds the file's verdicts afterwards
    void MarkFile(const std::string &in, const std::string &out, int64_t batch_bytes = (int64_t)64 << 20)
    {
        check(slx_dup_file_ex(d_, in.c_str(), out.c_str(), batch_bytes), "MarkFile");
        flags_.clear();
    }
    // empties the marker and keeps its header and knobs
    void Clear() { check(slx_dup_clear(d_), "Clear"); flags_.clear(); }
    slx_dup *raw() const { return d_; }

private:
    static void check(int rc, const char *who)
    {
        if (rc == SLX_EINVAL) throw std::invalid_argument(std::string("DuplicateMarker::") + who + " - " + slx_last_error());
        if (rc != SLX_OK) throw std::runtime_error(std::string("DuplicateMarker::") + who + " - " + slx_last_error());
    }
    slx_dup *d_ = nullptr;
    std::vector<uint8_t> flags_;
};

}  // namespace SeqLib
