// RecordEditor.h -- new next to the reference: the reference edits records one BamRecord at a time (RemoveTag, RemoveAllTags, AddZTag, AddIntTag,
// ClearSeqQualAndTags); this class fixes such a sequence of edits as a plan and applies it to a whole batch of records where it lies in HBM
// (slx_edit_*, include/seqlib_amd_edit.h, where the rules are written down).  The result is a device batch again: BamWriter::WriteDevice(d, n, d_rec_off,
// n_records) takes it unchanged, and so do the sorter, coverage, statistics, intervals and RefGenome.
//
//     RecordEditor ed;                                  // instead of:  while (auto r = reader.Next()) {
//     ed.DropTag("XA"); ed.AddZTag("RG", "grp1");       //                  r->RemoveTag("XA"); r->AddZTag("RG", "grp1");
//     while (ed.Apply(reader)) writer.WriteDevice(ed.Batch().d_stream, ed.Batch().n_bytes, ed.Batch().d_rec_off, ed.Batch().n_records);     //   writer.WriteRecord(*r); }
//
// A record the host loop would walk with a clamped field (hts_compat.h, bam_aux_skip) is refused here: the aux area must parse exactly to the record's end.
#pragma once
#include <stdexcept>
#include <string>
#include "SeqLib/BamReader.h"
#include "seqlib_amd_edit.h"

namespace SeqLib {

class RecordEditor {
    friend class RefGenome;          // WriteNmMd binds the NM and MD columns
public:
    explicit RecordEditor(int device = SLX_EDIT_AUTO) { check(slx_edit_create(device, &e_), "RecordEditor"); }
    ~RecordEditor() { if (e_) slx_edit_free(e_); }
    RecordEditor(const RecordEditor &) = delete;
    RecordEditor &operator=(const RecordEditor &) = delete;

    // ---- the plan (std::invalid_argument with the library's sentence for what it refuses)
    void ClearPlan() { check(slx_edit_plan_clear(e_), "ClearPlan"); }
    void DropTag(const std::string &tag) { check(slx_edit_drop_tag(e_, tag.c_str()), "DropTag"); }
    void DropAllTags() { check(slx_edit_drop_all_tags(e_), "DropAllTags"); }
    void ClearSeqQualAndTags() { check(slx_edit_clear_seq_qual(e_), "ClearSeqQualAndTags"); }
    void AddZTag(const std::string &tag, const std::string &value) { check(slx_edit_add_z(e_, tag.c_str(), value.data(), (int64_t)value.size()), "AddZTag"); }
    void AddIntTag(const std::string &tag, int32_t v, bool replace = false) { check(slx_edit_add_int(e_, tag.c_str(), v, replace ? 1 : 0), "AddIntTag"); }
    void SetKnob(const char *key, int64_t v) { check(slx_edit_set(e_, key, v), "SetKnob"); }
    int64_t Counter(const char *name) const { return slx_edit_counter(e_, name); }

    // Edits the rest of the batch the reader serves next (SetRegions and SetReadFilter are honoured; what Next() has handed out of it already is left out), which
    // is then used up; false at the end of the file.
    bool Apply(BamReader &rd)
    {
        if (!rd.rd_) throw std::runtime_error("RecordEditor::Apply - the reader is not open");
        if (!rd.advance()) { out_ = slx_edit_batch{}; return false; }
        const slx_bam_batch &b = rd.batch_;
        const uint64_t first = b.rec_off[rd.cur_];          // (the offsets count from the first one given: the stream moves up by as much)
        Apply((const uint8_t *)b.d_stream + first, b.n_bytes - (int64_t)first, (const uint64_t *)b.d_rec_off + rd.cur_, b.n_records - (int64_t)rd.cur_);
        rd.cur_ = (size_t)b.n_records;
        return true;
    }
    // ... any device batch: a builder's (slx_rec_batch), another editor's, a sorter's
    void Apply(const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n_records)
    {
        out_ = slx_edit_batch{};
        const int rc = slx_edit_apply_device(e_, d_stream, n_bytes, d_rec_off, n_records, &out_);
        if (rc != SLX_OK) throw std::runtime_error(std::string("RecordEditor::Apply - ") + slx_last_error());
    }
    // the last result; valid until the next Apply
    const slx_edit_batch &Batch() const { return out_; }
    slx_edit *raw() const { return e_; }

private:
    static void check(int rc, const char *who)
    {
        if (rc == SLX_EINVAL) throw std::invalid_argument(std::string("RecordEditor::") + who + " - " + slx_last_error());
        if (rc != SLX_OK) throw std::runtime_error(std::string("RecordEditor::") + who + " - " + slx_last_error());
    }
    slx_edit *e_ = nullptr;
    slx_edit_batch out_ = {};
};

}  // namespace SeqLib
