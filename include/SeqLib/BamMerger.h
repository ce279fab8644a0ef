// BamMerger.h -- SeqLib::BamMerger for the MI355X drop-in: several coordinate-sorted BAM files read as one, in coordinate order, or merged into one file.
// The reference's older multi-file BamReader iterated several BAMs in coordinate order on the host (a heap over one record per file); its users otherwise leave
// the library for `samtools merge`.  Here the files are read by the GPU reader and merged in HBM behind include/seqlib_amd_merge.h (which states the order, the
// header rule and the refusals), a round at a time:
//   AddFile(path)            one more input; the order of the calls breaks ties.  At most 64.
//   Header()                 the merged BamHeader: input 0's text with SO:coordinate, then the @RG / @PG / @CO lines the later inputs add
//   MergeTo(out_path)        everything into one BAM file through the GPU BGZF writer: header, records, EOF block; no file is left on an error
//   Next() / GetNextRecord   the merged iteration on the host: a round's batch is copied down and served record by record
//   NextBatch(b)             the same batch left in HBM (slx_merge_batch: stream, offsets, input of every record), for the units' add_device entries
//   SetKnob, Counter         slx_merge_set / slx_merge_counter by name
// Conventions as BamReader and BamWriter: false with a message on stderr instead of exceptions.  No fallback: without a GPU AddFile returns false.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <optional>
#include <string>
#include <utility>
#include <vector>
#include "SeqLib/BamHeader.h"
#include "SeqLib/BamRecord.h"
#include "seqlib_amd_merge.h"

namespace SeqLib {

class BamMerger {
public:
    BamMerger() = default;
    explicit BamMerger(int device) : device_(device) {}
    BamMerger(const BamMerger &) = delete;
    BamMerger &operator=(const BamMerger &) = delete;
    ~BamMerger() { if (m_) slx_merge_free(m_); }

    bool AddFile(const std::string &path)
    {
        if (!m_ && slx_merge_create(device_, &m_) != SLX_OK) { m_ = nullptr; return fail("AddFile"); }
        for (const auto &kv : knobs_) if (slx_merge_set(m_, kv.first.c_str(), kv.second) != SLX_OK) return fail("SetKnob");
        knobs_.clear();
        if (slx_merge_add_file(m_, path.c_str()) != SLX_OK) return fail("AddFile");
        paths_.push_back(path);
        return true;
    }
    size_t NumFiles() const { return paths_.size(); }

    // the header of the merged stream; an empty one before the first AddFile
    BamHeader Header() const
    {
        const char *h = nullptr; int64_t l = 0;
        if (!m_ || slx_merge_header(m_, &h, &l) != SLX_OK || l < 12) return BamHeader();
        const uint8_t *p = reinterpret_cast<const uint8_t *>(h);
        const uint32_t l_text = u32(p + 4);
        const std::string text(h + 8, l_text);
        const uint8_t *q = p + 8 + l_text;
        const uint32_t n_ref = u32(q);
        q += 4;
        // the dictionary is the binary one; the text is kept when its @SQ lines say the same (BamReader::Open's rule)
        const BamHeader from_text{text};
        bool same = from_text.NumSequences() == (int)n_ref;
        HeaderSequenceVector hsv;
        for (uint32_t i = 0; i < n_ref; ++i) {
            const uint32_t l_name = u32(q);
            const std::string name(reinterpret_cast<const char *>(q + 4), l_name ? l_name - 1 : 0);
            const uint32_t len = u32(q + 4 + l_name);
            q += 8 + l_name;
            hsv.push_back(HeaderSequence(name, len));
            same = same && from_text.IDtoName((int)i) == name && from_text.GetSequenceLength((int)i) == (int)len;
        }
        return same ? from_text : BamHeader(hsv);
    }

    // the inputs merged into out_path.  The merger is used up afterwards (its inputs are at their end).
    bool MergeTo(const std::string &out_path)
    {
        if (!m_ || paths_.empty()) { std::cerr << "BamMerger::MergeTo - no input; AddFile() first" << std::endl; return false; }
        if (out_path == "-") { std::cerr << "BamMerger::MergeTo - the output is a file, not a pipe" << std::endl; return false; }
        for (const std::string &p : paths_) if (p == out_path) { std::cerr << "BamMerger::MergeTo - '" << out_path << "' is an input: the output must be another file" << std::endl; return false; }
        const char *h = nullptr; int64_t l = 0;
        if (slx_merge_header(m_, &h, &l) != SLX_OK) return fail("MergeTo");
        slx_bgzf *w = nullptr;
        if (slx_bgzf_open(out_path.c_str(), (int)slx_merge_counter(m_, "device"), &w) != SLX_OK) return fail("MergeTo");
        int rc = slx_bgzf_write(w, h, l);
        if (rc == SLX_OK) rc = slx_bgzf_flush(w);
        if (rc == SLX_OK) rc = slx_merge_run(m_, w);
        const std::string msg = rc != SLX_OK ? slx_last_error() : "";
        const int rc2 = slx_bgzf_close(w);
        if (rc != SLX_OK || rc2 != SLX_OK) {
            std::cerr << "BamMerger::MergeTo - " << (rc != SLX_OK ? msg : std::string(slx_last_error())) << std::endl;
            std::remove(out_path.c_str());
            return false;
        }
        return true;
    }

    // the next round's batch in HBM, valid until the next call on the merger; n_records == 0 at the end.  Records already copied down for Next() are not served again.
    bool NextBatch(slx_merge_batch &b)
    {
        std::memset(&b, 0, sizeof b);
        if (!m_ || paths_.empty()) return false;
        if (slx_merge_next(m_, &b) != SLX_OK) return fail("NextBatch");
        return b.n_records > 0;
    }

    std::optional<BamRecord> Next()
    {
        if (!advance()) return std::nullopt;
        const uint8_t *p = stream_.data() + off_[cur_];
        last_input_ = input_[cur_];
        ++cur_;
        bam1_t *r = bam_init1();
        if (!r) throw std::bad_alloc();
        const size_t l_data = (size_t)u32(p) - 32;
        r->data = static_cast<uint8_t *>(std::malloc(l_data ? l_data : 1));
        if (!r->data) { bam_destroy1(r); throw std::bad_alloc(); }
        bam1_core_t &c = r->core;
        c.tid = (int32_t)u32(p + 4); c.pos = (int32_t)u32(p + 8);
        c.l_qname = p[12]; c.qual = p[13]; c.bin = u16(p + 14); c.n_cigar = u16(p + 16); c.flag = u16(p + 18);
        c.l_qseq = (int32_t)u32(p + 20); c.mtid = (int32_t)u32(p + 24); c.mpos = (int32_t)u32(p + 28); c.isize = (int32_t)u32(p + 32);
        c.l_extranul = 0;
        std::memcpy(r->data, p + 36, l_data);
        r->l_data = (int)l_data; r->m_data = (uint32_t)l_data;
        return BamRecord(r);
    }
    bool GetNextRecord(BamRecord &r)
    {
        std::optional<BamRecord> n = Next();
        if (!n) return false;
        r = std::move(*n);
        return true;
    }
    // the input (index of its AddFile call) the record Next() returned last came from
    int LastInput() const { return last_input_; }

    // before the first AddFile the value is kept and set when the merger is made
    bool SetKnob(const char *key, int64_t v)
    {
        if (!m_) { knobs_.push_back(std::make_pair(std::string(key), v)); return true; }
        if (slx_merge_set(m_, key, v) != SLX_OK) return fail("SetKnob");
        return true;
    }
    int64_t Counter(const char *name) const { return m_ ? slx_merge_counter(m_, name) : -1; }

private:
    static uint32_t u32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
    static uint16_t u16(const uint8_t *p) { uint16_t v; std::memcpy(&v, p, 2); return v; }
    static bool fail(const char *who) { std::cerr << "BamMerger::" << who << " - " << slx_last_error() << std::endl; return false; }
    // makes off_[cur_] a record: copies the next round down when the current one is used up; false at the end or on an error (message on stderr)
    bool advance()
    {
        if (cur_ < input_.size()) return true;
        if (eof_ || !m_ || paths_.empty()) return false;
        slx_merge_batch b;
        cur_ = 0; input_.clear();
        if (slx_merge_next(m_, &b) != SLX_OK) { eof_ = true; return fail("Next"); }
        if (b.n_records == 0) { eof_ = true; return false; }
        stream_.resize((size_t)b.n_bytes); off_.resize((size_t)b.n_records + 1); input_.resize((size_t)b.n_records);
        if (slx_merge_batch_to_host(m_, &b, stream_.data(), off_.data(), input_.data()) != SLX_OK) { eof_ = true; input_.clear(); return fail("Next"); }
        return true;
    }

    int device_ = -1;
    slx_merge *m_ = nullptr;
    std::vector<std::string> paths_;
    std::vector<std::pair<std::string, int64_t>> knobs_;
    std::vector<uint8_t> stream_, input_;
    std::vector<uint64_t> off_;
    size_t cur_ = 0;
    bool eof_ = false;
    int last_input_ = -1;
};

}  // namespace SeqLib
