// RefGenome.h -- SeqLib::RefGenome for the MI355X drop-in: an indexed reference genome, held in HBM behind include/seqlib_amd_ref.h.
// The reference class (SeqLib/RefGenome.h, src/RefGenome.cpp) is kept as it is used: RefGenome(), LoadIndex (false for an unreadable or malformed file, the
// message on stderr), QueryRegion(chr_name, p1, p2) with both ends inclusive and 0-based and its std::invalid_argument for nothing loaded, p1 > p2, p1 < 0, an
// unknown name and an empty result, IsEmpty().  What differs, and why:
//   - LoadIndex builds the .fai on the GPU from the FASTA itself (plain, BGZF or gzip) and keeps every base in HBM.  The reference's fai_load writes <file>.fai as
//     a side effect when there is none; this one writes nothing unless WriteFai is called, and a <file>.fai that is present and differs from the built index
//     fails the load ("stale index") instead of being believed.  Without a GPU LoadIndex throws std::runtime_error: there is no CPU fallback.
//   - QueryRegion clips p2 to the contig's end, as faidx_fetch_seq does; a region wholly behind the end is the reference's "empty query".
// New next to the reference, and the reason for the GPU: NumSequences / SequenceName / SequenceLength / WriteFai; QueryRegions(GRC) fetches many regions in one
// launch (ready for BWAIndex::ConstructIndex, named chr:p1-p2 with chr the FASTA's contig index); FetchBatch leaves them in HBM in the layout
// slx_align_batch_device takes; NmMd computes NM and MD:Z of every record of a batch that lies in HBM -- the batch a BamReader serves next, or the records
// alignToBam's builder left, or records in host memory -- against the resident bases (the rules are in seqlib_amd_ref.h).  A GenomicRegion is taken as [pos1, pos2], both ends inclusive, like
// QueryRegion's p1 and p2.  A C-ABI failure other than those named is a std::runtime_error.
#pragma once
#include <cstdint>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>
#include "SeqLib/BamHeader.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/GenomicRegionCollection.h"
#include "SeqLib/RecordEditor.h"
#include "SeqLib/UnalignedSequence.h"
#include "seqlib_amd_rec.h"
#include "seqlib_amd_ref.h"

namespace SeqLib {

// regions in HBM: n + 1 uint64 offsets into d_bases; valid until the RefGenome's next fetch
struct RefBatch { const void *d_bases = nullptr, *d_offs = nullptr; int64_t n_regions = 0, n_bytes = 0; };

class RefGenome {
    friend class Pileup;              // Sites(RefGenome&): the reference's handle, as it lies in HBM
public:
    RefGenome() = default;
    RefGenome(const RefGenome &) = delete;
    RefGenome &operator=(const RefGenome &) = delete;
    ~RefGenome() { if (ref_) slx_ref_close(ref_); }

    bool LoadIndex(const std::string &file)
    {
        if (ref_) slx_ref_close(ref_);
        ref_ = nullptr;
        const int rc = slx_ref_open(file.c_str(), -1, &ref_);
        if (rc == SLX_ENODEVICE) throw std::runtime_error(std::string("RefGenome::LoadIndex - ") + slx_last_error());
        if (rc != SLX_OK) { std::cerr << "RefGenome::LoadIndex - " << slx_last_error() << std::endl; ref_ = nullptr; return false; }
        return true;
    }
    bool IsEmpty() const { return ref_ == nullptr; }

    std::string QueryRegion(const std::string &chr_name, int32_t p1, int32_t p2) const
    {
        if (!ref_) throw std::invalid_argument("RefGenome::queryRegion index not loaded");
        if (p1 > p2) throw std::invalid_argument("RefGenome::queryRegion p1 must be <= p2");
        if (p1 < 0) throw std::invalid_argument("RefGenome::queryRegion p1 must be >= 0");
        const int64_t tid = slx_ref_tid(ref_, chr_name.c_str());
        if (tid < 0) throw std::invalid_argument("RefGenome::queryRegion - Could not find valid sequence");
        const slx_bam_region r = {(int32_t)tid, p1, (int64_t)p2 + 1};
        uint64_t offs[2] = {0, 0};
        check(slx_ref_fetch_host(ref_, &r, 1, 0, nullptr, 0, offs));
        std::string out((size_t)offs[1], '\0');
        if (!out.empty()) check(slx_ref_fetch_host(ref_, &r, 1, 0, &out[0], (int64_t)out.size(), offs));
        if (out.empty()) throw std::invalid_argument("RefGenome::queryRegion - Returning empty query on " + chr_name + ":" + std::to_string(p1) + "-" + std::to_string(p2));
        return out;
    }

    int NumSequences() const { return ref_ ? (int)slx_ref_nseq(ref_) : 0; }
    std::string SequenceName(int i) const { const char *n = ref_ ? slx_ref_name(ref_, i) : nullptr; if (!n) throw std::out_of_range("RefGenome::SequenceName - no such contig"); return n; }
    int64_t SequenceLength(int i) const { const int64_t l = ref_ ? slx_ref_len(ref_, i) : -1; if (l < 0) throw std::out_of_range("RefGenome::SequenceLength - no such contig"); return l; }
    int SequenceID(const std::string &name) const { return ref_ ? (int)slx_ref_tid(ref_, name.c_str()) : -1; }
    // the index as text; path empty: the FASTA's path + ".fai"
    std::string FaiText() const { need("FaiText"); int64_t n = 0; const char *t = slx_ref_fai_text(ref_, &n); return std::string(t, (size_t)n); }
    void WriteFai(const std::string &path = std::string()) const { need("WriteFai"); check(slx_ref_write_fai(ref_, path.empty() ? nullptr : path.c_str())); }
    void SetKnob(const char *key, int64_t v) { need("SetKnob"); check(slx_ref_set(ref_, key, v)); }
    int64_t Counter(const char *name) const { return ref_ ? slx_ref_counter(ref_, name) : -1; }

    // every region in one fetch, clipped to its contig (a region that is empty then gives an empty Seq); std::invalid_argument for a chr that is no contig
    UnalignedSequenceVector QueryRegions(const GRC &grc, bool upper = false) const
    {
        need("QueryRegions");
        const std::vector<slx_bam_region> r = regions(grc, "QueryRegions");
        std::vector<uint64_t> offs(r.size() + 1, 0);
        check(slx_ref_fetch_host(ref_, r.data(), (int64_t)r.size(), upper ? 1 : 0, nullptr, 0, offs.data()));
        std::string all((size_t)offs.back(), '\0');
        if (!all.empty()) check(slx_ref_fetch_host(ref_, r.data(), (int64_t)r.size(), upper ? 1 : 0, &all[0], (int64_t)all.size(), offs.data()));
        UnalignedSequenceVector out;
        out.reserve(r.size());
        for (size_t i = 0; i < r.size(); ++i)
            out.push_back(UnalignedSequence(std::to_string(r[i].tid) + ":" + std::to_string(r[i].beg) + "-" + std::to_string(r[i].end - 1), all.substr((size_t)offs[i], (size_t)(offs[i + 1] - offs[i]))));
        return out;
    }
    // the same, left in HBM: what slx_align_batch_device takes
    RefBatch FetchBatch(const GRC &grc, bool upper = true)
    {
        need("FetchBatch");
        const std::vector<slx_bam_region> r = regions(grc, "FetchBatch");
        RefBatch b;
        check(slx_ref_fetch_device(ref_, r.data(), (int64_t)r.size(), upper ? 1 : 0, &b.d_bases, &b.d_offs, &b.n_bytes));
        b.n_regions = (int64_t)r.size();
        return b;
    }

    // NM and MD of every record of the batch the reader serves next (SetRegions and SetReadFilter are honoured), which is then used up; returns how many records
    // that was, 0 at the end of the file.  Contigs are matched by name through the reader's header: a name the FASTA does not have makes its records not
    // eligible (nm -1, MD empty); a name it has with another length throws std::invalid_argument.
    size_t NmMd(BamReader &rd, std::vector<int32_t> &nm, std::vector<std::string> &md)
    {
        need("NmMd");
        if (!rd.rd_) throw std::runtime_error("RefGenome::NmMd - the reader is not open");
        const std::vector<int32_t> map = tid_map(rd.Header());
        nm.clear(); md.clear();
        if (!rd.advance()) return 0;
        const slx_bam_batch &b = rd.batch_;
        const int64_t k = b.n_records - (int64_t)rd.cur_;
        slx_ref_md m;
        const int32_t none = -1;          // (a header without contigs is still a map, not the identity)
        check(slx_ref_nm_md_device(ref_, b.d_stream, b.n_bytes, (const uint64_t *)b.d_rec_off + rd.cur_, k, map.empty() ? &none : map.data(), (int64_t)map.size(), &m));
        rd.cur_ = (size_t)b.n_records;
        down(m, nm, md);
        return (size_t)k;
    }
    // ... of the records a builder left in HBM (slx_rec_build*, BWAAligner::alignToBam); their tids are taken as the FASTA's
    size_t NmMd(const slx_rec_batch &b, std::vector<int32_t> &nm, std::vector<std::string> &md)
    {
        need("NmMd");
        slx_ref_md m;
        check(slx_ref_nm_md_device(ref_, b.d_stream, b.n_bytes, b.d_rec_off, b.n_records, nullptr, 0, &m));
        down(m, nm, md);
        return (size_t)b.n_records;
    }
    // calmd without leaving HBM: NM and MD of the batch the reader serves next, written back into its records there.  The editor's plan is applied, then NM:i is
    // replaced and MD:Z is replaced from the columns slx_ref_nm_md_device left in HBM; a record that is not eligible keeps the tags it has (nm -1 and an empty
    // MD add nothing).  The two adds join the editor's plan for this call only and leave it again: the plan needs room for two more adds and no NM or MD add of its own
    // (std::invalid_argument otherwise).  The result is ed.Batch(); the reader's
    // batch is used up.  Returns how many records that was, 0 at the end of the file; what Next() has handed out of the batch already is left out, as in NmMd(BamReader&).
    size_t WriteNmMd(BamReader &rd, RecordEditor &ed)
    {
        need("WriteNmMd");
        if (!rd.rd_) throw std::runtime_error("RefGenome::WriteNmMd - the reader is not open");
        const std::vector<int32_t> map = tid_map(rd.Header());
        if (!rd.advance()) return 0;
        const slx_bam_batch &b = rd.batch_;
        const int64_t k = b.n_records - (int64_t)rd.cur_;
        const uint64_t first = b.rec_off[rd.cur_];
        slx_ref_md m;
        const int32_t none = -1;
        check(slx_ref_nm_md_device(ref_, b.d_stream, b.n_bytes, (const uint64_t *)b.d_rec_off + rd.cur_, k, map.empty() ? &none : map.data(), (int64_t)map.size(), &m));
        write_back(ed, m, (const uint8_t *)b.d_stream + first, b.n_bytes - (int64_t)first, (const uint64_t *)b.d_rec_off + rd.cur_, k);
        rd.cur_ = (size_t)b.n_records;
        return (size_t)k;
    }
    // ... of the records a builder left in HBM; their tids are taken as the FASTA's
    size_t WriteNmMd(const slx_rec_batch &b, RecordEditor &ed)
    {
        need("WriteNmMd");
        slx_ref_md m;
        check(slx_ref_nm_md_device(ref_, b.d_stream, b.n_bytes, b.d_rec_off, b.n_records, nullptr, 0, &m));
        write_back(ed, m, b.d_stream, b.n_bytes, b.d_rec_off, b.n_records);
        return (size_t)b.n_records;
    }
    // ... of records in host memory (uploaded, then the same kernels); their tids are taken as the FASTA's
    size_t NmMd(const BamRecordPtrVector &recs, std::vector<int32_t> &nm, std::vector<std::string> &md)
    {
        need("NmMd");
        std::vector<uint8_t> stream;
        std::vector<uint64_t> off(1, 0);
        for (const BamRecordPtr &r : recs) {
            if (!r || !r->raw()) throw std::invalid_argument("RefGenome::NmMd - empty record");
            const std::vector<uint8_t> o = detail::packed_record(r->raw());
            stream.insert(stream.end(), o.begin(), o.end());
            off.push_back(stream.size());
        }
        slx_ref_md m;
        check(slx_ref_nm_md_host(ref_, stream.data(), (int64_t)stream.size(), off.data(), (int64_t)recs.size(), nullptr, 0, &m));
        down(m, nm, md);
        return recs.size();
    }

private:
    void need(const char *who) const { if (!ref_) throw std::invalid_argument(std::string("RefGenome::") + who + " index not loaded"); }
    static void check(int rc) { if (rc != SLX_OK) throw std::runtime_error(std::string("RefGenome - ") + slx_last_error()); }
    std::vector<slx_bam_region> regions(const GRC &grc, const char *who) const
    {
        std::vector<slx_bam_region> r;
        const int64_t n = slx_ref_nseq(ref_);
        for (const GenomicRegion &g : grc) {
            if (g.chr < 0 || g.chr >= n) throw std::invalid_argument(std::string("RefGenome::") + who + " - a region names contig " + std::to_string(g.chr) + ", which the FASTA does not have");
            r.push_back(slx_bam_region{g.chr, g.pos1, (int64_t)g.pos2 + 1});
        }
        return r;
    }
    std::vector<int32_t> tid_map(const BamHeader &h) const
    {
        std::vector<int32_t> map;
        for (int i = 0; i < h.NumSequences(); ++i) {
            const std::string name = h.IDtoName(i);
            const int64_t t = slx_ref_tid(ref_, name.c_str());
            if (t >= 0 && slx_ref_len(ref_, t) != (int64_t)h.GetSequenceLength(i))
                throw std::invalid_argument("RefGenome::NmMd - contig '" + name + "' has " + std::to_string(h.GetSequenceLength(i)) + " bases in the header and " + std::to_string(slx_ref_len(ref_, t)) + " in the FASTA");
            map.push_back((int32_t)t);
        }
        return map;
    }
    void write_back(RecordEditor &ed, const slx_ref_md &m, const void *d_stream, int64_t n_bytes, const void *d_rec_off, int64_t n)
    {
        if (slx_edit_add_int_column(ed.e_, "NM", m.d_nm, -1, 1) != SLX_OK) throw std::invalid_argument(std::string("RefGenome::WriteNmMd - ") + slx_last_error());
        if (slx_edit_add_z_column(ed.e_, "MD", m.d_md, m.md_bytes, m.d_md_off) != SLX_OK) {
            const std::string why = slx_last_error();
            (void)slx_edit_drop_column(ed.e_, "NM");
            throw std::invalid_argument("RefGenome::WriteNmMd - " + why);
        }
        // the two adds are the call's own: they leave the plan again, whatever becomes of the apply, so that the editor is afterwards what the caller made it
        struct Undo { slx_edit *e; ~Undo() { (void)slx_edit_drop_column(e, "MD"); (void)slx_edit_drop_column(e, "NM"); } } undo{ed.e_};
        ed.Apply(d_stream, n_bytes, d_rec_off, n);
    }
    void down(const slx_ref_md &m, std::vector<int32_t> &nm, std::vector<std::string> &md) const
    {
        const size_t n = (size_t)m.n_records;
        nm.assign(n, -1); md.assign(n, std::string());
        if (!n) return;
        std::vector<uint64_t> off(n + 1, 0);
        std::string all((size_t)m.md_bytes, '\0');
        check(slx_ref_md_to_host(ref_, &m, nm.data(), all.empty() ? nullptr : &all[0], off.data()));
        for (size_t i = 0; i < n; ++i) md[i] = all.substr((size_t)off[i], (size_t)(off[i + 1] - off[i]));
    }

    slx_ref *ref_ = nullptr;
};

}  // namespace SeqLib
