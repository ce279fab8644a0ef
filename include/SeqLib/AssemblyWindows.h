// AssemblyWindows.h -- new next to the reference: the reference's local-assembly loop reads a region of a BAM record by record into
// FermiAssembler::AddRead(const BamRecord&) and assembles window after window; this class takes whole batches of records where they lie in HBM, makes every
// record a read of each window it overlaps (slx_win_*, include/seqlib_amd_win.h, where the rules are written down) and hands the windows' reads to the
// assembler's kernels without a copy to the host (slx_fml_stage_device, slx_fml_assemble_staged).
//
//     AssemblyWindows aw(windows);                      // instead of:  std::vector<FermiAssembler> fa(windows.size());
//     aw.addReads(reader);                              //              while (auto r = reader.Next())
//     aw.Assemble(contigs);                             //                  for (w : windows that overlap *r) fa[w].AddRead(*r);
//                                                       //              for (w) { fa[w].PerformAssembly(); contigs[w] = fa[w].GetContigs(); }
//
// The read order and the bytes are exactly the loop's.  Not carried on this path: read names (Reads() names a read by its record's ordinal), a per-window
// read cap (use SetReadFilter on the reader), mate lookup, several GPUs, an arena larger than HBM.  A C-ABI failure is a std::runtime_error, a refused
// argument a std::invalid_argument.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "SeqLib/BamReader.h"
#include "SeqLib/BamRecord.h"
#include "SeqLib/FermiAssembler.h"
#include "SeqLib/GenomicRegionCollection.h"
#include "SeqLib/UnalignedSequence.h"
#include "seqlib_amd_rec.h"
#include "seqlib_amd_win.h"

namespace SeqLib {

class AssemblyWindows {
public:
    // windows: closed intervals, kept in the caller's order
    explicit AssemblyWindows(const GRC &windows, int device = SLX_WIN_AUTO)
    {
        std::vector<slx_grc_iv> iv(windows.size());
        for (size_t i = 0; i < windows.size(); ++i) { std::memset(&iv[i], 0, sizeof iv[i]); iv[i].chr = windows[i].chr; iv[i].pos1 = windows[i].pos1; iv[i].pos2 = windows[i].pos2; iv[i].strand = windows[i].strand; }
        check(slx_win_create(device, iv.data(), (int64_t)iv.size(), &w_), "AssemblyWindows");
    }
    ~AssemblyWindows() { if (w_) slx_win_free(w_); }
    AssemblyWindows(const AssemblyWindows &) = delete;
    AssemblyWindows &operator=(const AssemblyWindows &) = delete;

    // ---- the rules, for the reads added afterwards
    void SetSkipFlags(uint32_t flags) { SetKnob("skip_flags", flags); }
    void SetQualityTrim(int32_t qualTrim) { SetKnob("qual_trim", qualTrim); }          // -1: off
    void SetOriginalStrand(bool on) { SetKnob("original_strand", on ? 1 : 0); }
    void SetKnob(const char *key, int64_t v) { check(slx_win_set(w_, key, v), "SetKnob"); }
    int64_t Counter(const char *name) const { return slx_win_counter(w_, name); }

    // Drains the reader batch by batch from HBM (SetRegions and SetReadFilter are honoured; what Next() has handed out of the current batch already is left
    // out; a record served once per region it overlaps is a record each time) -> the records taken
    size_t addReads(BamReader &rd)
    {
        if (!rd.rd_) throw std::runtime_error("AssemblyWindows::addReads - the reader is not open");
        size_t n = 0;
        while (rd.advance()) {
            const slx_bam_batch &b = rd.batch_;
            const uint64_t first = b.rec_off[rd.cur_];          // (the offsets count from the first one given: the stream moves up by as much)
            const int64_t k = b.n_records - (int64_t)rd.cur_;
            check(slx_win_add_device(w_, (const uint8_t *)b.d_stream + first, b.n_bytes - (int64_t)first, (const uint64_t *)b.d_rec_off + rd.cur_, k), "addReads");
            rd.cur_ = (size_t)b.n_records;
            n += (size_t)k;
        }
        finished_ = false;
        return n;
    }
    // the records a builder left in HBM (slx_rec_build*, BWAAligner::alignToBam)
    void addBatch(const slx_rec_batch &b)
    {
        check(slx_win_add_device(w_, b.d_stream, b.n_bytes, b.d_rec_off, b.n_records), "addBatch");
        finished_ = false;
    }
    // one record from the host: uploaded, then the same kernels
    void addRead(const BamRecord &r)
    {
        if (!r.raw()) throw std::invalid_argument("AssemblyWindows::addRead - empty record");
        const std::vector<uint8_t> p = detail::packed_record(r.raw());
        const uint64_t off[2] = {0, (uint64_t)p.size()};
        check(slx_win_add_host(w_, p.data(), (int64_t)p.size(), off, 1), "addRead");
        finished_ = false;
    }

    size_t NumWindows() const { return (size_t)slx_win_counter(w_, "windows"); }
    size_t NumReads(size_t window)
    {
        finish();
        return (size_t)(win_off_.at(window + 1) - win_off_.at(window));
    }

    // contigs[w]: what a FermiAssembler holding window w's reads returns from PerformAssembly() + GetContigs()
    void Assemble(std::vector<std::vector<std::string> > &contigs, const fml_opt_t *options = nullptr)
    {
        finish();
        fml_opt_t o;
        if (options) o = *options; else fml_opt_init(&o);
        const int n_win = (int)view_.n_win;
        contigs.assign((size_t)n_win, std::vector<std::string>());
        if (n_win <= 0) return;
        slx_fml *f = detail::FmlContext::get();
        detail::fml_check(slx_fml_stage_device(f, view_.d_bases, view_.d_quals, view_.d_offs, view_.n_reads));
        std::vector<fml_utg_t *> utgs((size_t)n_win, nullptr);
        std::vector<int> n_utg((size_t)n_win, 0);
        detail::fml_check(slx_fml_assemble_staged(f, &o, win_off_.data(), n_win, utgs.data(), n_utg.data()));
        for (int w = 0; w < n_win; ++w) {
            for (int i = 0; i < n_utg[(size_t)w]; ++i) contigs[(size_t)w].push_back(std::string(utgs[(size_t)w][i].seq));
            slx_fml_utgs_free(n_utg[(size_t)w], utgs[(size_t)w]);
        }
    }

    // window w's reads copied down, each named by the ordinal of its record; for inspection and tests
    UnalignedSequenceVector Reads(size_t window)
    {
        finish();
        const int64_t r0 = win_off_.at(window), r1 = win_off_.at(window + 1);
        std::vector<char> bases((size_t)view_.total + 1), quals((size_t)view_.total + 1);
        std::vector<uint64_t> offs((size_t)view_.n_reads + 1);
        std::vector<int64_t> ord((size_t)view_.n_reads + 1);
        check(slx_win_download(w_, bases.data(), quals.data(), offs.data(), nullptr, ord.data()), "Reads");
        UnalignedSequenceVector out;
        for (int64_t r = r0; r < r1; ++r) {
            const size_t a = (size_t)offs[(size_t)r], n = (size_t)(offs[(size_t)r + 1] - offs[(size_t)r]);
            out.push_back(UnalignedSequence(std::to_string(ord[(size_t)r]), std::string(bases.data() + a, n), std::string(quals.data() + a, n)));
        }
        return out;
    }

    // empties the collector and keeps its windows and rules
    void Clear() { check(slx_win_clear(w_), "Clear"); finished_ = false; }
    slx_win *raw() const { return w_; }

private:
    void finish()
    {
        if (finished_) return;
        check(slx_win_finish(w_), "finish");
        check(slx_win_view(w_, &view_), "finish");
        win_off_.assign((size_t)view_.n_win + 1, 0);
        check(slx_win_download(w_, nullptr, nullptr, nullptr, win_off_.data(), nullptr), "finish");
        finished_ = true;
    }
    static void check(int rc, const char *who)
    {
        if (rc == SLX_EINVAL) throw std::invalid_argument(std::string("AssemblyWindows::") + who + " - " + slx_last_error());
        if (rc != SLX_OK) throw std::runtime_error(std::string("AssemblyWindows::") + who + " - " + slx_last_error());
    }
    slx_win *w_ = nullptr;
    slx_win_result view_ = {};
    std::vector<int64_t> win_off_;
    bool finished_ = false;
};

inline void FermiAssembler::AssembleRegions(BamReader &reader, const GRC &windows, std::vector<std::vector<std::string> > &contigs, const fml_opt_t *options)
{
    AssemblyWindows aw(windows);
    aw.addReads(reader);
    aw.Assemble(contigs, options);
}

}  // namespace SeqLib
