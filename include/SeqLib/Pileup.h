// Pileup.h -- SeqLib::Pileup for the MI355X drop-in: the per-position table of allele counts a SeqLib user builds by hand from Next() + GetCigar() + Sequence() +
// Qualities(), kept in HBM behind include/seqlib_amd_pile.h, which lists every rule.  There is no reference class: the interface is STCoverage's shape.
//   Pileup(GenomicRegion)     one window [pos1, pos2) of contig chr, what BamReader::SetRegion hands down for the same GenomicRegion; without SetHeader the
//                             contig is taken to end at the window's end (Sites then needs a FASTA contig of that length: set the header)
//   planes                    15 per position: for strand s (1 when the read is reversed) 7 * s + {A, C, G, T, N, DEL, INS}, and plane 14 for bases under
//                             SetMinBaseQuality; 60 bytes of HBM per reference base
//   addReads(BamReader&)      drains a reader batch by batch without a host round trip (SetRegions and SetReadFilter are honoured; a record served once per
//                             region it overlaps is counted once per region); addBatch takes the records alignToBam's builder left in HBM; addRead buffers on
//                             the host and goes up before any read
//   Sites(RefGenome&, ...)    the positions where the reads disagree with the reference, compacted on the GPU; the contig is matched by name through the header
// A C-ABI failure is a std::runtime_error.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "SeqLib/BamHeader.h"
#include "SeqLib/BamReader.h"
#include "SeqLib/BamRecord.h"
#include "SeqLib/GenomicRegion.h"
#include "SeqLib/RefGenome.h"
#include "seqlib_amd_pile.h"
#include "seqlib_amd_rec.h"

namespace SeqLib {

struct PileupSite {
    int64_t pos = 0;
    char ref = 'N';                                   // upper case
    int32_t depth = 0, alt = 0, ins = 0;
    std::array<int32_t, SLX_PILE_PLANES> plane{};
};

class Pileup {
public:
    explicit Pileup(const GenomicRegion &gr) : gr_(gr)
    {
        if (gr.chr < 0) throw std::invalid_argument("Pileup - the window names no contig");
    }
    Pileup(const Pileup &) = delete;
    Pileup &operator=(const Pileup &) = delete;
    ~Pileup() { if (p_) slx_pile_free(p_); }

    // the contigs; what was counted so far goes
    void SetHeader(const BamHeader &h)
    {
        std::vector<int64_t> len;
        std::vector<std::string> names;
        for (int i = 0; i < h.NumSequences(); ++i) { len.push_back(h.GetSequenceLength(i)); names.push_back(h.IDtoName(i)); }
        create(len, &names);
    }
    void SetMinMapq(int q) { flush(); min_mapq_ = q; }
    void SetMinBaseQuality(int q) { flush(); min_baseq_ = q; }
    void SetExcludeFlags(uint32_t f) { flush(); exclude_ = f; }              // default 0x704
    void SetKnob(const char *key, int64_t v) { need(); check(slx_pile_set(p_, key, v)); }
    int64_t Counter(const char *name) const { return p_ ? slx_pile_counter(p_, name) : -1; }

    // every record the reader still has, batch by batch, from HBM to HBM; returns how many were handed over
    size_t addReads(BamReader &rd)
    {
        if (!rd.rd_) throw std::runtime_error("Pileup::addReads - the reader is not open");
        if (!p_ && !have_header_) SetHeader(rd.Header());
        flush();
        apply();
        size_t n = 0;
        while (rd.advance()) {
            const slx_bam_batch &b = rd.batch_;
            const int64_t k = b.n_records - (int64_t)rd.cur_;
            check(slx_pile_add_device(p_, b.d_stream, b.n_bytes, (const uint64_t *)b.d_rec_off + rd.cur_, k));
            rd.cur_ = (size_t)b.n_records;
            n += (size_t)k;
        }
        return n;
    }
    // the records a builder left in HBM (slx_rec_build*, BWAAligner::alignToBam)
    void addBatch(const slx_rec_batch &b)
    {
        flush();
        apply();
        check(slx_pile_add_device(p_, b.d_stream, b.n_bytes, b.d_rec_off, b.n_records));
    }
    // buffered on the host; goes up through slx_pile_add_host when the buffer is full and before any read
    void addRead(const BamRecord &r)
    {
        if (!r.raw()) return;
        need();
        const std::vector<uint8_t> o = detail::packed_record(r.raw());
        stream_.insert(stream_.end(), o.begin(), o.end());
        off_.push_back(stream_.size());
        if (stream_.size() >= STAGE) flush();
    }

    // one plane over the window: pos2 - pos1 counts (fewer when the contig ends inside the window)
    std::vector<int32_t> Counts(int plane)
    {
        flush(); need();
        const void *d = nullptr; int64_t n = 0;
        check(slx_pile_counts_device(p_, plane, &d, &n));
        std::vector<int32_t> v((size_t)n);
        const int64_t beg = gr_.pos1 < 0 ? 0 : gr_.pos1;
        check(slx_pile_counts(p_, plane, beg, beg + n, v.data()));
        return v;
    }
    // the 15 counts of one position; all 0 outside the window
    std::array<int32_t, SLX_PILE_PLANES> At(int64_t pos)
    {
        flush(); need();
        std::array<int32_t, SLX_PILE_PLANES> a{};
        check(slx_pile_at(p_, pos, a.data()));
        return a;
    }
    // the candidate sites by the rule of seqlib_amd_pile.h, in ascending position.  The FASTA contig is the one with the window's contig's name (with a header), or
    // with its number (without); std::invalid_argument when the FASTA has no such contig
    std::vector<PileupSite> Sites(RefGenome &ref, int min_depth, int min_alt, int frac_num, int frac_den)
    {
        flush(); need();
        if (!ref.ref_) throw std::invalid_argument("Pileup::Sites - the reference is not loaded");
        const int64_t tid = names_.empty() ? (int64_t)gr_.chr : slx_ref_tid(ref.ref_, names_[(size_t)gr_.chr].c_str());
        if (tid < 0) throw std::invalid_argument("Pileup::Sites - the reference has no contig '" + names_[(size_t)gr_.chr] + "'");
        int64_t n = 0;
        check(slx_pile_sites(p_, ref.ref_, tid, min_depth, min_alt, frac_num, frac_den, &n));
        std::vector<slx_pile_site> raw((size_t)n);
        check(slx_pile_sites_to_host(p_, raw.data()));
        std::vector<PileupSite> out((size_t)n);
        for (size_t i = 0; i < raw.size(); ++i) {
            out[i].pos = raw[i].pos; out[i].ref = (char)raw[i].ref; out[i].depth = raw[i].depth; out[i].alt = raw[i].alt; out[i].ins = raw[i].ins;
            for (int k = 0; k < SLX_PILE_PLANES; ++k) out[i].plane[(size_t)k] = raw[i].plane[k];
        }
        return out;
    }
    // the last Sites() as text: name, 1-based position, reference base, depth, then A C G T N DEL INS as fwd,rev and the low-quality count
    void WriteSites(const std::string &path) { need(); check(slx_pile_sites_tsv(p_, path.c_str())); }
    void Clear()
    {
        stream_.clear(); off_.assign(1, 0);
        if (p_) check(slx_pile_clear(p_));
    }

private:
    static const size_t STAGE = (size_t)8 << 20;
    void check(int rc) const { if (rc != SLX_OK) throw std::runtime_error(std::string("Pileup - ") + slx_last_error()); }
    void create(const std::vector<int64_t> &len, const std::vector<std::string> *names)
    {
        stream_.clear(); off_.assign(1, 0);
        if (p_) { slx_pile_free(p_); p_ = nullptr; }
        std::vector<const char *> nm;
        names_.clear();
        if (names) { names_ = *names; for (const std::string &s : names_) nm.push_back(s.c_str()); }
        const slx_bam_region w = {gr_.chr, gr_.pos1, gr_.pos2};
        check(slx_pile_create(-1, (int)len.size(), len.data(), names ? nm.data() : nullptr, &w, &p_));
        have_header_ = true;
    }
    // the object, made on first use: of the header, or without one of a contig that ends where the window ends
    void need()
    {
        if (p_) return;
        std::vector<int64_t> len((size_t)gr_.chr + 1, 0);
        len[(size_t)gr_.chr] = gr_.pos2 < 0 ? 0 : gr_.pos2;
        create(len, nullptr);
    }
    void apply()
    {
        need();
        check(slx_pile_set(p_, "min_mapq", min_mapq_));
        check(slx_pile_set(p_, "min_baseq", min_baseq_));
        check(slx_pile_set(p_, "exclude_flags", exclude_));
    }
    void flush()
    {
        if (off_.size() <= 1) return;
        apply();
        const int rc = slx_pile_add_host(p_, stream_.data(), (int64_t)stream_.size(), off_.data(), (int64_t)off_.size() - 1);
        stream_.clear(); off_.assign(1, 0);
        check(rc);
    }

    slx_pile *p_ = nullptr;
    GenomicRegion gr_;
    bool have_header_ = false;
    int min_mapq_ = 0, min_baseq_ = 0;
    uint32_t exclude_ = 0x704;
    std::vector<std::string> names_;
    std::vector<uint8_t> stream_;
    std::vector<uint64_t> off_ = std::vector<uint64_t>(1, 0);
};

}  // namespace SeqLib
