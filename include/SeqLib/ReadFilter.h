// ReadFilter.h -- SeqLib::Filter for the MI355X drop-in: Flag, Range, FlagRule, AbstractRule, ReadFilter and ReadFilterCollection with the
// names and signatures of /root/reference/SeqLib/ReadFilter.h:80-576, over the C-ABI of include/seqlib_amd_filter.h.  The classes only hold the rules; every
// verdict comes from the one per-record body of the library (seqlib_amd/csrc/dev_rfilter.h): isValid(const BamRecord&) hands the record to
// slx_filter_test_record on the host, and BamReader::SetReadFilter (BamReader.h) hands the collection to the GPU, where every batch is evaluated and
// compacted before Next / NextBatch see it.  The semantics, quirks included, are restated in seqlib_amd_filter.h from src/ReadFilter.cpp:22-136, 457-658.
// Not declared, so that a use does not compile: the JSON constructor ReadFilterCollection(script, header), addGlobalRule and every parseJson
// (jsoncpp is third-party and not in the tree).  The phred and xp ranges and the strand / paired flags are carried and, as in the reference, never evaluated.
// AbstractRule::isValid and ReadFilter::isValid build their one-rule / one-filter collection on every call (the public fields may have changed); a
// ReadFilterCollection compiles once per AddReadFilter.
#pragma once
#include <cstdint>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "SeqLib/BamRecord.h"
#include "SeqLib/GenomicRegionCollection.h"
#include "seqlib_amd_filter.h"

namespace SeqLib {
namespace Filter {

class Flag {          // SeqLib/ReadFilter.h:87-122
public:
    Flag() : on(false), off(false), na(true) {}
    void setNA() { on = false; off = false; na = true; }
    void setOn() { on = true; off = false; na = false; }
    void setOff() { on = false; off = true; na = false; }
    bool isNA() const { return na; }
    bool isOn() const { return on; }
    bool isOff() const { return off; }
private:
    bool on, off, na;
};

class Range {          // SeqLib/ReadFilter.h:129-184
public:
    Range() : m_min(0), m_max(0), m_inverted(false), m_every(true) {}
    Range(int min, int max, bool inverted) : m_min(min), m_max(max), m_inverted(inverted), m_every(false) {}
    bool isValid(int val)
    {
        if (m_every) return true;
        return !m_inverted ? (val >= m_min && val <= m_max) : (val < m_min || val > m_max);
    }
    bool isEvery() const { return m_every; }
    int lowerBound() const { return m_min; }
    int upperBound() const { return m_max; }
    bool isInverted() const { return m_inverted; }
private:
    int m_min, m_max;
    bool m_inverted, m_every;
};

class FlagRule {          // SeqLib/ReadFilter.h:191-286
public:
    FlagRule() : every(false), m_all_on_flag(0), m_all_off_flag(0), m_any_on_flag(0), m_any_off_flag(0) {}
    Flag dup, supp, qcfail, hardclip, fwd_strand, rev_strand, mate_fwd_strand, mate_rev_strand, mapped, mate_mapped, ff, fr, rf, rr, ic, paired;
    void setAnyOnFlag(uint32_t f) { m_any_on_flag = f; every = (every && f == 0); }
    void setAnyOffFlag(uint32_t f) { m_any_off_flag = f; every = (every && f == 0); }
    void setAllOnFlag(uint32_t f) { m_all_on_flag = f; every = (every && f == 0); }
    void setAllOffFlag(uint32_t f) { m_all_off_flag = f; every = (every && f == 0); }
    bool isEvery() const { return every; }
    inline bool isValid(const BamRecord &r);
    // the masks and the evaluated tri-states in the C-ABI's form
    void fill(slx_filter_rule &o) const
    {
        o.all_on = m_all_on_flag; o.all_off = m_all_off_flag; o.any_on = m_any_on_flag; o.any_off = m_any_off_flag;
        const Flag *t[SLX_FT_N] = {&dup, &supp, &qcfail, &hardclip, &mapped, &mate_mapped, &ff, &fr, &rf, &rr, &ic};
        o.tri = 0;
        for (int i = 0; i < SLX_FT_N; ++i) o.tri |= (t[i]->isOn() ? 1u : t[i]->isOff() ? 2u : 0u) << (2 * i);
    }
private:
    bool every;
    uint32_t m_all_on_flag, m_all_off_flag, m_any_on_flag, m_any_off_flag;
};

namespace detail {
struct Handle {          // an slx_filter owned by a shared_ptr
    static std::shared_ptr<slx_filter> make()
    {
        slx_filter *f = nullptr;
        if (slx_filter_create(&f) != SLX_OK) throw std::runtime_error(std::string("SeqLib::Filter - ") + slx_last_error());
        return std::shared_ptr<slx_filter>(f, [](slx_filter *p) { slx_filter_free(p); });
    }
};
inline bool test(slx_filter *f, const BamRecord &r)
{
    if (!r.raw()) throw std::invalid_argument("SeqLib::Filter - empty BamRecord");
    const std::vector<uint8_t> p = SeqLib::detail::packed_record(r.raw());
    const int rc = slx_filter_test_record(f, p.data(), (int64_t)p.size());
    if (rc < 0) throw std::runtime_error(std::string("SeqLib::Filter - ") + slx_last_error());
    return rc == 1;
}
}  // namespace detail

class AbstractRule {          // SeqLib/ReadFilter.h:293-388
    friend class ReadFilter;
    friend class ReadFilterCollection;
public:
    AbstractRule() : m_count(0), subsam_frac(1), subsam_seed(999), motifs_inverted(false) {}
    // the motifs of a newline-separated file (src/ReadFilter.cpp:832-854); runtime_error when it cannot be read
    void addMotifRule(const std::string &f, bool inverted)
    {
        std::ifstream in(f.c_str());
        if (!in) throw std::runtime_error("AhoCorasick::TrieFromFile - Cannot read file: " + f);
        std::string pat;
        while (std::getline(in, pat, '\n')) motifs.push_back(pat);
        motifs_inverted = inverted;
    }
    inline bool isValid(const BamRecord &r);
    bool isEvery() const          // src/ReadFilter.cpp:22-31 (a FlagRule is never "every": its constructor says false)
    {
        return read_group.empty() && ins.isEvery() && del.isEvery() && isize.isEvery() && mapq.isEvery() && len.isEvery() && clip.isEvery() && nm.isEvery() && nbases.isEvery() &&
               fr.isEvery() && subsam_frac >= 1 && xp.isEvery() && motifs.empty();
    }
    void SetSubsampleRate(double s) { subsam_frac = s; }
    void SetRuleID(const std::string &s) { id = s; }
    void SetReadGroup(const std::string &rg) { read_group = rg; }

    FlagRule fr;
    Range isize, mapq, len, phred, clip, nm, nbases, ins, del, xp;

private:
    void add_to(slx_filter *f, int filter_id) const
    {
        slx_filter_rule o;
        std::memset(&o, 0, sizeof o);
        const Range *g[SLX_FR_N] = {&isize, &mapq, &len, &clip, &nm, &nbases, &ins, &del};
        for (int i = 0; i < SLX_FR_N; ++i) { o.r[i].min = g[i]->lowerBound(); o.r[i].max = g[i]->upperBound(); o.r[i].inverted = g[i]->isInverted(); o.r[i].every = g[i]->isEvery(); }
        fr.fill(o);
        o.subsample_frac = subsam_frac; o.subsample_seed = subsam_seed; o.motifs_inverted = motifs_inverted;
        std::vector<const char *> m;
        for (const std::string &s : motifs) m.push_back(s.c_str());
        if (slx_filter_add_rule(f, filter_id, &o, read_group.c_str(), m.data(), (int64_t)m.size()) != SLX_OK) throw std::runtime_error(std::string("SeqLib::Filter - ") + slx_last_error());
    }
    std::string read_group;
    size_t m_count;
    std::vector<std::string> motifs;
    std::string id;
    double subsam_frac;
    uint32_t subsam_seed;
    bool motifs_inverted;
};

class ReadFilter {          // SeqLib/ReadFilter.h:398-484
    friend class ReadFilterCollection;
public:
    ReadFilter() : excluder(false), m_applies_to_mate(false), m_count(0) {}
    bool isValid(const BamRecord &r)          // the rules only, not the regions (src/ReadFilter.cpp:33-49)
    {
        auto h = detail::Handle::make();
        add_to(h.get(), false, false);
        return detail::test(h.get(), r);
    }
    void AddRule(const AbstractRule &ar) { m_abstract_rules.push_back(ar); }
    void setRegions(const GRC &g) { m_grv = g; }
    void addRegions(const GRC &g) { for (const GenomicRegion &r : g) m_grv.add(r); }          // (the reference merges what overlaps: the same answers)
    bool isReadOverlappingRegion(const BamRecord &r) const          // src/ReadFilter.cpp:77-92
    {
        auto h = detail::Handle::make();
        ReadFilter only_regions;
        only_regions.m_grv = m_grv; only_regions.m_applies_to_mate = m_applies_to_mate;
        only_regions.add_to(h.get(), true, false);
        return detail::test(h.get(), r);
    }
    size_t size() const { return m_abstract_rules.size(); }
    void SetExcluder(bool e) { excluder = e; }
    void SetMateLinked(bool e) { m_applies_to_mate = e; }

private:
    void add_to(slx_filter *f, bool with_regions, bool with_excluder) const
    {
        std::vector<slx_bam_region> g;
        if (with_regions) for (const GenomicRegion &r : m_grv) g.push_back(slx_bam_region{r.chr, r.pos1, r.pos2});
        const int id = slx_filter_add_filter(f, with_excluder && excluder, m_applies_to_mate, g.data(), (int64_t)g.size());
        if (id < 0) throw std::runtime_error(std::string("SeqLib::Filter - ") + slx_last_error());
        for (const AbstractRule &a : m_abstract_rules) a.add_to(f, id);
    }
    GRC m_grv;
    std::string id;
    bool excluder;
    std::vector<AbstractRule> m_abstract_rules;
    bool m_applies_to_mate;
    size_t m_count;
};

class ReadFilterCollection {          // SeqLib/ReadFilter.h:493-576
public:
    ReadFilterCollection() {}
    void AddReadFilter(const ReadFilter &rf) { m_regions.push_back(rf); h_.reset(); }
    bool isValid(const BamRecord &r) { return detail::test(handle(), r); }          // src/ReadFilter.cpp:96-136
    GRC getAllRegions() const
    {
        GRC out;
        for (const ReadFilter &f : m_regions) for (const GenomicRegion &g : f.m_grv) out.add(g);
        return out;
    }
    size_t size() const { return m_regions.size(); }
    size_t numRules() const { size_t n = 0; for (const ReadFilter &f : m_regions) n += f.size(); return n; }
    void CheckHasIncluder()          // src/ReadFilter.cpp:272-287
    {
        for (const ReadFilter &f : m_regions) if (!f.excluder) return;
        ReadFilter mr;
        mr.m_abstract_rules.push_back(rule_all);
        mr.id = "WG_includer";
        AddReadFilter(mr);
    }
    // records tested and passed so far, on the host and on the GPU
    int64_t Counter(const char *name) const { return h_ ? slx_filter_counter(h_.get(), name) : 0; }
    // the compiled collection, for BamReader::SetReadFilter; it stays alive as long as a reader holds it
    std::shared_ptr<slx_filter> Handle() const { handle(); return h_; }

private:
    slx_filter *handle() const
    {
        if (!h_) {
            h_ = detail::Handle::make();
            for (const ReadFilter &f : m_regions) f.add_to(h_.get(), true, true);
        }
        return h_.get();
    }
    AbstractRule rule_all;
    std::vector<ReadFilter> m_regions;
    mutable std::shared_ptr<slx_filter> h_;
};

inline bool AbstractRule::isValid(const BamRecord &r)          // src/ReadFilter.cpp:457-563
{
    ReadFilter f;
    f.AddRule(*this);
    return f.isValid(r);
}
inline bool FlagRule::isValid(const BamRecord &r)              // src/ReadFilter.cpp:565-658
{
    AbstractRule a;
    a.fr = *this;
    return a.isValid(r);
}

}  // namespace Filter
}  // namespace SeqLib
