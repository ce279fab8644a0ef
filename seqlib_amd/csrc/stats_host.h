// stats_host.h -- the host side of the read statistics (include/seqlib_amd_stats.h): the group registry whose open-addressing table the kernels of dev_stats.h
// probe, the counter names, and the text made from the counts copied down.  Host code only; slx_stats.hip and tests/cpp/stats_host_test.cpp (under ASan + UBSan)
// go over it.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "dev_stats.h"

static const char *const ST_COUNTER_NAMES[ST_C_N] = {"reads", "supp", "qcfail", "duplicate", "unmap", "mate_unmap", "supplementary", "paired", "proper_pair", "read1", "read2",
                                                     "reverse", "bases", "nm_missing"};
static const char *const ST_TEXT_HEADER = "ReadGroup\tReadCount\tSupplementary\tUnmapped\tMateUnmapped\tQCFailed\tDuplicate\tMappingQuality\tNM\tInsertSize\tClippedBases\tMeanPhredScore\tReadLength\n";

static inline int st_counter_index(const char *name)
{
    for (int i = 0; i < ST_C_N; ++i) if (!strcmp(name, ST_COUNTER_NAMES[i])) return i;
    return -1;
}

// Groups in order of first appearance.  slots / koff / pool are what st_tab points at once uploaded: slots[i] = group + 1 or 0, never more than half full, so a
// probe ends at an empty slot.
struct st_groups {
    std::vector<uint32_t> slots, koff = std::vector<uint32_t>(1, 0);
    std::string pool;
    uint32_t n_grown = 0;
    void reset(uint32_t n_slots) { uint32_t p = 2; while (p < n_slots) p <<= 1; slots.assign(p, 0); koff.assign(1, 0); pool.clear(); }
    uint32_t size() const { return (uint32_t)koff.size() - 1; }
    std::string name(uint32_t g) const { return pool.substr(koff[g], koff[g + 1] - koff[g]); }
    void place(uint32_t g)
    {
        const uint32_t mask = (uint32_t)slots.size() - 1;
        uint32_t i = st_hash_bytes((const uint8_t *)pool.data() + koff[g], koff[g + 1] - koff[g]) & mask;
        while (slots[i]) i = (i + 1) & mask;
        slots[i] = g + 1;
    }
    uint32_t find(const uint8_t *key, uint32_t n) const
    {
        const uint32_t mask = (uint32_t)slots.size() - 1;
        for (uint32_t i = st_hash_bytes(key, n) & mask; slots[i]; i = (i + 1) & mask) {
            const uint32_t g = slots[i] - 1;
            if (koff[g + 1] - koff[g] == n && !memcmp(pool.data() + koff[g], key, n)) return g;
        }
        return ST_NO_GROUP;
    }
    // the group of the key, registered when new
    uint32_t intern(const uint8_t *key, uint32_t n)
    {
        uint32_t g = find(key, n);
        if (g != ST_NO_GROUP) return g;
        g = size();
        pool.append((const char *)key, n);
        koff.push_back((uint32_t)pool.size());
        if (2 * (size_t)(g + 1) > slots.size()) {
            slots.assign(2 * slots.size(), 0);
            ++n_grown;
            for (uint32_t k = 0; k < g; ++k) place(k);
        }
        place(g);
        return g;
    }
};

// a histogram's non-empty bins as first_second_count joined by ','
static inline void st_hist_text(const st_lay &L, int h, const uint64_t *row, std::string &out)
{
    bool any = false;
    for (uint32_t k = 0; k < L.nb[h]; ++k) {
        const uint64_t c = row[L.base[h] + 2 + k];
        if (!c) continue;
        if (any) out += ',';
        out += std::to_string(st_bin_lo(&L, h, k)) + "_" + std::to_string(st_bin_hi(&L, h, k)) + "_" + std::to_string(c);
        any = true;
    }
}
// one group's line, without the newline: name, reads, supp, unmap, mate_unmap, qcfail, duplicate, the six histograms
static inline void st_group_text(const st_lay &L, const std::string &name, const uint64_t *row, std::string &out)
{
    static const int order[6] = {ST_C_READS, ST_C_SUPP, ST_C_UNMAP, ST_C_MATE_UNMAP, ST_C_QCFAIL, ST_C_DUP};
    out += name;
    for (int c : order) { out += '\t'; out += std::to_string(row[c]); }
    for (int h = 0; h < ST_N_HIST; ++h) { out += '\t'; st_hist_text(L, h, row, out); }
}
static inline std::string st_text(const st_lay &L, const st_groups &G, const uint64_t *counts)
{
    std::string out = ST_TEXT_HEADER;
    for (uint32_t g = 0; g < G.size(); ++g) { st_group_text(L, G.name(g), counts + (size_t)g * L.row, out); out += '\n'; }
    return out;
}

// a host sink for st_adds: one row
struct st_sink_host {
    uint64_t *row;
    void add(uint32_t entry, uint32_t amount, bool on) { if (on) row[entry] += amount; }
};
