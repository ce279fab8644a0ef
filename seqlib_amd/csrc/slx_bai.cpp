// slx_bai.cpp -- the host side of the BAI index (bai_host.h): parsing with every count checked against the bytes left, the query plan, and the host-only
// entry points slx_bai_query / slx_bai_stats / slx_bai_free of include/seqlib_amd_bam.h.  Restated from SAMv1 section 5.2 (htslib is not part of this
// image); where the specification leaves a choice (the linear index's lower bound, merging of touching chunks) the rule is htslib's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "slx_internal.h"
#include "seqlib_amd_bam.h"
#include "bai_host.h"

namespace {
struct Cur {
    const uint8_t *p; uint64_t n, o;
    uint64_t left() const { return n - o; }
    bool u32(uint32_t &v) { if (left() < 4) return false; memcpy(&v, p + o, 4); o += 4; return true; }
    bool u64(uint64_t &v) { if (left() < 8) return false; memcpy(&v, p + o, 8); o += 8; return true; }
};
}

int bai_parse(const uint8_t *p, uint64_t n, const char *name, Bai &out)
{
    out = Bai();
    Cur c{p, n, 0};
    auto bad = [&](const char *what) { slx_set_error("BAI: '%s' is short, truncated or damaged (%s at byte %llu of %llu)", name, what, (unsigned long long)c.o, (unsigned long long)n); return SLX_EIO; };
    uint32_t magic, n_ref;
    if (!c.u32(magic) || memcmp(p, "BAI\1", 4) != 0) return bad("magic");
    if (!c.u32(n_ref) || (int32_t)n_ref < 0 || n_ref > c.left() / 8) return bad("n_ref");          // a reference takes n_bin and n_intv at least
    out.refs.resize(n_ref);
    for (BaiRef &r : out.refs) {
        uint32_t n_bin, n_intv;
        if (!c.u32(n_bin) || (int32_t)n_bin < 0 || n_bin > c.left() / 8) return bad("n_bin");
        r.n_bin = (int32_t)n_bin;
        for (uint32_t b = 0; b < n_bin; ++b) {
            uint32_t bin, n_chunk;
            if (!c.u32(bin) || !c.u32(n_chunk) || (int32_t)n_chunk < 0 || n_chunk > c.left() / 16) return bad("n_chunk");
            if (bin == BAI_META_BIN) {
                if (n_chunk != 2) return bad("pseudo-bin without its two chunks");
                for (uint64_t &m : r.meta) c.u64(m);
                r.has_meta = true;
                continue;
            }
            r.bins.push_back(BaiBin{bin, (uint32_t)r.chunks.size(), n_chunk});
            for (uint32_t k = 0; k < n_chunk; ++k) {
                uint64_t u = 0, v = 0;
                c.u64(u); c.u64(v);
                r.chunks.emplace_back(u, v);
            }
        }
        if (!c.u32(n_intv) || (int32_t)n_intv < 0 || n_intv > c.left() / 8) return bad("n_intv");
        r.ioffset.resize(n_intv);
        for (uint64_t &v : r.ioffset) c.u64(v);
    }
    if (c.left() == 0) return SLX_OK;                        // the trailing n_no_coor is optional
    if (!c.u64(out.n_no_coor)) return bad("n_no_coor");
    out.has_no_coor = true;
    return SLX_OK;
}

int bai_load_file(const char *path, Bai &out)
{
    if (!path) { slx_set_error("BAI: path is null"); return SLX_EINVAL; }
    FILE *f = fopen(path, "rb");
    if (!f) { slx_set_error("BAI: cannot open '%s'", path); return SLX_EIO; }
    std::vector<uint8_t> buf;
    uint8_t tmp[65536];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    const bool err = ferror(f) != 0;
    fclose(f);
    if (err) { slx_set_error("BAI: cannot read '%s'", path); return SLX_EIO; }
    return bai_parse(buf.data(), buf.size(), path, out);
}

void bai_plan(const Bai &b, int tid, int64_t beg, int64_t end, std::vector<std::pair<uint64_t, uint64_t>> &out)
{
    out.clear();
    if (tid < 0 || tid >= (int)b.refs.size()) return;
    if (beg < 0) beg = 0;
    if (end > (1ll << 29)) end = 1ll << 29;
    if (beg >= end) return;
    const BaiRef &r = b.refs[tid];
    const uint64_t n_intv = r.ioffset.size();
    const uint64_t min_off = n_intv ? r.ioffset[std::min<uint64_t>((uint64_t)beg >> 14, n_intv - 1)] : 0;
    const int64_t last = end - 1;
    auto wanted = [&](uint32_t bin) {
        if (bin == 0) return true;
        static const int sh[5] = {26, 23, 20, 17, 14};
        static const uint32_t base[5] = {1, 9, 73, 585, 4681};
        for (int l = 0; l < 5; ++l)
            if (bin >= base[l] + (uint32_t)(beg >> sh[l]) && bin <= base[l] + (uint32_t)(last >> sh[l]) && bin < (l < 4 ? base[l + 1] : 37449u)) return true;
        return false;
    };
    for (const BaiBin &bn : r.bins) {
        if (!wanted(bn.bin)) continue;
        for (uint32_t k = 0; k < bn.n; ++k)
            if (r.chunks[bn.first + k].second > min_off) out.push_back(r.chunks[bn.first + k]);
    }
    std::sort(out.begin(), out.end());
    size_t w = 0;
    for (size_t i = 0; i < out.size(); ++i) {
        if (w && out[i].first <= out[w - 1].second) out[w - 1].second = std::max(out[w - 1].second, out[i].second);
        else out[w++] = out[i];
    }
    out.resize(w);
}

extern "C" int slx_bai_query(const char *bai_path, int tid, int64_t beg, int64_t end, uint64_t **chunks, int64_t *n)
{
    if (!chunks || !n) { slx_set_error("slx_bai_query: null output"); return SLX_EINVAL; }
    *chunks = nullptr; *n = 0;
    Bai b;
    const int rc = bai_load_file(bai_path, b);
    if (rc != SLX_OK) return rc;
    if (tid < 0 || tid >= (int)b.refs.size()) { slx_set_error("slx_bai_query: reference %d is not one of the index's %d", tid, (int)b.refs.size()); return SLX_EINVAL; }
    std::vector<std::pair<uint64_t, uint64_t>> ch;
    bai_plan(b, tid, beg, end, ch);
    uint64_t *o = (uint64_t *)malloc(16 * ch.size() + 16);
    if (!o) { slx_set_error("out of memory"); return SLX_ENOMEM; }
    for (size_t i = 0; i < ch.size(); ++i) { o[2 * i] = ch[i].first; o[2 * i + 1] = ch[i].second; }
    *chunks = o; *n = (int64_t)ch.size();
    return SLX_OK;
}

extern "C" int slx_bai_stats(const char *bai_path, int *n_ref, uint64_t *n_no_coor, int tid, uint64_t *n_mapped, uint64_t *n_unmapped, int *n_bin, int *n_intv)
{
    Bai b;
    const int rc = bai_load_file(bai_path, b);
    if (rc != SLX_OK) return rc;
    if (n_ref) *n_ref = (int)b.refs.size();
    if (n_no_coor) *n_no_coor = b.n_no_coor;
    if (tid < 0) return SLX_OK;                              // the file's two figures only
    if (tid >= (int)b.refs.size()) { slx_set_error("slx_bai_stats: reference %d is not one of the index's %d", tid, (int)b.refs.size()); return SLX_EINVAL; }
    const BaiRef &r = b.refs[tid];
    if (n_mapped) *n_mapped = r.meta[2];
    if (n_unmapped) *n_unmapped = r.meta[3];
    if (n_bin) *n_bin = r.n_bin;
    if (n_intv) *n_intv = (int)r.ioffset.size();
    return SLX_OK;
}

extern "C" void slx_bai_free(void *p) { free(p); }
