// edit_host.h -- the host side of the record editor that needs no device: the plan as the plan calls of include/seqlib_amd_edit.h build it, and a batch put
// through the bodies of dev_edit.h on the CPU, lane 0 of 1 (what slx_edit_record runs, and tests/cpp/edit_host_test.cpp under sanitizers).  Host code only.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "dev_edit.h"

// the plan and the constants its Z adds point into
struct ed_host_plan {
    ed_plan P;
    std::vector<uint8_t> consts;
    ed_host_plan() { memset(&P, 0, sizeof P); }
};

static inline bool ed_tag_ok(const char *t)
{
    if (!t || !t[0] || !t[1] || t[2]) return false;
    const auto alpha = [](char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); };
    return alpha(t[0]) && (alpha(t[1]) || (t[1] >= '0' && t[1] <= '9'));
}
static inline int ed_find_add(const ed_plan &P, const char *tag)
{
    for (uint32_t a = 0; a < P.n_add; ++a) if (P.add[a].tag == ED_TAG(tag[0], tag[1])) return (int)a;
    return -1;
}
// the plan calls: empty string = done, otherwise what is wrong (SLX_EINVAL)
static inline std::string ed_plan_drop(ed_host_plan &H, const char *tag)
{
    if (!ed_tag_ok(tag)) return "a tag is two bytes in [A-Za-z][A-Za-z0-9]";
    if (H.P.n_drop >= ED_MAX_DROP) return "more than 8 dropped names";
    H.P.drop[H.P.n_drop++] = ED_TAG(tag[0], tag[1]);
    return "";
}
// kind ED_INT: ival; ED_Z: value[0, n); a column: its pointers (and ival = absent).  A column call for a tag whose add is that column already binds in place.
static inline std::string ed_plan_add(ed_host_plan &H, const char *tag, uint32_t kind, int32_t ival, bool replace, const void *value, int64_t n, const void *vals, const void *text,
                                      const void *toff, int64_t n_text)
{
    if (!ed_tag_ok(tag)) return "a tag is two bytes in [A-Za-z][A-Za-z0-9]";
    if (n_text < 0) return "a negative n_text";
    int at = ed_find_add(H.P, tag);
    const bool column = kind == ED_INT_COL || kind == ED_Z_COL;
    if (at >= 0 && !(column && H.P.add[at].kind == kind)) return "a name twice among the adds";
    if (kind == ED_Z) {
        if (!value || n <= 0 || memchr(value, 0, (size_t)n)) return "a constant Z value is not empty and holds no NUL";
        if (H.consts.size() + (size_t)n + 1 > ED_MAX_CONST) return "constants above 4096 bytes in total";
    }
    if (at < 0) {
        if (H.P.n_add >= ED_MAX_ADD) return "more than 8 adds";
        at = (int)H.P.n_add++;
    }
    ed_add &A = H.P.add[at];
    memset(&A, 0, sizeof A);
    A.tag = ED_TAG(tag[0], tag[1]); A.kind = kind; A.replace = replace ? 1 : 0; A.ival = ival;
    if (kind == ED_Z) {
        A.coff = (uint32_t)H.consts.size(); A.clen = (uint32_t)n;
        H.consts.insert(H.consts.end(), (const uint8_t *)value, (const uint8_t *)value + n);
        H.consts.push_back(0);
    }
    A.vals = (const int32_t *)vals; A.text = (const uint8_t *)text; A.toff = (const uint64_t *)toff; A.n_text = (uint64_t)n_text;
    return "";
}

// A batch in host memory through the size step, the sum and the gather, lane 0 of 1.  P's pointers (columns, consts) are host pointers.  ED_OK with the edited
// stream and its n + 1 offsets, or the refusal and in *bad the first record it names.  out and new_off are sized exactly.
static inline uint32_t ed_apply_on_host(const ed_plan &P, const uint8_t *stream, uint64_t n_bytes, const uint64_t *off, uint64_t n, std::vector<uint8_t> *out,
                                        std::vector<unsigned long long> *new_off, uint64_t *bad, std::vector<ed_desc> *desc_out = nullptr)
{
    std::vector<ed_desc> D(n ? n : 1);
    new_off->assign(n + 1, 0);
    *bad = ED_NONE;
    if (n == 0 && n_bytes) { *bad = 0; return ED_E_RECORD; }
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t span = 0, seq_at = 0, aux_at = 0, rc = ED_OK;
        bool own = false;
        uint64_t len = 0;
        if (!ed_span(stream, n_bytes, off, i, n, &span, &own)) rc = ED_E_RECORD;
        else if (own) {
            const uint8_t *rec = stream + (off[i] - off[0]);
            if (!ed_fixed(rec, span, &seq_at, &aux_at)) rc = ED_E_RECORD;
            else rc = ed_size_record<false>(P, rec, span, seq_at, aux_at, i, &D[i], &len, 0, 1);
        }
        if (rc != ED_OK) { *bad = i; return rc; }
        (*new_off)[i + 1] = (*new_off)[i] + len;
    }
    const uint64_t total = (*new_off)[n];
    out->assign(total, 0);
    std::vector<uint8_t> img(ED_TILE + 16);
    uint8_t *lds = img.data() + ((16 - ((uintptr_t)img.data() & 15)) & 15);
    ed_tile T;
    for (uint64_t t = 0; t * ED_TILE < total; ++t) ed_gather_tile(P, stream, off, new_off->data(), D.data(), (int64_t)n, total, t, lds, &T, out->data(), 0, 1);
    if (desc_out) *desc_out = D;
    return ED_OK;
}
