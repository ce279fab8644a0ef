// The wave sort of seqlib_amd/csrc/dev_wave_sort.h on the host: the 64 lanes are a loop around wave_sort_stage, stage by stage, which is what
// the barrier between stages makes of them on the device.  Built with -fsanitize=address,undefined by tests/test_wave_sort_host.py.
//   - distinct keys: exactly std::sort's permutation, for every size and each of the four orders the kernels use;
//   - slots at and beyond m are neither read (the loads assert) nor written (guard values);
//   - exactly one equal pair at the first, a middle and the last sorted position raises the tie flag, and the list filled again from the
//     saved order is the input.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../../seqlib_amd/csrc/dev_wave_sort.h"

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const int GUARD = 8;
static const int GUARD_VAL = -777;

// keys by handle, as the kernels hold them in LDS
struct Keys {
    std::vector<int64_t> k64;          // re / rb / hash / pos
    std::vector<int> ka, kb;           // score / mapq, qb / alt / rid
};

// the four orders (dev_fin.h: the three region sorts; dev_fin2.h: the hit sort)
static bool less_kind(const Keys &K, int kind, int x, int y)
{
    switch (kind) {
    case 0: return K.k64[x] < K.k64[y];                                                                                         // re
    case 1: { const int sx = K.ka[x], sy = K.ka[y]; const int64_t bx = K.k64[x], by = K.k64[y];                                  // score desc, rb, qb
              return sx > sy || (sx == sy && (bx < by || (bx == by && K.kb[x] < K.kb[y]))); }
    case 2: { const int sx = K.ka[x], sy = K.ka[y]; if (sx != sy) return sx > sy;                                                // score desc, alt, hash
              const int ax = K.kb[x], ay = K.kb[y];
              return ax < ay || (ax == ay && (uint64_t)K.k64[x] < (uint64_t)K.k64[y]); }
    default: { if (K.ka[x] != K.ka[y]) return K.ka[x] > K.ka[y];                                                                 // mapq desc, rid, pos
               if (K.kb[x] != K.kb[y]) return K.kb[x] < K.kb[y];
               return K.k64[x] < K.k64[y]; }
    }
}
static bool same_key(const Keys &K, int kind, int x, int y) { return !less_kind(K, kind, x, y) && !less_kind(K, kind, y, x); }

// keys with few distinct values in the leading fields (so that the later ones decide), no two handles equal under the order
static Keys make_keys(int m, int kind, std::mt19937_64 &rng)
{
    Keys K;
    K.k64.resize(m); K.ka.resize(m); K.kb.resize(m);
    for (int h = 0; h < m; ++h) {
        K.ka[h] = kind == 0 ? 0 : (int)(rng() % (kind == 3 ? 61 : 7)) + (kind == 3 ? 0 : 30);
        K.kb[h] = kind == 2 ? (int)(rng() % 2) : (int)(rng() % 5);
        K.k64[h] = kind == 2 ? (int64_t)rng() : (int64_t)(rng() % (kind == 0 ? (1ull << 40) : 64));          // (hashes use the top bit: compared unsigned)
    }
    std::vector<int> o(m);
    for (int i = 0; i < m; ++i) o[i] = i;
    std::sort(o.begin(), o.end(), [&](int x, int y) { return less_kind(K, kind, x, y); });
    bool dup = false;
    for (int i = 0; i + 1 < m; ++i) dup |= same_key(K, kind, o[i], o[i + 1]);
    if (!dup) return K;
    // the small ranges collide: every handle gets its own value of the field the order reads last, in a shuffled assignment
    std::vector<int> perm(m);
    for (int i = 0; i < m; ++i) perm[i] = i;
    std::shuffle(perm.begin(), perm.end(), rng);
    for (int h = 0; h < m; ++h) {
        if (kind == 1) K.kb[h] = perm[h];
        else if (kind == 2) K.k64[h] = (int64_t)(((uint64_t)perm[h] << 52) ^ (rng() & ((1ull << 52) - 1)));
        else K.k64[h] = (int64_t)perm[h] * 3 - m;          // (negative positions too)
    }
    return K;
}

// handle form: an index array of m slots (+ guards), keys read through the handle
static bool run_handles(int m, std::vector<int> &idx, const Keys &K, int kind)
{
    int *p = idx.data();
    auto load = [&](int i) { if (i < 0 || i >= m) { ++failures; printf("FAIL: load of slot %d, m = %d\n", i, m); return 0; } return p[i]; };
    auto store = [&](int i, int h) { if (i < 0 || i >= m) { ++failures; printf("FAIL: store to slot %d, m = %d\n", i, m); return; } p[i] = h; };
    auto less = [&](int x, int y) { return less_kind(K, kind, x, y); };
    for (WaveSortStage s = wave_sort_begin(); wave_sort_next(m, s);)
        for (int lane = 0; lane < WSORT_LANES; ++lane) wave_sort_stage(m, s, lane, load, store, less);
    bool tie = false;
    for (int lane = 0; lane < WSORT_LANES; ++lane) tie |= wave_sort_tie(m, lane, load, less);
    return tie;
}

// record form (the hit sort): the keys themselves move, the element's number rides in the low bits of the first field
struct Rec { int64_t pos; int rid, mq_e; };
static bool run_records(int m, std::vector<Rec> &rec)
{
    Rec *p = rec.data();
    auto load = [&](int i) { if (i < 0 || i >= m) { ++failures; printf("FAIL: load of record %d, m = %d\n", i, m); return Rec{0, 0, 0}; } return p[i]; };
    auto store = [&](int i, const Rec &r) { if (i < 0 || i >= m) { ++failures; printf("FAIL: store to record %d, m = %d\n", i, m); return; } p[i] = r; };
    auto less = [&](const Rec &a, const Rec &b) {
        const int am = a.mq_e >> 11, bm = b.mq_e >> 11;
        if (am != bm) return am > bm;
        if (a.rid != b.rid) return a.rid < b.rid;
        return a.pos < b.pos;
    };
    for (WaveSortStage s = wave_sort_begin(); wave_sort_next(m, s);)
        for (int lane = 0; lane < WSORT_LANES; ++lane) wave_sort_stage(m, s, lane, load, store, less);
    bool tie = false;
    for (int lane = 0; lane < WSORT_LANES; ++lane) tie |= wave_sort_tie(m, lane, load, less);
    return tie;
}

static void one_case(int m, int kind, std::mt19937_64 &rng)
{
    Keys K = make_keys(m, kind, rng);
    std::vector<int> input(m);
    for (int i = 0; i < m; ++i) input[i] = i;
    std::shuffle(input.begin(), input.end(), rng);
    std::vector<int> expect = input;
    std::sort(expect.begin(), expect.end(), [&](int x, int y) { return less_kind(K, kind, x, y); });

    // ---- distinct keys
    std::vector<int> idx(input);
    idx.resize(m + GUARD, GUARD_VAL);
    bool tie = run_handles(m, idx, K, kind);
    CHECK(!tie, "m %d kind %d: tie flag on distinct keys", m, kind);
    CHECK(std::equal(expect.begin(), expect.end(), idx.begin()), "m %d kind %d: not std::sort's permutation", m, kind);
    for (int g = 0; g < GUARD; ++g) CHECK(idx[m + g] == GUARD_VAL, "m %d kind %d: guard %d changed", m, kind, g);
    if (kind == 3) {          // the same keys as records
        std::vector<Rec> rec(m + GUARD, Rec{-1, -1, -1});
        for (int i = 0; i < m; ++i) rec[i] = Rec{K.k64[input[i]], K.kb[input[i]], K.ka[input[i]] << 11 | input[i]};
        tie = run_records(m, rec);
        CHECK(!tie, "m %d records: tie flag on distinct keys", m);
        bool ok = true;
        for (int i = 0; i < m; ++i) ok &= (rec[i].mq_e & 2047) == expect[i] && rec[i].pos == K.k64[expect[i]] && rec[i].rid == K.kb[expect[i]];
        CHECK(ok, "m %d records: not std::sort's permutation", m);
        for (int g = 0; g < GUARD; ++g) CHECK(rec[m + g].pos == -1 && rec[m + g].rid == -1 && rec[m + g].mq_e == -1, "m %d records: guard %d changed", m, g);
    }

    // ---- exactly one equal pair, at the first, a middle and the last sorted position
    const int at[3] = {0, (m - 2) / 2, m - 2};
    for (int w = 0; w < 3; ++w) {
        if (w > 0 && at[w] == at[w - 1]) continue;
        Keys T = K;
        const int a = expect[at[w]], b = expect[at[w] + 1];
        T.k64[b] = T.k64[a]; T.ka[b] = T.ka[a]; T.kb[b] = T.kb[a];          // (b's keys lay between a's and the next element's: still one pair)
        std::vector<int> saved(input);                                    // what the caller keeps of the order before the sort
        idx.assign(input.begin(), input.end());
        idx.resize(m + GUARD, GUARD_VAL);
        tie = run_handles(m, idx, T, kind);
        CHECK(tie, "m %d kind %d: no tie flag for the equal pair at sorted position %d", m, kind, at[w]);
        bool sorted = true;
        for (int i = 0; i + 1 < m; ++i) sorted &= !less_kind(T, kind, idx[i + 1], idx[i]);
        CHECK(sorted, "m %d kind %d: the list with a tie at %d is not in order", m, kind, at[w]);
        {                                                                 // the network only moved handles: still every handle once, so the saved order is all the caller needs
            std::vector<int> seen(idx.begin(), idx.begin() + m);
            std::sort(seen.begin(), seen.end());
            bool perm = true;
            for (int i = 0; i < m; ++i) perm &= seen[i] == i;
            CHECK(perm, "m %d kind %d: the list with a tie at %d is no permutation of the input", m, kind, at[w]);
        }
        for (int i = 0; i < m; ++i) idx[i] = saved[i];                    // the fall-back's refill
        CHECK(std::equal(input.begin(), input.end(), idx.begin()), "m %d kind %d: refilled list differs from the input", m, kind);
        for (int g = 0; g < GUARD; ++g) CHECK(idx[m + g] == GUARD_VAL, "m %d kind %d tie %d: guard %d changed", m, kind, at[w], g);
        if (kind == 3) {
            std::vector<Rec> rec(m + GUARD, Rec{-1, -1, -1});
            for (int i = 0; i < m; ++i) rec[i] = Rec{T.k64[input[i]], T.kb[input[i]], T.ka[input[i]] << 11 | input[i]};
            CHECK(run_records(m, rec), "m %d records: no tie flag for the equal pair at sorted position %d", m, at[w]);
        }
    }
}

int main()
{
    static const int sizes[] = {2, 3, 63, 64, 65, 127, 128, 129, 511, 640, 769, 1000, 2047, 2048};
    std::mt19937_64 rng(20240611);
    int cases = 0;
    // the stage count the notes quote: log2(k) * (log2(k) + 1) / 2 for the first power of two k >= m
    {
        int n512 = 0, n1000 = 0, n2048 = 0;
        for (WaveSortStage s = wave_sort_begin(); wave_sort_next(512, s);) ++n512;
        for (WaveSortStage s = wave_sort_begin(); wave_sort_next(1000, s);) ++n1000;
        for (WaveSortStage s = wave_sort_begin(); wave_sort_next(2048, s);) ++n2048;
        CHECK(n512 == 45 && n1000 == 55 && n2048 == 66, "stages: %d %d %d", n512, n1000, n2048);
        WaveSortStage s = wave_sort_begin();
        CHECK(!wave_sort_next(0, s) && !wave_sort_next(1, s), "a list of 0 or 1 has no stage");
    }
    for (int m : sizes)
        for (int kind = 0; kind < 4; ++kind)
            for (int rep = 0; rep < (m <= 129 ? 4 : 2); ++rep) { one_case(m, kind, rng); ++cases; }
    // sorted, reversed and rotated inputs of every size up to 130 (every partial last block of the small networks)
    for (int m = 2; m <= 130; ++m) {
        Keys K;
        K.k64.resize(m); K.ka.assign(m, 0); K.kb.assign(m, 0);
        for (int h = 0; h < m; ++h) K.k64[h] = (int64_t)h * 5 - 100;
        for (int form = 0; form < 3; ++form) {
            std::vector<int> idx(m + GUARD, GUARD_VAL);
            for (int i = 0; i < m; ++i) idx[i] = form == 0 ? i : form == 1 ? m - 1 - i : (i + m / 3) % m;
            const bool tie = run_handles(m, idx, K, 0);
            bool ok = !tie;
            for (int i = 0; i < m; ++i) ok &= idx[i] == i;
            for (int g = 0; g < GUARD; ++g) ok &= idx[m + g] == GUARD_VAL;
            CHECK(ok, "m %d form %d: wrong order", m, form);
            ++cases;
        }
    }
    printf("wave_sort_test: cases %d, failures %d\n", cases, failures);
    return failures ? 1 : 0;
}
