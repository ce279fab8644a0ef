// lane_rows_test.cpp -- the lane kernels' row loop (seqlib_amd/csrc/dev_lane_rows.h) compiled for the host and run on rows of EXACTLY the
// columns the kernel gives a job, so that AddressSanitizer sees any cell the loop touches beyond them (tests/test_lane_rows_host.py builds it
// with -fsanitize=address,undefined and holds what it prints against the checker's ksw_extend2).
//
//   lane_rows_test run <cases>      one line per case:  layout lane cols h0 w zdrop pen5 pen3 query0 target0 query1 target1
//                                   layout: w = LaneWide, n = LaneNarrow; the sequences as digits 0..4, "-" = none; side 0 (left of the seed)
//                                   is walked downwards from the seed, side 1 upwards, as in lane_extend_core.
//                                   Prints, per case, one line per side that ran:  case side score qle tle gtle gscore max_off aw
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <fstream>
#include <sstream>
#include "../../include/seqlib_amd.h"
#include "../../seqlib_amd/csrc/dev_lane_rows.h"

struct MatRows { uint32_t packed[5]; int q4[5]; };          // dev_ext_wave.h's, filled the same way
static MatRows make_matrows(const int8_t *mat)
{
    MatRows m;
    for (int t = 0; t < 5; ++t) {
        m.packed[t] = (uint32_t)(uint8_t)mat[t * 5] | (uint32_t)(uint8_t)mat[t * 5 + 1] << 8 | (uint32_t)(uint8_t)mat[t * 5 + 2] << 16 | (uint32_t)(uint8_t)mat[t * 5 + 3] << 24;
        m.q4[t] = mat[t * 5 + 4];
    }
    return m;
}

struct Bases {              // heap arrays of exactly the bases: a fetch outside them is an ASan report
    const uint8_t *qs, *ts;
    int q(int j) const { return qs[j]; }
    int t(int64_t p) { return ts[p]; }
};

static std::vector<uint8_t> digits(const std::string &s) { std::vector<uint8_t> v; if (s != "-") for (char c : s) v.push_back((uint8_t)(c - '0')); return v; }

template <typename L>
static void run_case(int id, L &row, int h0, const slx_opt &o, const std::vector<uint8_t> sq[2], const std::vector<uint8_t> st[2])
{
    // the read: side 0's query reversed, then side 1's (the seed has no bases here); the reference the same way
    const size_t nq = sq[0].size() + sq[1].size(), nt = st[0].size() + st[1].size();
    uint8_t *qs = (uint8_t *)malloc(nq ? nq : 1), *ts = (uint8_t *)malloc(nt ? nt : 1);
    for (size_t i = 0; i < sq[0].size(); ++i) qs[sq[0].size() - 1 - i] = sq[0][i];
    for (size_t i = 0; i < sq[1].size(); ++i) qs[sq[0].size() + i] = sq[1][i];
    for (size_t i = 0; i < st[0].size(); ++i) ts[st[0].size() - 1 - i] = st[0][i];
    for (size_t i = 0; i < st[1].size(); ++i) ts[st[0].size() + i] = st[1][i];
    LaneSide sd[2];
    sd[0].qlen = (int)sq[0].size(); sd[0].tlen = (int)st[0].size(); sd[0].q0 = (int)sq[0].size() - 1; sd[0].t0 = (int64_t)st[0].size() - 1; sd[0].end_bonus = o.pen_clip5;
    sd[1].qlen = (int)sq[1].size(); sd[1].tlen = (int)st[1].size(); sd[1].q0 = (int)sq[0].size(); sd[1].t0 = (int64_t)st[0].size(); sd[1].end_bonus = o.pen_clip3;
    const MatRows mr = make_matrows(o.mat);
    Bases b{qs, ts};
    lane_rows_extend(sd, h0, o, mr, row, b, [&](int side, const LaneRes &r) {
        printf("%d %d %d %d %d %d %d %d %d\n", id, side, r.score, r.qle, r.tle, r.gtle, r.gscore, r.max_off, r.aw);
    });
    free(qs); free(ts);
}

static int run(const char *path)
{
    std::ifstream in(path);
    std::string line;
    int id = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        char layout; int lane, cols, h0, w, zdrop, pen5, pen3;
        std::string f[4];
        if (!(ss >> layout >> lane >> cols >> h0 >> w >> zdrop >> pen5 >> pen3 >> f[0] >> f[1] >> f[2] >> f[3])) { fprintf(stderr, "bad case line %d\n", id); return 2; }
        slx_opt o;
        memset(&o, 0, sizeof o);
        o.a = 1; o.b = 4; o.o_del = o.o_ins = 6; o.e_del = o.e_ins = 1; o.w = w; o.zdrop = zdrop; o.pen_clip5 = pen5; o.pen_clip3 = pen3;
        for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) o.mat[i * 5 + j] = (int8_t)(i == 4 || j == 4 ? -1 : (i == j ? o.a : -o.b));
        const std::vector<uint8_t> sq[2] = {digits(f[0]), digits(f[2])}, st[2] = {digits(f[1]), digits(f[3])};
        if (layout == 'w') {
            uint32_t *mem = (uint32_t *)malloc(LaneWide::bytes(cols));          // all 64 lanes' rows, as in LDS: exactly `cols` columns
            LaneWide row; row.init(mem, cols, lane);
            run_case(id, row, h0, o, sq, st);
            free(mem);
        } else {
            // the cells and the query codes in blocks of their own, each exactly as long as `cols` columns make it (in LDS the codes follow the cells)
            uint16_t *cells = (uint16_t *)malloc((size_t)cols * WAVE * 2);
            uint32_t *codes = (uint32_t *)malloc((size_t)((cols + 7) / 8) * WAVE * 4);
            LaneNarrow row; row.eh = cells + lane; row.qa = codes + lane;
            run_case(id, row, h0, o, sq, st);
            free(cells); free(codes);
        }
        ++id;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "run")) return run(argv[2]);
    fprintf(stderr, "usage: lane_rows_test run <cases>\n");
    return 2;
}
