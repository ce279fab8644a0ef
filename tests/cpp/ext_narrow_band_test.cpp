// ext_narrow_band_test.cpp -- the narrow band of the extension's row loop (seqlib_amd/csrc/dev_lane_rows.h: ext_narrow_band, LaneSide::wband, LaneRing;
// derivation in dev_ext_wave.h) on the host: lane_rows_extend with and without the clamp, on rows of exactly the columns a job needs
// (tests/test_ext_narrow_host.py builds this with -fsanitize=address,undefined and compares what it prints, with itself and with the checker's ksw_extend2).
//
//   ext_narrow_band_test run <cases> <mode> <clamp>     mode: 0 = exit off, 1 = strict, 2 = relaxed (EXT_ROW_EXIT_*)
//       clamp: 0 = none; 1 = every side gets ext_narrow_band's band, from the loss of its own diagonal and the job's h0 as the lower bound of its start;
//              2 = as 1, and a job whose sides all have a band and whose scores fit 8 bits runs on a LaneRing row (a ring of exactly 32 columns per lane); 3 = as 1 with the band ONE
//              NARROWER (what an off-by-one in the bound would compute)
//       one line per case:  kind cols h0 w zdrop pen5 pen3 query0 target0 query1 target1
//       (the sequences as digits 0..4, "-" = none; side 0 is walked downwards from the seed, side 1 upwards, as in lane_extend_core)
//       Prints, per case, one line per side that ran:  case side score qle tle gtle gscore max_off aw wband loss ring
//       then:                                          # cells <DP cells of all cases>
//   ext_narrow_band_test band     ext_narrow_band alone: "o_del e_del o_ins e_ins zdrop amax L h0 qlen tlen w_eff" lines on stdin -> the band per line
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

// a row policy that counts the cells the loop computes (one put per cell, one per row for eh[end])
template <typename L>
struct Counting : L {
    unsigned long long puts = 0;
    void put(int j, int h, int e, uint32_t old) { ++puts; L::put(j, h, e, old); }
};

static std::vector<uint8_t> digits(const std::string &s) { std::vector<uint8_t> v; if (s != "-") for (char c : s) v.push_back((uint8_t)(c - '0')); return v; }

static unsigned long long run_case(int id, int cols, int h0, const slx_opt &o, const std::vector<uint8_t> sq[2], const std::vector<uint8_t> st[2], int mode, int clamp)
{
    const size_t nq = sq[0].size() + sq[1].size(), nt = st[0].size() + st[1].size();
    uint8_t *qs = (uint8_t *)malloc(nq ? nq : 1), *ts = (uint8_t *)malloc(nt ? nt : 1);
    for (size_t i = 0; i < sq[0].size(); ++i) qs[sq[0].size() - 1 - i] = sq[0][i];
    for (size_t i = 0; i < sq[1].size(); ++i) qs[sq[0].size() + i] = sq[1][i];
    for (size_t i = 0; i < st[0].size(); ++i) ts[st[0].size() - 1 - i] = st[0][i];
    for (size_t i = 0; i < st[1].size(); ++i) ts[st[0].size() + i] = st[1][i];
    LaneSide sd[2];
    sd[0].qlen = (int)sq[0].size(); sd[0].tlen = (int)st[0].size(); sd[0].q0 = (int)sq[0].size() - 1; sd[0].t0 = (int64_t)st[0].size() - 1; sd[0].end_bonus = o.pen_clip5;
    sd[1].qlen = (int)sq[1].size(); sd[1].tlen = (int)st[1].size(); sd[1].q0 = (int)sq[0].size(); sd[1].t0 = (int64_t)st[0].size(); sd[1].end_bonus = o.pen_clip3;
    int amax = 0;
    for (int i = 0; i < 25; ++i) amax = amax > o.mat[i] ? amax : o.mat[i];
    int loss[2] = {-1, -1};
    bool all = true;
    for (int s = 0; s < 2; ++s) {
        if (!sd[s].qlen) continue;
        if (clamp && sd[s].tlen >= sd[s].qlen) {
            loss[s] = 0;
            for (int p = 0; p < sd[s].qlen; ++p) loss[s] += amax - o.mat[st[s][p] * 5 + sq[s][p]];
            int w = ext_narrow_band(o, amax, loss[s], h0, sd[s].qlen, sd[s].tlen, ext_eff_band(o, sd[s].qlen, amax, sd[s].end_bonus, o.w));
            if (clamp == 3 && w >= 0) w = w > 0 ? w - 1 : 0;
            sd[s].wband = w;
        }
        if (sd[s].wband < 0) all = false;
    }
    const bool ring = clamp == 2 && all && h0 + (sd[0].qlen + sd[1].qlen) * amax < 256;          // 8-bit cells: where no score can reach 256, as for LaneNarrow
    const MatRows mr = make_matrows(o.mat);
    Bases b{qs, ts};
    auto done = [&](int side, const LaneRes &r) {
        printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", id, side, r.score, r.qle, r.tle, r.gtle, r.gscore, r.max_off, r.aw, sd[side].wband, loss[side], ring ? 1 : 0);
    };
    unsigned long long cells;
    if (ring) {
        uint32_t *mem = (uint32_t *)malloc(LaneRing::bytes(cols));       // 32 columns of cells for each of the 64 lanes, and the query codes
        Counting<LaneRing> row; row.init(mem, cols, id % WAVE);
        lane_rows_extend(sd, h0, o, mr, row, b, done, mode);
        cells = row.puts;
        free(mem);
    } else {
        uint32_t *mem = (uint32_t *)malloc(LaneWide::bytes(cols));       // all 64 lanes' rows, as in LDS: exactly `cols` columns
        Counting<LaneWide> row; row.init(mem, cols, id % WAVE);
        lane_rows_extend(sd, h0, o, mr, row, b, done, mode);
        cells = row.puts;
        free(mem);
    }
    free(qs); free(ts);
    return cells;
}

static int run(const char *path, int mode, int clamp)
{
    std::ifstream in(path);
    std::string line;
    int id = 0;
    unsigned long long cells = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        std::string kind, f[4];
        int cols, h0, w, zdrop, pen5, pen3;
        if (!(ss >> kind >> cols >> h0 >> w >> zdrop >> pen5 >> pen3 >> f[0] >> f[1] >> f[2] >> f[3])) { fprintf(stderr, "bad case line %d\n", id); return 2; }
        slx_opt o;
        memset(&o, 0, sizeof o);
        o.a = 1; o.b = 4; o.o_del = o.o_ins = 6; o.e_del = o.e_ins = 1; o.w = w; o.zdrop = zdrop; o.pen_clip5 = pen5; o.pen_clip3 = pen3;
        for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) o.mat[i * 5 + j] = (int8_t)(i == 4 || j == 4 ? -1 : (i == j ? o.a : -o.b));
        const std::vector<uint8_t> sq[2] = {digits(f[0]), digits(f[2])}, st[2] = {digits(f[1]), digits(f[3])};
        cells += run_case(id, cols, h0, o, sq, st, mode, clamp);
        ++id;
    }
    printf("# cells %llu\n", cells);
    return 0;
}

static int band()
{
    int od, ed, oi, ei, zdrop, amax, L, h0, qlen, tlen, w_eff;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d", &od, &ed, &oi, &ei, &zdrop, &amax, &L, &h0, &qlen, &tlen, &w_eff) == 11) {
        slx_opt o;
        memset(&o, 0, sizeof o);
        o.o_del = od; o.e_del = ed; o.o_ins = oi; o.e_ins = ei; o.zdrop = zdrop;
        printf("%d\n", ext_narrow_band(o, amax, L, h0, qlen, tlen, w_eff));
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "band")) return band();
    if (argc == 5 && !strcmp(argv[1], "run")) return run(argv[2], atoi(argv[3]), atoi(argv[4]));
    fprintf(stderr, "usage: ext_narrow_band_test run <cases> <mode 0|1|2> <clamp 0|1|2|3> | band\n");
    return 2;
}
