// ext_row_exit_test.cpp -- the row exit of the extension's row loop (seqlib_amd/csrc/dev_lane_rows.h: ext_row_bound / ext_row_done; derivation in
// dev_ext_wave.h) on the host: lane_rows_extend with the exit off, strict and relaxed, on rows of exactly the columns a job needs
// (tests/test_ext_row_exit_host.py builds this with -fsanitize=address,undefined and holds what it prints against the checker's ksw_extend2).
//
//   ext_row_exit_test run <cases> <mode>     mode: 0 = exit off, 1 = strict, 2 = relaxed (EXT_ROW_EXIT_*)
//       one line per case:  kind cols h0 w zdrop pen5 pen3 query0 target0 query1 target1
//       (the sequences as digits 0..4, "-" = none; side 0 is walked downwards from the seed, side 1 upwards, as in lane_extend_core)
//       Prints, per case, one line per side that ran:  case side score qle tle gtle gscore max_off aw
//       then per kind:                                 # kind cases trials rows exits        (trials = band trials run, rows = DP rows, exits = trials the exit ended)
//   ext_row_exit_test guard                  the precondition alone: "qlen w h0 neg" lines on stdin -> 0 / 1 per line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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

struct Bases {              // heap arrays of exactly the bases: a fetch outside them is an ASan report.  The loop fetches one target base per row
    const uint8_t *qs, *ts;
    unsigned long long rows;
    int q(int j) const { return qs[j]; }
    int t(int64_t p) { ++rows; return ts[p]; }
};

struct Tally { unsigned long long cases = 0, trials = 0, rows = 0, exits = 0; };

static std::vector<uint8_t> digits(const std::string &s) { std::vector<uint8_t> v; if (s != "-") for (char c : s) v.push_back((uint8_t)(c - '0')); return v; }

static void run_case(int id, int cols, int h0, const slx_opt &o, const std::vector<uint8_t> sq[2], const std::vector<uint8_t> st[2], int mode, Tally &ta)
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
    const MatRows mr = make_matrows(o.mat);
    Bases b{qs, ts, 0};
    uint32_t *mem = (uint32_t *)malloc(LaneWide::bytes(cols));          // all 64 lanes' rows, as in LDS: exactly `cols` columns
    LaneWide row; row.init(mem, cols, id % WAVE);
    unsigned int n_exit = 0;
    lane_rows_extend(sd, h0, o, mr, row, b, [&](int side, const LaneRes &r) {
        printf("%d %d %d %d %d %d %d %d %d\n", id, side, r.score, r.qle, r.tle, r.gtle, r.gscore, r.max_off, r.aw);
        ta.trials += r.aw == o.w ? 1 : 2;
    }, mode, &n_exit);
    ++ta.cases; ta.rows += b.rows; ta.exits += n_exit;
    free(mem); free(qs); free(ts);
}

static int run(const char *path, int mode)
{
    std::ifstream in(path);
    std::string line;
    std::map<std::string, Tally> tally;
    int id = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind, f[4];
        int cols, h0, w, zdrop, pen5, pen3;
        if (!(ss >> kind >> cols >> h0 >> w >> zdrop >> pen5 >> pen3 >> f[0] >> f[1] >> f[2] >> f[3])) { fprintf(stderr, "bad case line %d\n", id); return 2; }
        slx_opt o;
        memset(&o, 0, sizeof o);
        o.a = 1; o.b = 4; o.o_del = o.o_ins = 6; o.e_del = o.e_ins = 1; o.w = w; o.zdrop = zdrop; o.pen_clip5 = pen5; o.pen_clip3 = pen3;
        for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) o.mat[i * 5 + j] = (int8_t)(i == 4 || j == 4 ? -1 : (i == j ? o.a : -o.b));
        const std::vector<uint8_t> sq[2] = {digits(f[0]), digits(f[2])}, st[2] = {digits(f[1]), digits(f[3])};
        run_case(id, cols, h0, o, sq, st, mode, tally[kind]);
        ++id;
    }
    for (const auto &kv : tally) printf("# %s %llu %llu %llu %llu\n", kv.first.c_str(), kv.second.cases, kv.second.trials, kv.second.rows, kv.second.exits);
    return 0;
}

// ext_row_exit_ok for "qlen w h0 neg" lines on stdin (w = the effective band; neg = 1: a negative gap extension penalty), bwa's default penalties otherwise
static int guard()
{
    int qlen, w, h0, neg;
    while (scanf("%d %d %d %d", &qlen, &w, &h0, &neg) == 4) {
        slx_opt o;
        memset(&o, 0, sizeof o);
        o.o_del = o.o_ins = 6; o.e_del = 1; o.e_ins = neg ? -1 : 1;
        printf("%d\n", ext_row_exit_ok(o, qlen, w, h0) ? 1 : 0);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "guard")) return guard();
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], atoi(argv[3]));
    fprintf(stderr, "usage: ext_row_exit_test run <cases> <mode 0|1|2> | guard\n");
    return 2;
}
