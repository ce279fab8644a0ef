// inf_member (seqlib_amd/csrc/dev_inflate.h) as the wave runs it, on the host: `nlanes` threads, a lane each, one shared inf_tables and one shared output, and
// INF_SYNC() a real barrier over the group (tests/cpp/lanes_sim.h).  On the GPU the lanes of a wave run in step, so a missing INF_SYNC() passes by luck; here
// the barrier is the only thing that orders one lane's accesses against another's, so that under ThreadSanitizer an access no INF_SYNC() covers is a report,
// and a lane that leaves a barrier early hangs the group, which the watchdog turns into a failure that names the stream.  tests/test_inflate_foreign.py builds
// this twice (-fsanitize=address,undefined and -fsanitize=thread) and runs it directly:
//   argv[1]  the valid set, repeated {u32 compressed size, u32 ISIZE, deflate bytes}: every lane returns INF_OK and the bytes equal zlib's;
//   argv[2]  the refused set, repeated {u32 size, u32 ISIZE, u32 expected code or 0 for any non-zero, bytes}: every lane returns the same code, non-zero exactly
//            when zlib does not end the stream with ISIZE bytes, and the code named where one is.
// For 7 and for 64 lanes.  Prints "<nlanes> lanes <valid> valid <refused> refused <bad> bad" for each.
#include <pthread.h>
#include <signal.h>
#include <unistd.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <zlib.h>
#include "lanes_sim.h"

static thread_local pthread_barrier_t *tl_bar;
#define INF_SYNC() pthread_barrier_wait(tl_bar)
#include "../../seqlib_amd/csrc/dev_inflate.h"

struct Case { std::vector<uint8_t> comp; uint32_t isize, code; bool valid; };

static std::vector<Case> load(const char *path, bool valid)
{
    std::vector<Case> out;
    FILE *f = fopen(path, "rb");
    if (!f) { printf("cannot open %s\n", path); exit(2); }
    uint32_t h[3] = {0, 0, 0};
    while (fread(h, 4, valid ? 2 : 3, f) == (valid ? 2u : 3u)) {
        Case c; c.comp.resize(h[0]); c.isize = h[1]; c.code = valid ? 0 : h[2]; c.valid = valid;
        if (h[0] && fread(c.comp.data(), 1, h[0], f) != h[0]) exit(2);
        out.push_back(c);
    }
    fclose(f);
    return out;
}

static volatile long g_case = -1;
static volatile int g_nlanes = 0;
static void watchdog(int)
{
    char msg[96];
    const int n = snprintf(msg, sizeof msg, "hung: %d lanes, stream %ld: a lane left a barrier the others wait at\n", g_nlanes, (long)g_case);
    if (write(1, msg, (size_t)n) < 0) { }
    _exit(3);
}

static long run_all(const std::vector<Case> &cases, uint32_t nlanes)
{
    long bad = 0;
    pthread_barrier_t turn;                         // between streams: lane 0 sets up and checks alone
    pthread_barrier_init(&turn, nullptr, nlanes);
    uint8_t *ci = nullptr, *co = nullptr;
    inf_tables *t = nullptr;
    std::vector<int> rc(nlanes);
    g_nlanes = (int)nlanes;
    lanes_run(nlanes, [&](uint32_t lane, const GroupLane &W) {
        tl_bar = &W.g->bar;
        for (size_t k = 0; k < cases.size(); ++k) {
            const Case &c = cases[k];
            const uint32_t n = (uint32_t)c.comp.size();
            if (lane == 0) {
                g_case = (long)k;
                // exact-size heap copies: one byte past either end is a sanitizer report
                ci = (uint8_t *)malloc(n ? n : 1);
                if (n) memcpy(ci, c.comp.data(), n);
                co = (uint8_t *)malloc(c.isize ? c.isize : 1);
                t = (inf_tables *)malloc(sizeof(inf_tables));
                memset(t, 0, sizeof *t);
            }
            pthread_barrier_wait(&turn);
            rc[lane] = inf_member(ci, n, co, c.isize, t, (int)lane, (int)nlanes);
            pthread_barrier_wait(&turn);
            if (lane == 0) {
                std::vector<uint8_t> want(c.isize + 1);
                z_stream zs; memset(&zs, 0, sizeof zs);
                inflateInit2(&zs, -15);
                zs.next_in = (Bytef *)c.comp.data(); zs.avail_in = n; zs.next_out = want.data(); zs.avail_out = c.isize;
                const int zr = inflate(&zs, Z_FINISH);
                const bool zok = zr == Z_STREAM_END && zs.total_out == c.isize;
                inflateEnd(&zs);
                const char *set = c.valid ? "valid" : "refused";
                for (uint32_t l = 1; l < nlanes; ++l)
                    if (rc[l] != rc[0]) { printf("%u lanes, %s %zu: lane %u returns %d, lane 0 %d\n", nlanes, set, k, l, rc[l], rc[0]); ++bad; break; }
                if (zok != c.valid) { printf("%u lanes, %s %zu: zlib %s it\n", nlanes, set, k, zok ? "accepts" : "refuses"); ++bad; }
                if (zok != (rc[0] == INF_OK)) { printf("%u lanes, %s %zu: zlib %s, inf_member %d\n", nlanes, set, k, zok ? "accepts" : "refuses", rc[0]); ++bad; }
                else if (zok && memcmp(co, want.data(), c.isize) != 0) { printf("%u lanes, %s %zu: bytes differ from zlib's\n", nlanes, set, k); ++bad; }
                if (c.code && rc[0] != (int)c.code) { printf("%u lanes, %s %zu: code %d, expected %u\n", nlanes, set, k, rc[0], c.code); ++bad; }
                free(ci); free(co); free(t);
            }
        }
    });
    pthread_barrier_destroy(&turn);
    return bad;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::vector<Case> valid = load(argv[1], true), refused = load(argv[2], false);
    std::vector<Case> all = valid;
    all.insert(all.end(), refused.begin(), refused.end());
    signal(SIGALRM, watchdog);
    long bad = 0;
    for (uint32_t nlanes : {7u, 64u}) {
        alarm(60);
        const long b = run_all(all, nlanes);
        alarm(0);
        printf("%u lanes %zu valid %zu refused %ld bad\n", nlanes, valid.size(), refused.size(), b);
        bad += b;
    }
    return bad ? 1 : 0;
}
