/* The record index of the BAM reader (seqlib_amd/csrc/dev_bamidx.h: k_bam_guess / k_bam_round / k_bam_fill) restated in scalar C and held against the plain
 * chain walk: the stream (argv[1]: block_size-prefixed BAM records, possibly cut at the end) is split into chunks of argv[2] bytes; every chunk but the
 * first guesses its first record start (a whole record with a plausible header from which three more chain, or the end of the stream), is walked from its guess, and a
 * resolution pass confirms chunk 0, then every chunk whose guess equals its predecessor's confirmed exit, and walks the others again from the true entry.
 * argv[3] = number of references, argv[4] = 1 forces every guess wrong.  Prints one JSON line: records, whether the starts equal the serial walk's, the
 * repaired chunks, the bytes of whole records. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NONE UINT64_MAX
static const uint8_t *S;
static uint64_t N;
static int32_t NREF;

static uint32_t u32(uint64_t o) { uint32_t v; memcpy(&v, S + o, 4); return v; }
static uint16_t u16(uint64_t o) { uint16_t v; memcpy(&v, S + o, 2); return v; }

/* header at o looks like a record's; *nx = where the next one would start */
static int plausible(uint64_t o, uint64_t *nx)
{
    if (o + 36 > N) return 0;
    uint64_t bs = u32(o);
    int32_t rid = (int32_t)u32(o + 4), l_seq = (int32_t)u32(o + 20), mrid = (int32_t)u32(o + 24);
    unsigned l_name = S[o + 12], n_cig = u16(o + 16);
    if (l_name < 1 || l_seq < 0) return 0;
    if (rid < -1 || rid >= NREF || mrid < -1 || mrid >= NREF) return 0;
    if (bs < 32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq) return 0;
    if (o + 36 + l_name - 1 < N && S[o + 36 + l_name - 1] != 0) return 0;
    *nx = o + 4 + bs;
    return 1;
}

static uint64_t guess(uint64_t cs, uint64_t ce)
{
    for (uint64_t o = cs; o < ce; ++o) {
        uint64_t q;
        if (!plausible(o, &q) || q > N) continue;      /* the first record of a chain is whole */
        int ok = 1;
        for (int j = 0; j < 3; ++j) {
            if (q + 36 > N) break;                      /* the end of the stream */
            if (!plausible(q, &q)) { ok = 0; break; }
            if (q > N) break;                           /* the record that the end of the stream cuts */
        }
        if (ok) return o;
    }
    return NONE;
}

/* whole records starting in [e, ce): appended to out (if any); returns the exit; *cut set when the stream's end cuts a record (exit = its start) */
static uint64_t walk(uint64_t e, uint64_t ce, uint64_t *out, uint64_t *n_out, int *cut)
{
    while (e < ce) {
        if (e + 4 > N || e + 4 + (uint64_t)u32(e) > N) { *cut = 1; return e; }
        if (out) out[*n_out] = e;
        ++*n_out;
        e += 4 + (uint64_t)u32(e);
    }
    return e;
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END); N = (uint64_t)ftell(f); fseek(f, 0, SEEK_SET);
    uint8_t *buf = malloc(N + 1);
    if (fread(buf, 1, N, f) != N) return 2;
    fclose(f);
    S = buf;
    const uint64_t C = strtoull(argv[2], 0, 10);
    NREF = atoi(argv[3]);
    const int fail = atoi(argv[4]);
    const uint64_t K = (N + C - 1) / C;
    /* the serial walk */
    uint64_t *ref = malloc(8 * (N / 4 + 2)), n_ref_rec = 0;
    int cut0 = 0;
    const uint64_t end0 = walk(0, N, ref, &n_ref_rec, &cut0);
    /* speculate */
    uint64_t *g = malloc(8 * (K + 1)), *ex = malloc(8 * (K + 1)), *cnt = malloc(8 * (K + 1));
    char *cutk = calloc(K + 1, 1);
    for (uint64_t k = 0; k < K; ++k) {
        const uint64_t cs = k * C, ce = cs + C < N ? cs + C : N;
        g[k] = k ? guess(cs, ce) : 0;
        if (k && fail) g[k] = g[k] == NONE ? cs : g[k] + 1;
        cnt[k] = 0; ex[k] = NONE;
        if (g[k] != NONE) { int c = 0; uint64_t n = 0, *tmp = malloc(8 * (C / 4 + 2)); ex[k] = walk(g[k], ce, tmp, &n, &c); cnt[k] = n; cutk[k] = (char)c; free(tmp); }
    }
    /* resolve: chunk 0 is confirmed; chunk k is confirmed when its guess is its predecessor's confirmed exit (or it guessed "none" and indeed no record
     * starts in it); the others are walked again from the true entry */
    uint64_t repaired = 0, entry = 0, total = 0;
    int cut = 0;
    uint64_t *got = malloc(8 * (N / 4 + 2)), n_got = 0;
    for (uint64_t k = 0; k < K; ++k) {
        const uint64_t cs = k * C, ce = cs + C < N ? cs + C : N;
        (void)cs;
        int none_ok = g[k] == NONE && (cut || entry >= ce);
        if (g[k] == NONE && !none_ok) {          /* "none" also holds when the only start in the chunk is the record that the end of the stream cuts */
            uint64_t n = 0; int c = 0;
            walk(entry, ce, 0, &n, &c);
            none_ok = n == 0;
        }
        if (k && g[k] != entry && !none_ok) ++repaired;
        if (cut) continue;                       /* the cut record swallows the rest */
        if (k == 0 || g[k] == entry) {           /* the speculative walk stands: its count and exit are the true ones */
            uint64_t n = 0; int c = 0;
            const uint64_t x = walk(entry, ce, got + n_got, &n, &c);
            if (n != cnt[k] || x != ex[k] || c != cutk[k]) { printf("{\"error\": \"confirmed chunk %llu differs from its own walk\"}\n", (unsigned long long)k); return 1; }
            n_got += n; entry = x; cut = c;
        } else if (none_ok && (cut || entry >= ce)) {
            /* nothing starts here: the entry passes through */
        } else {
            uint64_t n = 0; int c = 0;
            entry = walk(entry, ce, got + n_got, &n, &c);
            n_got += n; cut = c;
        }
    }
    total = entry;
    int same = n_got == n_ref_rec && total == end0 && cut == cut0;
    for (uint64_t i = 0; same && i < n_got; ++i) same = got[i] == ref[i];
    printf("{\"records\": %llu, \"same\": %d, \"repaired\": %llu, \"chunks\": %llu, \"end\": %llu, \"cut\": %d}\n", (unsigned long long)n_got, same, (unsigned long long)repaired,
           (unsigned long long)K, (unsigned long long)total, cut);
    return same ? 0 : 1;
}
