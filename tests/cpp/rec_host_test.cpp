// rec_host_test.cpp -- seqlib_amd/csrc/dev_rec.h compiled for the host (lane 0 of 1), run under ASan + UBSan by tests/test_rec_builder.py.
//   rec_host_test <image> <stream out>
// The image (tests/rec_util.py, write_image) holds a synthetic slx_hits, the reads and the names.  Every array goes into a malloc of exactly its size, the
// stream into one of exactly n_bytes and the LDS tile into one of exactly REC_TILE: a read or a store outside is the sanitizer's to report.  Prints
// "refused <SLX code> <REC code> <read>" or "ok <records> <bytes>", then the record offsets on one line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../seqlib_amd/csrc/dev_rec.h"

template <typename T> static T *take(FILE *f, size_t n)
{
    T *p = (T *)malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    if (!p || (n && fread(p, sizeof(T), n, f) != n)) { fprintf(stderr, "short image\n"); exit(2); }
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: rec_host_test <image> <stream out>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t *hdr = take<int64_t>(f, 8);
    const size_t N = (size_t)hdr[0], H = (size_t)hdr[1], Cg = (size_t)hdr[2];
    const int hardclip = (int)hdr[3], xa = (int)hdr[4], on_device = (int)hdr[7];
    rec_in in;
    memset(&in, 0, sizeof in);
    in.n_reads = (int64_t)N; in.n_hits = (int64_t)H; in.hardclip = hardclip;
    int64_t *hit_off = take<int64_t>(f, N + 1), *pos = take<int64_t>(f, H), *cig_off = take<int64_t>(f, H + 1);
    uint64_t *offs = take<uint64_t>(f, N + 1), *name_offs = take<uint64_t>(f, N + 1);
    int32_t *rid = take<int32_t>(f, H), *score = take<int32_t>(f, H), *nm = take<int32_t>(f, H), *na = take<int32_t>(f, H), *n_cigar_ops = take<int32_t>(f, H);
    uint32_t *cigar = take<uint32_t>(f, Cg);
    uint16_t *flag = take<uint16_t>(f, H);
    uint8_t *mapq = take<uint8_t>(f, H), *bases = take<uint8_t>(f, (size_t)hdr[5]), *names = take<uint8_t>(f, (size_t)hdr[6]);
    fclose(f);
    in.hit_off = hit_off; in.pos = pos; in.cig_off = cig_off; in.offs = offs; in.name_offs = name_offs; in.rid = rid; in.score = score; in.nm = nm; in.na = na;
    in.n_cigar_ops = n_cigar_ops; in.cigar = cigar; in.flag = flag; in.mapq = mapq; in.bases = bases; in.names = names;
    std::vector<void *> owned = {hdr, hit_off, pos, cig_off, offs, name_offs, rid, score, nm, na, n_cigar_ops, cigar, flag, mapq, bases, names};
    int rc = 0;
    const int pre = rec_check_result(on_device, xa ? (const void *)hit_off : nullptr);
    if (pre != REC_OK) printf("refused %d %d -1\n", rec_slx_code(pre), pre);
    else {
        // the owner map, the sizes (the wave form as one lane, too: both must agree), the prefix sum
        int64_t *owner = (int64_t *)malloc(H * 8 ? H * 8 : 1);
        rec_meta *meta = (rec_meta *)malloc(H * sizeof(rec_meta) ? H * sizeof(rec_meta) : 1);
        unsigned long long *len = (unsigned long long *)malloc((H + 1) * 8), *rec_off = (unsigned long long *)malloc((H + 1) * 8);
        owned.insert(owned.end(), {owner, meta, len, rec_off});
        for (size_t i = 0; i < N; ++i) for (int64_t k = hit_off[i]; k < hit_off[i + 1]; ++k) owner[k] = (int64_t)i;
        unsigned long long refusal = REC_NO_REFUSAL;
        for (size_t k = 0; k < H; ++k) {
            rec_part p = rec_cigar_part(in, (int64_t)k, 0, 1);
            rec_part q = {0, 0, 0, 0};          // the shares of 64 lanes, added up: what k_rec_size_wide reduces
            for (int lane = 0; lane < 64; ++lane) { const rec_part s = rec_cigar_part(in, (int64_t)k, lane, 64); rec_part_add(q, s); }
            if (p.tstart != q.tstart || p.qlen != q.qlen || p.rlen != q.rlen || p.any_ref != q.any_ref) { fprintf(stderr, "hit %zu: the shared walk differs\n", k); rc = 1; }
            const uint32_t code = rec_size_finish(in, (int64_t)k, owner[k], p, meta, len);
            const unsigned long long key = (unsigned long long)owner[k] << 8 | code;
            if (code != REC_OK && key < refusal) refusal = key;
        }
        len[H] = 0;
        unsigned long long total = 0;
        for (size_t k = 0; k <= H; ++k) { rec_off[k] = total; total += len[k]; }
        if (refusal != REC_NO_REFUSAL) printf("refused %d %d %llu\n", rec_slx_code((int)(refusal & 0xff)), (int)(refusal & 0xff), refusal >> 8);
        else {
            uint8_t *out = (uint8_t *)malloc(total ? total : 1), *lds = (uint8_t *)aligned_alloc(16, REC_TILE);
            owned.insert(owned.end(), {out, lds});
            memset(out, 0xa5, total);
            for (unsigned long long t = 0; t * REC_TILE < total; ++t) {
                memset(lds, 0x5a, REC_TILE);
                rec_fill_tile(in, meta, owner, rec_off, total, t, lds, out, 0, 1);
            }
            FILE *g = fopen(argv[2], "wb");
            if (!g || fwrite(out, 1, total, g) != total) { perror(argv[2]); return 2; }
            fclose(g);
            printf("ok %zu %llu\n", H, total);
            for (size_t k = 0; k <= H; ++k) printf("%llu%c", rec_off[k], k == H ? '\n' : ' ');
        }
    }
    for (void *p : owned) free(p);
    return rc;
}
