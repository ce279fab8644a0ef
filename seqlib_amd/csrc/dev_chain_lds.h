// dev_chain_lds.h -- k_chain with a light read's chaining state in LDS.
//
// dev_chain_body (dev_chain.h) keeps a read's seeds, chain summaries and the two handle lists in about fifteen columns of the read's
// seed-slot region and reads them back while it works: the binary search over c_pos[ord[m]], a chain's summary on every switch, two
// s_next walks per chain for its weight, head and tail of both chains in the filter's overlap test, the flatten pass.  A light read has
// about nine seeds and one or two chains, so every column it touches is one 64-byte line of which it uses a sixth -- and with some 6 000
// waves x 64 lanes x 15 lines in flight against 4 MB of L2 per XCD nearly every read-back is a miss (measured for the HBM version:
// 2.9 KB fetched and 0.9 KB written per read, 80 L2 requests per read, 67 % of them misses, the waves waiting 90 % of their cycles).
//
// Here the same body runs on LdsWS: the columns are a slice of LDS per lane, and what the later kernels read of them is written to the
// seed-slot region ONCE, when the read is done (commit).  Nothing is read back from HBM, and the columns only this kernel uses are not
// written at all: c_tail, c_kept and ib (the filter's own; ib is a scratch list the extension and finalize kernels fill themselves).
// c_pos is written although no kernel reads it after chaining: the stage dump of slx_debug_stage reports it.
//
// The slice: column-major across the lanes like the rows of dev_ext_lane.h / dev_cig_lane.h -- element k of a 4-byte column is word
// k * 64 + lane, so the 64 lanes of an access fall into 64 different banks whatever k each of them is at; an 8-byte column the same with
// 8-byte elements; a column of handles (a seed or chain number, below 128: one byte) packs four elements into the lane's word of a row.
//
// What does not fit takes k_chain on the HBM columns, unchanged: a read with more than CHAIN_LDS_SEEDS seed slots (decided before
// anything runs) and a read that comes to its 10th chain -- bwa's ordered chain set stops being a single leaf there and dev_kbtree.h
// builds its nodes in the read's region slots; the LDS pass has written nothing to HBM by then, so the read simply starts over.  Such
// reads are one in twenty-five, which with 64 reads per wave is nearly every wave, and they are the long ones (13 to 63 seed slots,
// every step a round trip to HBM): run on the spot, or 64 at a time by the wave that met them, they were 85 % of this kernel's time
// at the two waves per SIMD its slices allow (measured: 16.4 ms alone against k_chain's 19.6).  They go on a list instead, and
// k_chain runs after this kernel with that list as its order, at its own occupancy.
#pragma once
#include "dev_chain.h"

#ifndef SLX_WIDE          // (the 64-bit packing is for contigs; their chunks carry s_score and stay on the HBM columns)

#ifndef CHAIN_LDS_SEEDS
#define CHAIN_LDS_SEEDS 12        // seed slots a read may have to chain in LDS.  Measured on C3 (profiles/NOTES_chain_lds.md): 8 slots (11 waves per CU, 94.4 % of the
                                  // reads) 69.6, 12 (8 waves, 96.0 %) 69.9 / 70.2 / 70.0, 16 (7 waves, 99.2 %) 69.3 / 69.8 / 69.6 M reads/s, off 69.0 / 69.1
#endif

#define LDS_AS __attribute__((address_space(3)))

// element of a column: T is what the algorithm sees (the type of the HBM column), S what the slice stores
template <typename T, typename S>
struct LdsRef {
    LDS_AS S *p;
    __device__ __forceinline__ operator T() const { return (T)*p; }
    __device__ __forceinline__ LdsRef &operator=(T v) { *p = (S)v; return *this; }
    __device__ __forceinline__ LdsRef &operator=(const LdsRef &o) { *p = *o.p; return *this; }
};

// a column of one lane; walks and indexes like a pointer (the sorts of dev_sort.h take it as one)
template <typename T, typename S>
struct LdsCol {
    LDS_AS char *b;               // the lane's element 0
    int k;                        // index this "pointer" stands at
    static_assert(sizeof(S) == 1 || sizeof(S) == 4 || sizeof(S) == 8, "LdsCol: 1-, 4- or 8-byte elements");
    static __host__ __device__ constexpr int rows(int n) { return sizeof(S) == 1 ? (n + 3) / 4 : n * (int)(sizeof(S) / 4); }      // 256-byte rows of n elements
    __device__ __forceinline__ void init(LDS_AS char *slice, int row, int lane) { b = slice + row * 256 + lane * (sizeof(S) == 8 ? 8 : 4); k = 0; }
    __device__ __forceinline__ LdsRef<T, S> operator[](int i) const
    {
        const int e = k + i;
        return LdsRef<T, S>{(LDS_AS S *)(b + (sizeof(S) == 1 ? (e >> 2) * 256 + (e & 3) : e * 64 * (int)sizeof(S)))};
    }
    __device__ __forceinline__ LdsRef<T, S> operator*() const { return (*this)[0]; }
    __device__ __forceinline__ LdsCol operator+(int n) const { return LdsCol{b, k + n}; }
    __device__ __forceinline__ LdsCol operator-(int n) const { return LdsCol{b, k - n}; }
    __device__ __forceinline__ LdsCol &operator++() { ++k; return *this; }
    __device__ __forceinline__ LdsCol &operator--() { --k; return *this; }
    __device__ __forceinline__ bool operator<(const LdsCol &o) const { return k < o.k; }
    __device__ __forceinline__ bool operator>(const LdsCol &o) const { return k > o.k; }
};

// the storage of dev_chain_body in LDS: NS seeds, NC = min(NS, 9) chains (the 10th chain is the kbtree's)
template <typename I, int NS>
struct LdsWS {
    static constexpr bool in_lds = true;
    static constexpr int NC = NS < 2 * KB_T - 1 ? NS : 2 * KB_T - 1;
    static_assert(NS >= 1 && NS < 128, "LdsWS: handles are stored as signed bytes");
    static_assert(sizeof(qp_t) == 4, "LdsWS: 16 + 16-bit packed query positions");
    typedef LdsCol<int64_t, I> PosCol;            // reference positions as the index holds them: below 2 x l_pac, which an I holds
    typedef LdsCol<qp_t, qp_t> QlCol;
    typedef LdsCol<int32_t, int32_t> IntCol;
    typedef LdsCol<int32_t, int8_t> HandleCol;
    typedef LdsCol<int8_t, int8_t> ByteCol;
    PosCol s_rbeg, c_pos;
    QlCol s_ql;
    IntCol c_rid, c_w;
    HandleCol s_next, c_head, c_tail, c_n, c_first, ia, ib;
    ByteCol c_kept;
    static constexpr int32_t *s_score = nullptr;      // (chunks with per-seed scores do not come here)
    DReg *regs;                                   // the exact-match shortcut writes the read's region where it belongs
    ReadWS g;                                     // where commit() writes
    // rows of 256 bytes, the 8-byte columns (if any) first
    static constexpr int R_SRBEG = 0, R_CPOS = R_SRBEG + PosCol::rows(NS), R_SQL = R_CPOS + PosCol::rows(NC), R_CRID = R_SQL + QlCol::rows(NS),
                         R_CW = R_CRID + IntCol::rows(NC), R_SNEXT = R_CW + IntCol::rows(NS), R_CHEAD = R_SNEXT + HandleCol::rows(NS),
                         R_CTAIL = R_CHEAD + HandleCol::rows(NC), R_CN = R_CTAIL + HandleCol::rows(NC), R_CFIRST = R_CN + HandleCol::rows(NC),
                         R_IA = R_CFIRST + HandleCol::rows(NC), R_IB = R_IA + HandleCol::rows(NC), R_CKEPT = R_IB + HandleCol::rows(NC),
                         ROWS = R_CKEPT + ByteCol::rows(NC);
    static __host__ __device__ constexpr size_t bytes() { return (size_t)ROWS * 256; }       // per wave
    __device__ __forceinline__ void init(LDS_AS char *slice, int lane)
    {
        s_rbeg.init(slice, R_SRBEG, lane); c_pos.init(slice, R_CPOS, lane); s_ql.init(slice, R_SQL, lane); c_rid.init(slice, R_CRID, lane);
        c_w.init(slice, R_CW, lane); s_next.init(slice, R_SNEXT, lane); c_head.init(slice, R_CHEAD, lane); c_tail.init(slice, R_CTAIL, lane);
        c_n.init(slice, R_CN, lane); c_first.init(slice, R_CFIRST, lane); ia.init(slice, R_IA, lane); ib.init(slice, R_IB, lane);
        c_kept.init(slice, R_CKEPT, lane);
    }
    __device__ __forceinline__ void bind(const ReadWS &ws) { g = ws; regs = ws.regs; }
    __device__ __forceinline__ int s_qbeg(int s) const { return QP_HI((qp_t)s_ql[s]); }
    __device__ __forceinline__ int s_len(int s) const { return QP_LO((qp_t)s_ql[s]); }
    // no room for seed number ns, or for chain number c
    __device__ __forceinline__ bool full(int ns, int c) const { return ns >= NS || c >= NC; }
    // the read is done: ns seeds, nc chains.  c_w holds the flattened seed lists of the kept chains by now (at most ns entries) or, where
    // the lists stop short, the weights of the chains (nc <= ns entries); entries past both were never set in the slice and go out as they are --
    // nothing reads them, and on the HBM columns they hold whatever the last chunk left there
    __device__ __forceinline__ void commit(int ns, int nc) const
    {
        for (int s = 0; s < ns; ++s) { g.s_rbeg[s] = s_rbeg[s]; g.s_ql[s] = s_ql[s]; g.s_next[s] = s_next[s]; g.c_w[s] = c_w[s]; }
        for (int c = 0; c < nc; ++c) {
            g.c_pos[c] = c_pos[c]; g.c_head[c] = c_head[c]; g.c_n[c] = c_n[c]; g.c_rid[c] = c_rid[c]; g.c_first[c] = c_first[c]; g.ia[c] = ia[c];
        }
    }
};

// left: the reads for the HBM columns (k_chain takes them next, with `left` as its order list); n_left counts them
template <typename I>
__global__ void __launch_bounds__(64) k_chain_lds(DevFM<I> fm, DevRef R, Chunk ck, DevOpt dopt, const int *order, unsigned int *queue, const unsigned int *n_slots,
                                                  int *left, unsigned int *n_left, unsigned int *stat)          // stat[0] += reads that gave the LDS pass up, stat[1] += reads done in LDS
{
    typedef LdsWS<I, CHAIN_LDS_SEEDS> LW;
    extern __shared__ __attribute__((aligned(16))) unsigned char chain_lds_slice[];
    const slx_opt &opt = dopt.o;
    const int n_todo = (int)*n_slots;
    const int lane = threadIdx.x & 63;
    LW lw;
    lw.init((LDS_AS char *)chain_lds_slice, lane);
    unsigned int n_bail = 0, n_lds = 0;
    while (true) {
        const int slot = next_slot(queue);
        if (__all(slot >= n_todo)) break;
        if (slot >= n_todo) continue;
        const int r = order ? order[slot] : slot;
        const ReadWS ws = make_ws(ck, r);
        bool done = false;
        if (ws.cap <= CHAIN_LDS_SEEDS) {
            lw.bind(ws);
            done = dev_chain_body<I>(fm, R, ck, opt, r, lw);
            if (done) ++n_lds; else ++n_bail;
        }
        if (!done) left[wave_fetch_inc(n_left)] = r;
    }
    // two adds per wave
    for (int d = 32; d; d >>= 1) { n_bail += __shfl_xor(n_bail, d); n_lds += __shfl_xor(n_lds, d); }
    if (lane == 0) { if (n_bail) atomicAdd(stat, n_bail); if (n_lds) atomicAdd(stat + 1, n_lds); }
}

#endif  // !SLX_WIDE
