// drgnn_posecluster.h -- what clustering of docking poses does whatever rule relates two poses: the neighbour relation as
// bit rows and the greedy loop.  A rule is a plain record with a free function
//     DEV int related(const Rule&, int i, int j)      bits of pose pair (i, j): 1 j is a neighbour of i, 2 i is a neighbour of j
// (FccRule of drgnn_fcc.h: the fraction of common contacts; DistRule of drgnn_rmsd.h: a distance matrix under a cutoff).
// tests/fcc_ref.py states the greedy rule in numpy; every output is integer-valued and held to exact equality.
//
//   relation  nb u64 [M, MW], MW = ceil(M / 64): bit j of row i says that j is a neighbour of i; nbt its transpose (bit j
//             of row i: i is a neighbour of j); the tail bits are zero
//   greedy    deg[i] = alive neighbours of i; the centre is the alive pose of largest deg, smallest index on a tie; stop
//             when deg[centre] < min_size - 1; the cluster is the centre and its alive neighbours, which all die
//
// Kernels (one launch each):
//   pc_relation  a wave per (pose i, word of 64 poses j): a lane asks the rule about its pair, two ballots give the word
//                of nb and of nbt, lane 0 stores both; lanes past M vote 0.
//   pc_greedy    ONE workgroup: deg from popcounts, then per cluster an integer max over (deg, -index) keys, the members
//                = nb[centre] & alive, and for every member the alive poses of ITS nbt row lose one (integer atomics on
//                LDS: order-free).  Per step: M keys + members x MW words, not M x MW.
// Host emulation (DRGNN_EMU): a "wave" is a loop over its 64 lanes.
#pragma once
#include "drgnn_rt.h"

#define PC_CCAP 4096                 // poses of one clustering call: deg + member list 8 B each in LDS (32 KiB)
#define PC_KEY_SHIFT 12              // greedy key = deg << 12 | (PC_CCAP - 1 - index)
typedef unsigned long long pc_word;

struct PoseClusterArgs {
    int n, min_size;
    pc_word* nb;                     // [M, MW]
    pc_word* nbt;                    // [M, MW]
    int32_t* labels;                 // [M]
    int32_t* centres;                // [M], the first n_clusters are set
    int32_t* sizes;                  // [M]
    int32_t* n_clusters;             // [1]
};
struct PoseGreedyShared {
    int deg[PC_CCAP];
    int list[PC_CCAP];
    pc_word alive[PC_CCAP / 64], member[PC_CCAP / 64];
    int best, n_list;
};
static_assert(PC_CCAP <= (1 << PC_KEY_SHIFT) && PC_CCAP % 64 == 0, "a pose index fits the low bits of the greedy key");
static_assert(sizeof(PoseGreedyShared) <= 64 * 1024, "the degrees and the member list fit the static LDS of a workgroup");

#ifdef DRGNN_EMU
DEV int pc_popc(pc_word x) { return __builtin_popcountll(x); }
DEV int pc_ctz(pc_word x) { return __builtin_ctzll(x); }
#else
DEV int pc_popc(pc_word x) { return __popcll(x); }
DEV int pc_ctz(pc_word x) { return __ffsll((long long)x) - 1; }
#endif

// ---- neighbour relation ---------------------------------------------------------------------------------------------
// One workgroup: words block * DRGNN_NWAVES .. of the M * MW words, a wave each
template <class Rule>
DEV void pc_relation(const Rule& rule, const PoseClusterArgs& a, int64_t block) {
    const int MW = (a.n + 63) / 64;
#ifdef DRGNN_EMU
    for (int64_t it = block * DRGNN_NWAVES; it < imin((int)((block + 1) * DRGNN_NWAVES), a.n * MW); ++it) {
        const int i = (int)(it / MW), w = (int)(it % MW);
        pc_word fwd = 0, back = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int j = 64 * w + lane;
            const int rel = j < a.n ? related(rule, i, j) : 0;
            if (rel & 1) fwd |= (pc_word)1 << lane;
            if (rel & 2) back |= (pc_word)1 << lane;
        }
        a.nb[it] = fwd;
        a.nbt[it] = back;
    }
#else
    const int64_t it = block * DRGNN_NWAVES + (int)threadIdx.x / DRGNN_WAVE;
    const int lane = (int)threadIdx.x % DRGNN_WAVE;
    if (it >= (int64_t)a.n * MW) return;                             // (the whole wave)
    const int i = (int)(it / MW), w = (int)(it % MW), j = 64 * w + lane;
    const int rel = j < a.n ? related(rule, i, j) : 0;
    const pc_word fwd = __ballot(rel & 1), back = __ballot(rel & 2);
    if (lane == 0) { a.nb[it] = fwd; a.nbt[it] = back; }
#endif
}

// ---- greedy clustering ----------------------------------------------------------------------------------------------
#ifdef DRGNN_EMU
#define PC_WAVE_MAX(v) ((void)0)
#define PC_WAVE_LEADER true
#else
#define PC_WAVE_MAX(v) _Pragma("unroll") for (int x_ = 1; x_ < 64; x_ <<= 1) { const int o_ = __shfl_xor((v), x_, 64); (v) = o_ > (v) ? o_ : (v); }
#define PC_WAVE_LEADER (((int)threadIdx.x & 63) == 0)
#endif
// ONE workgroup
DEV void pc_greedy(const PoseClusterArgs& a, PoseGreedyShared& s) {
    const int M = a.n, MW = (M + 63) / 64;
    FOR_TID(i, M) {
        int d = 0;
        for (int w = 0; w < MW; ++w) d += pc_popc(a.nb[(int64_t)i * MW + w]);
        s.deg[i] = d;
        a.labels[i] = -1;
    }
    FOR_TID(w, MW) s.alive[w] = (w + 1 < MW || M % 64 == 0) ? ~(pc_word)0 : (((pc_word)1 << (M % 64)) - 1);
    FOR_TID(i, 1) { s.best = -1; s.n_list = 0; }
    BARRIER();
    int k = 0;
    for (; k < M; ++k) {
        // the centre: the largest (deg, -index) over the alive poses
        {
#ifdef DRGNN_EMU
            for (int i = 0; i < M; ++i)
                if ((s.alive[i >> 6] >> (i & 63)) & 1) ATOMIC_MAX(&s.best, (s.deg[i] << PC_KEY_SHIFT) | (PC_CCAP - 1 - i));
#else
            int key = -1;
            for (int i = (int)threadIdx.x; i < M; i += DRGNN_NTHREADS)
                if ((s.alive[i >> 6] >> (i & 63)) & 1) key = imax(key, (s.deg[i] << PC_KEY_SHIFT) | (PC_CCAP - 1 - i));
            PC_WAVE_MAX(key)
            if (PC_WAVE_LEADER && key >= 0) ATOMIC_MAX(&s.best, key);
#endif
        }
        BARRIER();
        const int best = s.best;                                      // (the same on every lane: the loop is uniform)
        if (best < 0 || (best >> PC_KEY_SHIFT) < a.min_size - 1) break;
        const int c = PC_CCAP - 1 - (best & (PC_CCAP - 1));
        FOR_TID(w, MW) s.member[w] = (a.nb[(int64_t)c * MW + w] & s.alive[w]) | (w == (c >> 6) ? (pc_word)1 << (c & 63) : 0);
        BARRIER();
        FOR_TID(w, MW) s.alive[w] &= ~s.member[w];
        FOR_TID(i, M) {
            if ((s.member[i >> 6] >> (i & 63)) & 1) {
                a.labels[i] = k;
                s.list[ATOMIC_ADD(&s.n_list, 1)] = i;
            }
        }
        FOR_TID(i, 1) { a.centres[k] = c; a.sizes[k] = (best >> PC_KEY_SHIFT) + 1; s.best = -1; }
        BARRIER();
        // every alive pose that has a member as a neighbour loses one
        const int nl = s.n_list;
        FOR_TID(it, nl * MW) {
            const int j = s.list[it / MW], w = it % MW;
            pc_word x = a.nbt[(int64_t)j * MW + w] & s.alive[w];
            while (x) {
                ATOMIC_ADD(&s.deg[64 * w + pc_ctz(x)], -1);
                x &= x - 1;
            }
        }
        BARRIER();
        FOR_TID(i, 1) s.n_list = 0;
        BARRIER();
    }
    FOR_TID(i, 1) a.n_clusters[0] = k;
}
