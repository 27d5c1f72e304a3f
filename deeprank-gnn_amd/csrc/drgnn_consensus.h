// drgnn_consensus.h -- the contact consensus of docking poses (CONSRANK; Oliva, Vangone and Cavallo 2013): how often a set
// of poses, or every cluster of it, has each residue pair in contact, how well a pose agrees with that, and the contacts
// at least min_count poses share.  O(M) in the poses: what says which few thousand decoys are worth the M^2 stages of
// drgnn_fcc.h / drgnn_rmsd.h.  tests/consensus_ref.py states the rule in numpy; everything here is an integer, so the results
// are held to exact equality.
//
//   inputs     bits u64 [M, nA, WB] as fc_pose leaves them (bit b % 64 of word b / 64 of row a), WB = ceil(nB / 64); the bits
//              of a row's last word at or past nB are IGNORED: never counted, never used as an index.  A grouping as lists:
//              order i32 [L] pose indices, group_ptr i32 [G + 1] offsets into order; a pose may be listed in no group, in one
//              or in several, or several times in one (it then counts as often)
//   counts     i32 [G, nA, nB]: counts[g, a, b] = the listed poses of g with bit (a, b) set
//   residues   i32 [G, nA + nB]: r < nA the listed poses of g with any bit in row r; r >= nA those with bit (a, r - nA) set
//              for some a (poses, not contacts)
//   numerator  i64 [M']: row[m] < 0 ? 0 : the sum of counts[row[m], a, b] over the bits (a, b) of pose m
//   consensus  bits u64 [G, nA, WB]: bit (a, b) iff counts[g, a, b] >= min_count[g]; the tail bits zero; n_contacts i32 [G]
//
// Kernels (one launch each):
//   cs_count     a wave per list entry; the host side zeroes counts and residues in front of the launch (a memset on the
//                stream), and the waves add into them with integer atomics: integer adds commute, so the result has no
//                order in it.  The wave finds its group by bisection of group_ptr, then reads its pose 64 words at a time
//                (512 contiguous bytes); nearly all words are zero, so the ballot of the non-zero ones is walked: the word
//                is broadcast (v_readlane), lane b adds 1 to counts[g, a, 64 w + b] when its bit is set, lane 0 adds 1 to
//                the row's residue count when the row changes (the words of a pose come row by row), and lane w ORs the
//                word into its register: the OR over the rows of word column w, from which lane b adds the residue
//                counts of chain 1 at the end.  No LDS, no barrier.  About two atomics per contact of a pose.
//                (Built first and measured, profiles/consensus_ab.txt: a layout without atomics, a wave per word (a, w)
//                walking the list.  It has to give the OR over ALL rows of a word column to one workgroup, which then
//                reads every line of the bit tensor on one compute unit: 2.2 ms at 8 192 poses of 1ATN.)
//   cs_numer     one workgroup per pose.  A wave loads 64 words of the pose at once; for every non-zero one lane b adds
//                counts[row, a, 64 w + b] when its bit is set and 64 w + b < nB.  int64 sums, through the wave (shuffles)
//                and LDS.
//   cs_bits      CS_BW words of one group per workgroup, CS_BW / DRGNN_NWAVES per wave; the ballot of (b < nB && count >=
//                min_count) IS the word; a wave adds the popcounts of its words to n_contacts[g], zeroed by the host side
//                like counts.
// Host emulation (DRGNN_EMU): a "wave" is a loop over its 64 lanes.
#pragma once
#include "drgnn_rt.h"
#include "drgnn_fcc.h"

#define CS_GCAP 65535                // groups of one call: the grid's y of cs_bits
#define CS_ECAP INT32_MAX            // entries of counts [G, nA, nB]: 32-bit indices
#define CS_NCAP ((int)((1ll << 32) / DRGNN_NTHREADS) - 1)              // poses of one numerator call: a workgroup each, the launch's work-items stay below 2^32
#define CS_PCAP INT32_MAX            // poses and list entries of a counting call: 32-bit indices
#define CS_COUNT_WGS (1 << 16)       // workgroups of cs_count at most: the waves stride over longer lists
#define CS_BW (4 * DRGNN_NWAVES)     // words of a workgroup of cs_bits
static_assert(FC_RCAP <= 64 * DRGNN_WAVE, "a lane per word column of a row");

struct ConsCountArgs {
    const pc_word* bits;             // [M, nA, WB]
    const int32_t* order;            // [L]
    const int32_t* group_ptr;        // [G + 1]
    int n_a, n_b, n_groups;
    int64_t n_listed;
    int32_t* counts;                 // [G, nA, nB], zero on entry
    int32_t* residues;               // [G, nA + nB], zero on entry
};

struct ConsNumerArgs {
    const pc_word* bits;             // [M', nA, WB]
    const int32_t* counts;           // [G, nA, nB]
    const int32_t* row;              // [M']
    int n_a, n_b;
    long long* numerators;           // [M']
};
struct ConsNumerShared {
    long long wave_sum[DRGNN_NWAVES];
};

struct ConsBitsArgs {
    const int32_t* counts;           // [G, nA, nB]
    const int32_t* min_count;        // [G]
    int n_a, n_b;
    pc_word* bits;                   // [G, nA, WB]
    int32_t* n_contacts;             // [G], zero on entry
};

// the bits of word w of a row that are residues: all of them but in a last word with a tail
DEV pc_word cs_valid(int w, int n_b) { return 64 * w + 64 <= n_b ? ~(pc_word)0 : (((pc_word)1 << (n_b - 64 * w)) - 1); }

// ---- counts and residue counts ------------------------------------------------------------------------------------------
// the group of list entry e: the last g with group_ptr[g] <= e (groups without entries are passed over)
DEV int cs_group_of(const ConsCountArgs& a, int64_t e) {
    int lo = 0, hi = a.n_groups;                                       // group_ptr[lo] <= e < group_ptr[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (a.group_ptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// One workgroup: list entries DRGNN_NWAVES * blk + wave, then every n_blocks-th workgroup's worth further on
DEV void cs_count(const ConsCountArgs& a, int blk, int n_blocks) {
    const int nA = a.n_a, nB = a.n_b, WB = (nB + 63) / 64, W = nA * WB;
#ifdef DRGNN_EMU
    for (int64_t e = (int64_t)blk * DRGNN_NWAVES; e < a.n_listed; e += (int64_t)n_blocks * DRGNN_NWAVES)
        for (int64_t p = e; p < e + DRGNN_NWAVES && p < a.n_listed; ++p) {
            const int g = cs_group_of(a, p);
            const pc_word* B = a.bits + (int64_t)a.order[p] * W;
            int32_t* res = a.residues + (int64_t)g * (nA + nB);
            int32_t* cnt = a.counts + (int64_t)g * nA * nB;
            pc_word col[FC_RCAP / 64 + 1] = {0};
            int last_row = -1;
            for (int it = 0; it < W; ++it) {
                const int ra = it / WB, w = it % WB;
                const pc_word word = B[it] & cs_valid(w, nB);
                if (word == 0) continue;
                for (int lane = 0; lane < 64; ++lane)
                    if ((word >> lane) & 1) ATOMIC_ADD(&cnt[(int64_t)ra * nB + 64 * w + lane], 1);
                col[w] |= word;
                if (ra != last_row) ATOMIC_ADD(&res[ra], 1);
                last_row = ra;
            }
            for (int w = 0; w < WB; ++w)
                for (int lane = 0; lane < 64; ++lane)
                    if ((col[w] >> lane) & 1) ATOMIC_ADD(&res[nA + 64 * w + lane], 1);
        }
#else
    const int wave = (int)threadIdx.x / DRGNN_WAVE, lane = (int)threadIdx.x % DRGNN_WAVE;
    const FastDiv fd = fastdiv_make(WB);
    for (int64_t e = (int64_t)blk * DRGNN_NWAVES + wave; e < a.n_listed; e += (int64_t)n_blocks * DRGNN_NWAVES) {      // (the wave's)
        const int g = cs_group_of(a, e);
        const pc_word* B = a.bits + (int64_t)a.order[e] * W;
        int32_t* res = a.residues + (int64_t)g * (nA + nB);
        int32_t* cnt = a.counts + (int64_t)g * nA * nB;
        pc_word col = 0;                                               // lane w: the OR over the rows of word column w
        int last_row = -1;
        for (int c0 = 0; c0 < W; c0 += DRGNN_WAVE) {
            const int it = c0 + lane;
            pc_word word = 0;
            if (it < W) {
                const int ra = fastdiv(fd, it);
                word = B[it] & cs_valid(fastmod(fd, it, ra), nB);
            }
            pc_word mask = __ballot(word != 0);
            while (mask) {                                             // (wave-uniform)
                const int j = pc_ctz(mask);
                mask &= mask - 1;
                const pc_word wj = (pc_word)lane_get_i64((long long)word, j);
                const int ra = fastdiv(fd, c0 + j), w = fastmod(fd, c0 + j, ra);
                if ((wj >> lane) & 1) ATOMIC_ADD(&cnt[(int64_t)ra * nB + 64 * w + lane], 1);
                if (lane == w) col |= wj;
                if (lane == 0 && ra != last_row) ATOMIC_ADD(&res[ra], 1);
                last_row = ra;
            }
        }
        for (int w = 0; w < WB; ++w) {
            const pc_word cw = (pc_word)lane_get_i64((long long)col, w);
            if ((cw >> lane) & 1) ATOMIC_ADD(&res[nA + 64 * w + lane], 1);
        }
    }
#endif
}

// ---- numerators -------------------------------------------------------------------------------------------------------------
// One workgroup: pose m
DEV void cs_numer(const ConsNumerArgs& a, int64_t m, ConsNumerShared& s) {
    const int nA = a.n_a, nB = a.n_b, WB = (nB + 63) / 64, W = nA * WB;
    const int row = a.row[m];
    if (row < 0) {                                                     // (the workgroup's)
        FOR_TID(i, 1) a.numerators[m] = 0;
        return;
    }
    const pc_word* B = a.bits + m * W;
    const int32_t* C = a.counts + (int64_t)row * nA * nB;
#ifdef DRGNN_EMU
    (void)s;
    long long sum = 0;
    for (int it = 0; it < W; ++it) {
        const pc_word word = B[it];
        if (word == 0) continue;
        const int ra = it / WB, w = it % WB;
        for (int lane = 0; lane < 64; ++lane) {
            const int b = 64 * w + lane;
            if (b < nB && ((word >> lane) & 1)) sum += C[(int64_t)ra * nB + b];
        }
    }
    a.numerators[m] = sum;
#else
    const int wave = (int)threadIdx.x / DRGNN_WAVE, lane = (int)threadIdx.x % DRGNN_WAVE;
    const FastDiv fd = fastdiv_make(WB);
    long long sum = 0;
    for (int c0 = wave * DRGNN_WAVE; c0 < W; c0 += DRGNN_NTHREADS) {   // 64 words of the pose at once: nearly all are zero
        const pc_word word = c0 + lane < W ? B[c0 + lane] : 0;
        pc_word mask = __ballot(word != 0);
        while (mask) {                                                 // (wave-uniform)
            const int j = pc_ctz(mask);
            mask &= mask - 1;
            const pc_word wj = (pc_word)lane_get_i64((long long)word, j);
            const int ra = fastdiv(fd, c0 + j), b = 64 * fastmod(fd, c0 + j, ra) + lane;
            if (b < nB && ((wj >> lane) & 1)) sum += C[(int64_t)ra * nB + b];
        }
    }
#pragma unroll
    for (int d = DRGNN_WAVE / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d, DRGNN_WAVE);
    if (lane == 0) s.wave_sum[wave] = sum;
    BARRIER();
    FOR_TID(i, 1) {
        long long total = 0;
        for (int k = 0; k < DRGNN_NWAVES; ++k) total += s.wave_sum[k];
        a.numerators[m] = total;
    }
#endif
}

// ---- consensus bits ---------------------------------------------------------------------------------------------------------
// One workgroup: words [CS_BW * blk, CS_BW * (blk + 1)) of group g
DEV void cs_bits(const ConsBitsArgs& a, int g, int blk) {
    const int nA = a.n_a, nB = a.n_b, WB = (nB + 63) / 64, W = nA * WB;
    const int least = a.min_count[g];
    const int32_t* C = a.counts + (int64_t)g * nA * nB;
    pc_word* out = a.bits + (int64_t)g * W;
    const int i0 = blk * CS_BW, i1 = imin(i0 + CS_BW, W);
#ifdef DRGNN_EMU
    int count = 0;
    for (int it = i0; it < i1; ++it) {
        const int ra = it / WB, w = it % WB;
        pc_word word = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int b = 64 * w + lane;
            if (b < nB && C[(int64_t)ra * nB + b] >= least) word |= (pc_word)1 << lane;
        }
        out[it] = word;
        count += pc_popc(word);
    }
    if (count) ATOMIC_ADD(&a.n_contacts[g], count);
#else
    const int wave = (int)threadIdx.x / DRGNN_WAVE, lane = (int)threadIdx.x % DRGNN_WAVE;
    const FastDiv fd = fastdiv_make(WB);
    int count = 0;                                                     // (the same on every lane of the wave)
#pragma unroll
    for (int k = 0; k < CS_BW / DRGNN_NWAVES; ++k) {
        const int it = i0 + k * DRGNN_NWAVES + wave;
        if (it >= i1) break;                                           // (wave-uniform)
        const int ra = fastdiv(fd, it), b = 64 * fastmod(fd, it, ra) + lane;
        const pc_word word = __ballot(b < nB && C[(int64_t)ra * nB + (b < nB ? b : 0)] >= least);
        if (lane == 0) out[it] = word;
        count += pc_popc(word);
    }
    if (lane == 0 && count) ATOMIC_ADD(&a.n_contacts[g], count);
#endif
}
