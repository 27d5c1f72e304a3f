// drgnn_lddt.h -- the local distance difference test of docking poses (lDDT; Mariani, Biasini, Barbato and Schwede 2013):
// the superposition-free quality measure over all atom pairs of a pose, its inter-chain restriction (the interface lDDT)
// and the per-residue form.  tests/lddt_ref.py states the rule in numpy; everything the kernel produces is an integer, so
// the results are held to exact equality.  Conventions at exact ties are this project's own.
//
//   atoms        only heavy atoms count, on both sides (hydrogens: the name rule of counted_atoms).  A reference atom and a
//                table atom correspond when (chain, res_seq, atom name) are equal.  Table atoms without a partner are
//                ignored; reference atoms without a partner stay in the denominators.
//   pairs        a reference pair is two reference heavy atoms on the table's two chains, of different residues
//                (chain, res_seq), with d_ref < inclusion_radius (strict); d_ref = sqrt((dx dx + dy dy) + dz dz) in fp64 on
//                the reference coordinates, computed once on the host and handed over as fp64
//   preserved    for a threshold t: lo = max(d_ref - t, 0), hi = d_ref + t; a pair with both atoms matched is preserved at t
//                in a pose when lo lo <= d2 <= hi hi, d2 = (dx dx + dy dy) + dz dz in fp64 from the pose's fp32 coordinates,
//                every product and sum rounded on its own (no contraction), no square root on the pose side
//   counts       per pose and threshold the preserved pairs: over all pairs, over the inter-chain ones, and per table
//                residue over the pairs with an end in it (a pair counts for both of its residues)
//   scores       the host's: lddt = sum_t all_t / (K n_pairs), ilddt the same over the inter-chain pairs, per residue over
//                the pairs of the residue (NaN without one); the denominators are the reference's totals
//   left out     the renaming of chemically equivalent atoms, stereochemistry checks, a sequence separation, pose-against-
//                pose matrices
//
// The matched pairs come as entries grouped by owning residue, every pair in both directions: entry_ptr i32 [R + 1], self
// atom (of the owning residue), other atom, d_ref f64.  A pair is inter-chain when exactly one of its atoms lies before
// first_b, the first atom of chain B.  The per-residue counts are then plain segmented sums, and their total over the
// residues is exactly twice the per-pose count.
//
// One workgroup per (LD_RB residues, pass of PP poses).  Its 16 waves take the residues one after another, each the next
// one not yet taken (a counter in LDS), lanes across the residue's entries.  A count is the popcount of the wave's ballot, so
// it is the same on every lane: no wave reduction, no floating-point atomics.  Lane 0 writes the residue's counts and adds
// them to the wave's row in LDS; after the barrier the workgroup adds its sums to counts [M, 2, K] (zeroed by the host side
// in front of the launch) with integer atomics, which commute.  ld_halve then halves counts in place: each pair once.  A
// pose's integers depend on the pose alone: not on M, the pass it shares, the wave that took a residue, its place in the
// batch or the run.
// PP = 1: a lane takes 4 entries at a time, so that 4 index loads and then 24 coordinate loads are in flight together (the
// loop is bound by the latency of its two dependent loads).  PP = 4: the bounds lo^2, hi^2 of an entry serve four poses.
// profiles/lddt_ab.txt has both: PP = 4 is the faster one at 1 024 poses of 1ATN (6.1 against 6.9 ms); at 64 poses, where
// four poses to a pass leave fewer workgroups than compute units, the two are within their spread and the call is bound by
// its host-side checks.  The library takes PP = 4 from LD_FILL workgroups of such passes on.
// Host emulation (DRGNN_EMU): a "wave" is one lane that walks all entries of the residue; wave 0 takes every residue.
#pragma once
#include "drgnn_rt.h"

#define LD_KMAX 8                    // thresholds of one call
#define LD_RB 64                     // residues of a workgroup: its waves take them one after another
#define LD_PPMAX 4                   // poses that share a pass over the list at most
#define LD_FILL 1024                 // workgroups from which on four poses share a pass: four per compute unit
#define LD_MAX_WGS 4194303           // workgroups of one launch: 2^32 / 1024 lanes - 1
#define LD_MAX_Y 65535               // the grid's limit in y

struct LddtArgs {
    const float* xyz;                // [M, T, 3]
    const int32_t* entry_ptr;        // [R + 1]
    const int32_t* self_atom;        // [E] an atom of the owning residue
    const int32_t* other_atom;       // [E]
    const double* d_ref;             // [E]
    double t[LD_KMAX];               // the thresholds, increasing
    int n_thresholds, n_atoms, n_residues, first_b;
    int64_t n_poses, m0;             // poses of the call; the first pose of this launch
    int32_t* counts;                 // [M, 2, K] all, inter; zero on entry, doubled until ld_halve
    int32_t* residue_counts;         // [M, R, 2, K] or null
};

struct LddtShared {
    int32_t sum[DRGNN_NWAVES][LD_PPMAX * 2 * LD_KMAX];       // [wave][pose of the pass, all / inter, threshold]
    int32_t next;                                            // residues of the workgroup taken so far
};

#ifdef DRGNN_EMU
#define LD_LANES 1
#define LD_COUNT(p) ((p) ? 1 : 0)
#define LD_NOFMA
#define LD_UNROLL
#else
#define LD_LANES DRGNN_WAVE
#define LD_COUNT(p) __popcll(__ballot(p))
#define LD_NOFMA _Pragma("clang fp contract(off)")
#define LD_UNROLL _Pragma("unroll")
#endif

// residue r of the poses m0 .. m0 + PP (np of them in the batch): the wave's counts go to residue_counts and are added to the
// wave's row of s.  KT: the thresholds' padded count, 4 or 8 (a.t is zero past K; what is counted there is never read).  A lane
// takes LD_PPMAX / PP entries at a time: their index loads, then their gathers, stand together in front of the arithmetic, with
// no branch between them (an entry past the end reads the last one and counts nothing; a pose past the batch reads pose m0).
template <int PP, int KT> DEV void ld_residue(const LddtArgs& a, int r, int64_t m0, int np, int wave, int lane, LddtShared& s) {
    LD_NOFMA
    constexpr int U = LD_PPMAX / PP;
    const int K = a.n_thresholds;
    const int e0 = a.entry_ptr[r], e1 = a.entry_ptr[r + 1];
    const float* X[PP];
LD_UNROLL
    for (int p = 0; p < PP; ++p) X[p] = a.xyz + 3 * (m0 + (p < np ? p : 0)) * (int64_t)a.n_atoms;
    int all[PP][KT], inter[PP][KT];
LD_UNROLL
    for (int p = 0; p < PP; ++p)
LD_UNROLL
        for (int k = 0; k < KT; ++k) all[p][k] = inter[p][k] = 0;
    for (int c0 = e0; c0 < e1; c0 += U * LD_LANES) {
        bool on[U];
        int i[U], j[U];
        double d[U];
        float pi[U][PP][3], pj[U][PP][3];
LD_UNROLL
        for (int u = 0; u < U; ++u) {
            const int e = c0 + u * LD_LANES + lane;
            on[u] = e < e1;
            const int at = on[u] ? e : e1 - 1;
            i[u] = a.self_atom[at]; j[u] = a.other_atom[at]; d[u] = a.d_ref[at];
        }
LD_UNROLL
        for (int u = 0; u < U; ++u)
LD_UNROLL
            for (int p = 0; p < PP; ++p)
LD_UNROLL
                for (int c = 0; c < 3; ++c) {
                    pi[u][p][c] = X[p][3 * (int64_t)i[u] + c];
                    pj[u][p][c] = X[p][3 * (int64_t)j[u] + c];
                }
LD_UNROLL
        for (int u = 0; u < U; ++u) {
            const bool across = (i[u] < a.first_b) != (j[u] < a.first_b);
            double lo2[KT], hi2[KT];
LD_UNROLL
            for (int k = 0; k < KT; ++k) {
                double lo = d[u] - a.t[k];
                lo = lo > 0.0 ? lo : 0.0;
                const double hi = d[u] + a.t[k];
                lo2[k] = lo * lo;
                hi2[k] = hi * hi;
            }
LD_UNROLL
            for (int p = 0; p < PP; ++p) {
                const double dx = (double)pi[u][p][0] - (double)pj[u][p][0], dy = (double)pi[u][p][1] - (double)pj[u][p][1],
                             dz = (double)pi[u][p][2] - (double)pj[u][p][2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
LD_UNROLL
                for (int k = 0; k < KT; ++k) {
                    const bool kept = on[u] && lo2[k] <= d2 && d2 <= hi2[k];      // (NaN: not preserved)
                    all[p][k] += LD_COUNT(kept);
                    inter[p][k] += LD_COUNT(kept && across);
                }
            }
        }
    }
    if (lane != 0) return;                                             // (the counts are the wave's: the same on every lane)
LD_UNROLL
    for (int p = 0; p < PP; ++p) {
        if (p >= np) break;
        int32_t* out = a.residue_counts ? a.residue_counts + ((m0 + p) * a.n_residues + r) * 2 * (int64_t)K : nullptr;
LD_UNROLL
        for (int k = 0; k < KT; ++k) {
            if (k >= K) break;
            if (out) { out[k] = all[p][k]; out[K + k] = inter[p][k]; }
            s.sum[wave][(p * 2) * LD_KMAX + k] += all[p][k];
            s.sum[wave][(p * 2 + 1) * LD_KMAX + k] += inter[p][k];
        }
    }
}

// the residues a wave takes from its workgroup's: the next one not yet taken, until none is left (residues differ in their
// entries by an order of magnitude: a fixed share would leave the workgroup waiting for its slowest wave)
template <int PP, int KT> DEV void ld_wave(const LddtArgs& a, int blk, int64_t m0, int wave, int lane, LddtShared& s) {
    const int r1 = imin(a.n_residues, (blk + 1) * LD_RB);
    const int np = (int)(a.n_poses - m0 < PP ? a.n_poses - m0 : PP);
    for (;;) {
#ifdef DRGNN_EMU
        const int r = blk * LD_RB + s.next++;
#else
        int taken = 0;
        if (lane == 0) taken = ATOMIC_ADD(&s.next, 1);
        const int r = blk * LD_RB + __builtin_amdgcn_readfirstlane(taken);
#endif
        if (r >= r1) return;                                           // (the wave's)
        ld_residue<PP, KT>(a, r, m0, np, wave, lane, s);
    }
}

// One workgroup: the residues [blk * LD_RB, (blk + 1) * LD_RB) of the poses m0 .. m0 + PP
template <int PP, int KT> DEV void ld_block(const LddtArgs& a, int blk, int64_t m0, LddtShared& s) {
    const int K = a.n_thresholds;
    FOR_TID(i, DRGNN_NWAVES * LD_PPMAX * 2 * LD_KMAX) (&s.sum[0][0])[i] = 0;
    FOR_TID(i, 1) s.next = 0;
    BARRIER();
#ifdef DRGNN_EMU
    for (int wave = 0; wave < DRGNN_NWAVES; ++wave) ld_wave<PP, KT>(a, blk, m0, wave, 0, s);
#else
    ld_wave<PP, KT>(a, blk, m0, (int)threadIdx.x / DRGNN_WAVE, (int)threadIdx.x % DRGNN_WAVE, s);
#endif
    BARRIER();
    FOR_TID(i, PP * 2 * LD_KMAX) {
        const int p = i / (2 * LD_KMAX), c = (i / LD_KMAX) % 2, k = i % LD_KMAX;
        if (k < K && m0 + p < a.n_poses) {
            int total = 0;
            for (int w = 0; w < DRGNN_NWAVES; ++w) total += s.sum[w][i];
            if (total) ATOMIC_ADD(&a.counts[((m0 + p) * 2 + c) * (int64_t)K + k], total);
        }
    }
}

// One item: word i of counts [M, 2, K], every pair counted from both of its residues -> once
DEV void ld_halve_item(const LddtArgs& a, int64_t i) {
    if (i < a.n_poses * 2 * a.n_thresholds) a.counts[i] >>= 1;
}
