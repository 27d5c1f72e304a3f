// drgnn_fcc.h -- clustering of docking poses by their fraction of common contacts (FCC; Rodrigues et al. 2012, the rule of
// HADDOCK's cluster_fcc with the tie between equally connected centres made deterministic).  tests/fcc_ref.py states the
// rule in numpy; everything here is integer-valued except two fp64 divisions per pose pair, so the results are held to
// exact equality.
//
//   contacts  residue pair (a in chain 0, b in chain 1) of pose m is a contact iff an atom of a and an atom of b lie at
//             if_d2 <= cut2 (fp32, no contraction; cut2 = (float)(cutoff * cutoff), the product taken in fp64).  The atoms
//             given are the counted atoms: the caller leaves hydrogens out of xyz / atom_ptr when they do not count.
//             bits u64 [M, nA, WB], WB = ceil(nB / 64): bit b % 64 of word b / 64 of row a; n[m] = the number of set bits
//   common    common[i, j] = sum over the words of popcount(bits_i & bits_j), int32
//   relation  fcc(i, j) = n_i == 0 ? 0.0 : (double)common[i, j] / (double)n_i; j is a neighbour of i iff i != j and
//             fcc(i, j) >= cut_fwd and fcc(j, i) >= cut_rev (directed): FccRule and its `related`.  The bit rows of the
//             relation and the greedy loop on them are rule-independent: pc_relation and pc_greedy of
//             drgnn_posecluster.h, which the RMSD rule of drgnn_rmsd.h runs too
//
// Kernels (one launch each):
//   fc_pose      one workgroup per pose.  Phase 0: lanes over the residues, a bounding sphere each (its centre is the
//                fp32 centroid, its radius the largest distance of an atom from THAT stored centre) into LDS.  Phase 1: a
//                wave owns 64 consecutive chain-1 residues of one chain-0 residue; a lane decides its pair (sphere test,
//                then the atom pairs) and the wave's ballot IS the 64-bit word: one plain store, lanes past nB vote 0, so
//                the tail bits are zero.  The count is the sum of the popcounts: per wave in a register, the 16 partial
//                sums through LDS, added by one lane.
//   fc_common    one workgroup per FC_TILE x FC_TILE tile of pose pairs, one lane per pair; the words of the 2 x FC_TILE
//                poses go through LDS FC_KW at a time (rows padded by one word: the lanes of a wave read FC_TILE rows).
// The sphere test is conservative: with the stored centre c and r >= |x - c| up to rounding for every atom x of the
// residue, two atoms within cut imply |ca - cb| <= cut + ra + rb.  The fp32 rounding of if_d2, sqrt and the sums is below
// 1e-6 relative plus one step of a coordinate (1e-3 A at |x| < 10^4); the test allows (cut + ra + rb) * 1.0001 + 0.01 A,
// so it never drops a pair the atoms keep.  A residue without atoms has radius -1 and no contact.
// Host emulation (DRGNN_EMU): a "wave" is a loop over its 64 lanes.
#pragma once
#include "drgnn_rt.h"
#include "drgnn_iface.h"
#include "drgnn_posecluster.h"

#define FC_RCAP 3072                 // residues of a complex, both chains: 16 B of sphere each in LDS (48 KiB)
#define FC_PCAP 16384                // poses on either side of one drgnn_pose_common call: the output stays below 2^28 ints
#define FC_TILE 32                   // pose pairs per workgroup of fc_common: FC_TILE^2 = the workgroup's lanes
#define FC_KW 64                     // words staged at a time: 2 * FC_TILE * (FC_KW + 1) * 8 B = 33 KiB

struct FccContactArgs {
    const float* xyz;                // [M, T, 3]
    const int32_t* atom_ptr;         // [R + 1]
    int n_atoms, n_res, n_a;         // T, R, residues of chain 0
    float cut, cut2;
    pc_word* bits;                   // [M, nA, WB]
    int32_t* n_contacts;             // [M]
};
struct FccContactShared {
    float sphere[FC_RCAP][4];
    int wave_count[DRGNN_NTHREADS / DRGNN_WAVE];
};

struct FccCommonArgs {
    const pc_word* a;                // [Ma, W]
    const pc_word* b;                // [Mb, W]
    int n_a, n_b;
    int64_t n_words;
    int32_t* common;                 // [Ma, Mb]
};
struct FccCommonShared {
    pc_word a[FC_TILE][FC_KW + 1], b[FC_TILE][FC_KW + 1];
};

struct FccRule {                     // the rule of the neighbour relation (pc_relation of drgnn_posecluster.h)
    const int32_t* common;           // [M, M]
    const int32_t* n_contacts;       // [M]
    int n;
    double cut_fwd, cut_rev;
};

// ---- contacts -------------------------------------------------------------------------------------------------------
// the exact rule for residues ra (chain 0) and rb (chain 1, a global residue index) of the pose at X, behind the sphere test
DEV bool fc_pair(const FccContactArgs& a, const float* X, const FccContactShared& s, int ra, int rb) {
    const float* sa = s.sphere[ra];
    const float* sb = s.sphere[rb];
    if (sa[3] < 0.f || sb[3] < 0.f) return false;
    const float thr = (a.cut + sa[3] + sb[3]) * 1.0001f + 0.01f;
    if (!(if_d2(sa[0], sa[1], sa[2], sb[0], sb[1], sb[2]) <= thr * thr)) return false;
    const int a0 = a.atom_ptr[ra], a1 = a.atom_ptr[ra + 1], b0 = a.atom_ptr[rb], b1 = a.atom_ptr[rb + 1];
    for (int p = a0; p < a1; ++p) {
        const float ax = X[3 * p], ay = X[3 * p + 1], az = X[3 * p + 2];
        for (int q = b0; q < b1; ++q)
            if (if_d2(ax, ay, az, X[3 * q], X[3 * q + 1], X[3 * q + 2]) <= a.cut2) return true;
    }
    return false;
}

// One workgroup: pose m
DEV void fc_pose(const FccContactArgs& a, int64_t m, FccContactShared& s) {
    const float* X = a.xyz + m * (int64_t)a.n_atoms * 3;
    const int nA = a.n_a, nB = a.n_res - a.n_a, WB = (nB + 63) / 64;
    pc_word* out = a.bits + m * (int64_t)nA * WB;
    // ---- 0 spheres
    FOR_TID(r, a.n_res) {
        const int p0 = a.atom_ptr[r], p1 = a.atom_ptr[r + 1];
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int p = p0; p < p1; ++p) { sx += X[3 * p]; sy += X[3 * p + 1]; sz += X[3 * p + 2]; }
        const double n = (double)(p1 - p0);
        const float cx = p1 > p0 ? (float)(sx / n) : 0.f, cy = p1 > p0 ? (float)(sy / n) : 0.f, cz = p1 > p0 ? (float)(sz / n) : 0.f;
        float far2 = 0.f;
        for (int p = p0; p < p1; ++p) {
            const float d = if_d2(X[3 * p], X[3 * p + 1], X[3 * p + 2], cx, cy, cz);
            far2 = d > far2 ? d : far2;
        }
        s.sphere[r][0] = cx; s.sphere[r][1] = cy; s.sphere[r][2] = cz;
        s.sphere[r][3] = p1 > p0 ? IF_SQRT(far2) : -1.f;
    }
    BARRIER();
    // ---- 1 words
#ifdef DRGNN_EMU
    int count = 0;
    for (int it = 0; it < nA * WB; ++it) {
        const int ra = it / WB, w = it % WB;
        pc_word word = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int b = 64 * w + lane;
            if (b < nB && fc_pair(a, X, s, ra, nA + b)) word |= (pc_word)1 << lane;
        }
        out[it] = word;
        count += pc_popc(word);
    }
    a.n_contacts[m] = count;
#else
    const int wave = (int)threadIdx.x / DRGNN_WAVE, lane = (int)threadIdx.x % DRGNN_WAVE;
    const FastDiv fd = fastdiv_make(WB);
    int count = 0;                                                   // (the same on every lane of the wave)
    for (int it = wave; it < nA * WB; it += DRGNN_NWAVES) {
        const int ra = fastdiv(fd, it), w = fastmod(fd, it, ra);
        const int b = 64 * w + lane;
        const pc_word word = __ballot(b < nB && fc_pair(a, X, s, ra, nA + b));
        if (lane == 0) out[it] = word;
        count += pc_popc(word);
    }
    if (lane == 0) s.wave_count[wave] = count;
    BARRIER();
    FOR_TID(i, 1) {
        int total = 0;
        for (int k = 0; k < DRGNN_NWAVES; ++k) total += s.wave_count[k];
        a.n_contacts[m] = total;
    }
#endif
}

// ---- common contacts ------------------------------------------------------------------------------------------------
// One workgroup: the pairs (FC_TILE * ti + y, FC_TILE * tj + x)
DEV void fc_common(const FccCommonArgs& a, int ti, int tj, FccCommonShared& s) {
    const int i0 = ti * FC_TILE, j0 = tj * FC_TILE;
#ifdef DRGNN_EMU
    (void)s;
    for (int i = i0; i < imin(i0 + FC_TILE, a.n_a); ++i)
        for (int j = j0; j < imin(j0 + FC_TILE, a.n_b); ++j) {
            int acc = 0;
            for (int64_t k = 0; k < a.n_words; ++k) acc += pc_popc(a.a[i * a.n_words + k] & a.b[j * a.n_words + k]);
            a.common[(int64_t)i * a.n_b + j] = acc;
        }
#else
    const int y = (int)threadIdx.x / FC_TILE, x = (int)threadIdx.x % FC_TILE;
    int acc = 0;
    for (int64_t k0 = 0; k0 < a.n_words; k0 += FC_KW) {
        const int nk = (int)(a.n_words - k0 < FC_KW ? a.n_words - k0 : FC_KW);
        FOR_TID(e, 2 * FC_TILE * FC_KW) {                              // consecutive lanes: consecutive words of one pose
            const int side = e / (FC_TILE * FC_KW), row = (e / FC_KW) % FC_TILE, k = e % FC_KW;
            const int pose = (side ? j0 : i0) + row;
            pc_word v = 0;
            if (k < nk && pose < (side ? a.n_b : a.n_a)) v = (side ? a.b : a.a)[(int64_t)pose * a.n_words + k0 + k];
            if (side) s.b[row][k] = v; else s.a[row][k] = v;
        }
        BARRIER();
        for (int k = 0; k < nk; ++k) acc += pc_popc(s.a[y][k] & s.b[x][k]);
        BARRIER();
    }
    if (i0 + y < a.n_a && j0 + x < a.n_b) a.common[(int64_t)(i0 + y) * a.n_b + j0 + x] = acc;
#endif
}

// ---- neighbour relation ---------------------------------------------------------------------------------------------
DEV double fc_fraction(int common, int n) { return n == 0 ? 0.0 : (double)common / (double)n; }
// bits of pose pair (i, j): 1 j is a neighbour of i, 2 i is a neighbour of j (the rule pc_relation asks)
DEV int related(const FccRule& a, int i, int j) {
    if (i == j) return 0;
    const double fij = fc_fraction(a.common[(int64_t)i * a.n + j], a.n_contacts[i]);
    const double fji = fc_fraction(a.common[(int64_t)j * a.n + i], a.n_contacts[j]);
    return ((fij >= a.cut_fwd && fji >= a.cut_rev) ? 1 : 0) | ((fji >= a.cut_fwd && fij >= a.cut_rev) ? 2 : 0);
}
