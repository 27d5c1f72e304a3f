// drgnn_rmsd.h -- the pose-by-pose RMSD matrix of docking poses of one topology (pairwise l-RMSD / i-RMSD) and the
// neighbour relation of RMSD clustering (the rule of HADDOCK's cluster_struc and of ClusPro: DistRule and its `related`;
// the bit rows of the relation and the greedy loop are pc_relation and pc_greedy of drgnn_posecluster.h).
// tests/rmsd_ref.py states both rules in numpy.
//
//   distance  poses p_i, p_j (f32 -> f64), an atom list `rms` (nR >= 1) and an atom list `fit` (nF >= 3) or none.
//             Without fit: D[i, j] = sqrt(sum_a |p_i[a] - p_j[a]|^2 / nR) over rms.  With fit: the optimal proper rotation
//             R and translation of pose i's fit atoms onto pose j's, applied to pose i, then the same sum over rms, in
//             its moment form: with both poses centred about their own fit centroid, S = sum p_i p_j^T over fit gives
//             Horn's 4 x 4 matrix, its largest eigenvector the rotation, and with C = sum p_i p_j^T and A = sum |p|^2
//             over rms:  D^2 = (A_i + A_j - 2 sum_jk R[k][j] C[j][k]) / nR.
//   relation  j is a neighbour of i iff i != j and D[i, j] <= cutoff (fp64, on the stored value; a NaN is no neighbour)
//
// Kernels (one launch each):
//   rm_prepare   one workgroup per pose.  The fit centroid in fp64 by RM_SLOTS fixed slots (slot s takes the atoms s,
//                s + RM_SLOTS, .. in that order) and a pairwise tree, as drgnn_score.h does; then the record of the pose:
//                the centred fp64 coordinates of the fit atoms, of the rms atoms, and sum |x|^2 of both sets (the fit
//                atoms' by slots and tree again; the rms atoms' in the order rm_pairs sums the diagonal of C, so that a
//                pose against a copy of itself is at exactly 0).  No floating-point atomics.
//   rm_pairs     one workgroup per RM_TILE x RM_TILE tile of pose pairs, one lane per pair.  The records of the tile's
//                2 x RM_TILE poses go through LDS RM_K atoms at a time; a row is 3 RM_K + 1 doubles, an odd number, so the
//                32 rows the lanes of a wave read lie on distinct pairs of banks.  A lane keeps S and C in fp64 registers,
//                adding the atoms in the order of the lists: the order depends on the selection only, never on the tile
//                or on M.  Then it fits its pair with the Jacobi routine of drgnn_score.h and writes D.
//                When both sides are the same batch the tiles below the diagonal do nothing, a lane with i < j writes
//                D[i, j] and D[j, i], and the diagonal is written as 0.
// Both directions of a pair have the same bits, whichever side of a call a pose is on: S and C of the reversed pair are
// the exact transposes (a product and a sum do not depend on the order of their operands), and rm_distance evaluates the
// pair in ONE of the two directions, chosen by the sign of the first non-zero of Horn's three antisymmetric entries,
// which the reversal negates exactly.  When all three are zero S is symmetric, the rotation matrix too, and the last sum
// is ordered so that a transposed C gives the same roundings.
// A collinear or coincident fit set leaves the rotation undetermined: the result is then undefined (finite or NaN).
// Host emulation (DRGNN_EMU): a lane is a loop iteration that reads the records from memory in the same order.
#pragma once
#include "drgnn_rt.h"
#include "drgnn_score.h"
#include "drgnn_posecluster.h"

#define RM_PCAP 4096                 // poses on either side of one drgnn_pose_rmsd call: 128 tiles a side
#define RM_TILE 32                   // pose pairs per workgroup: RM_TILE^2 = the workgroup's lanes
#define RM_K 32                      // atoms staged at a time (even: the row of 3 RM_K + 1 doubles is odd)
#define RM_LD (3 * RM_K + 1)         // 2 * RM_TILE * RM_LD * 8 B = 48.5 KiB
#define RM_LOG_SLOTS 7
#define RM_SLOTS (1 << RM_LOG_SLOTS) // accumulation slots of the centroid and of sum |x|^2

struct RmsdArgs {
    const float* xyz_a;              // [Ma, T, 3]
    const float* xyz_b;              // [Mb, T, 3]
    const int32_t* fit_idx;          // [nF]
    const int32_t* rms_idx;          // [nR]
    int n_atoms, n_fit, n_rms, n_a, n_b;
    int same;                        // both sides are one batch: rec_b == rec_a
    double* rec_a;                   // [Ma, 3 nF + 3 nR + 2]: fit coordinates, rms coordinates, sum |x|^2 of fit, of rms
    double* rec_b;                   // [Mb, ..]
    double* d;                       // [Ma, Mb]
};
struct RmsdPrepShared {
    double sum[3][RM_SLOTS];
};
struct RmsdPairShared {
    double a[RM_TILE][RM_LD], b[RM_TILE][RM_LD];
};
struct DistRule {                    // the rule of the neighbour relation (pc_relation of drgnn_posecluster.h)
    const double* d;                 // [M, M]
    int n;
    double cutoff;
};

DEV int64_t rm_record(const RmsdArgs& a) { return 3 * ((int64_t)a.n_fit + a.n_rms) + 2; }

// a product and a sum rounded on their own (no contraction into an FMA), for the one sum that has to round alike for C and C^T
#ifdef DRGNN_EMU
DEV double rm_mul(double x, double y) { volatile double r = x * y; return r; }
DEV double rm_add(double x, double y) { volatile double r = x + y; return r; }
#define RM_FMA(x, y, z) (rm_mul((x), (y)) + (z))                       // the emulation rounds the product
#else
DEV double rm_mul(double x, double y) { return __dmul_rn(x, y); }
DEV double rm_add(double x, double y) { return __dadd_rn(x, y); }
#define RM_FMA(x, y, z) fma((x), (y), (z))                             // one rounding, wherever the compiler would contract or not
#endif

// ---- records --------------------------------------------------------------------------------------------------------
// slot j += slot j + h over `rows` rows of s.sum
DEV void rm_tree(RmsdPrepShared& s, int rows) {
    for (int h = RM_SLOTS / 2, sh = RM_LOG_SLOTS - 1; h >= 1; h >>= 1, --sh) {
        FOR_TID(i, rows * h) {
            const int k = i >> sh, j = i & (h - 1);
            s.sum[k][j] += s.sum[k][j + h];
        }
        BARRIER();
    }
}

// One workgroup: pose m of side `side`
DEV void rm_prepare(const RmsdArgs& a, int side, int64_t m, RmsdPrepShared& s) {
    const float* X = (side ? a.xyz_b : a.xyz_a) + m * (int64_t)a.n_atoms * 3;
    double* rec = (side ? a.rec_b : a.rec_a) + m * rm_record(a);
    const int nF = a.n_fit, nR = a.n_rms;
    // ---- the fit centroid
    FOR_TID(t, RM_SLOTS) {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int i = t; i < nF; i += RM_SLOTS) {
            const float* p = X + 3 * (int64_t)a.fit_idx[i];
            sx += (double)p[0]; sy += (double)p[1]; sz += (double)p[2];
        }
        s.sum[0][t] = sx; s.sum[1][t] = sy; s.sum[2][t] = sz;
    }
    BARRIER();
    rm_tree(s, 3);
    const double n = (double)(nF > 0 ? nF : 1);
    const double cx = s.sum[0][0] / n, cy = s.sum[1][0] / n, cz = s.sum[2][0] / n;     // (0 without a fit list)
    BARRIER();
    // ---- centred coordinates, sum |x|^2 of both lists
    FOR_TID(e, nF + nR) {
        const float* p = X + 3 * (int64_t)(e < nF ? a.fit_idx[e] : a.rms_idx[e - nF]);
        rec[3 * (int64_t)e] = (double)p[0] - cx; rec[3 * (int64_t)e + 1] = (double)p[1] - cy; rec[3 * (int64_t)e + 2] = (double)p[2] - cz;
    }
    FOR_TID(slot, RM_SLOTS) {                                          // sum |x|^2 of the fit atoms: slots and tree
        double acc = 0.0;
        for (int i = slot; i < nF; i += RM_SLOTS) {
            const float* p = X + 3 * (int64_t)a.fit_idx[i];
            const double x = (double)p[0] - cx, y = (double)p[1] - cy, w = (double)p[2] - cz;
            acc += x * x + y * y + w * w;
        }
        s.sum[0][slot] = acc;
    }
    BARRIER();
    rm_tree(s, 1);
    // sum |x|^2 of the rms atoms, summed as rm_pairs sums the diagonal of C: one chain per coordinate in the order of the list,
    // then (xx + yy) + zz.  A pose against a copy of itself (S symmetric, the rotation exactly the identity) then has
    // A_i + A_j - 2 sum R o C = 0 exactly, in whichever call and on whichever side the copy is.
    FOR_TID(j, 3) {
        const double c = j == 0 ? cx : j == 1 ? cy : cz;
        double acc = 0.0;
        for (int i = 0; i < nR; ++i) {
            const double x = (double)X[3 * (int64_t)a.rms_idx[i] + j] - c;
            acc = RM_FMA(x, x, acc);
        }
        s.sum[1][j] = acc;
    }
    BARRIER();
    FOR_TID(z, 1) {
        rec[3 * ((int64_t)nF + nR)] = s.sum[0][0];
        rec[3 * ((int64_t)nF + nR) + 1] = rm_add(rm_add(s.sum[1][0], s.sum[1][1]), s.sum[1][2]);
    }
}

// ---- one pair -------------------------------------------------------------------------------------------------------
// D of a pair from its cross sums S (fit) and C (rms), both [row of pose i][column of pose j], and A_i + A_j
DEV double rm_distance(const double (&S0)[3][3], const double (&C0)[3][3], double ai, double aj, int n_rms) {
    const double h1 = S0[1][2] - S0[2][1], h2 = S0[2][0] - S0[0][2], h3 = S0[0][1] - S0[1][0];
    const bool flip = h1 != 0.0 ? h1 < 0.0 : h2 != 0.0 ? h2 < 0.0 : h3 < 0.0;        // evaluate the reversed pair instead
    double S[3][3], C[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) { S[j][k] = flip ? S0[k][j] : S0[j][k]; C[j][k] = flip ? C0[k][j] : C0[j][k]; }
    double h[4][4];
    h[0][0] = S[0][0] + S[1][1] + S[2][2];
    h[1][1] = S[0][0] - S[1][1] - S[2][2];
    h[2][2] = -S[0][0] + S[1][1] - S[2][2];
    h[3][3] = -S[0][0] - S[1][1] + S[2][2];
    h[0][1] = h[1][0] = S[1][2] - S[2][1];
    h[0][2] = h[2][0] = S[2][0] - S[0][2];
    h[0][3] = h[3][0] = S[0][1] - S[1][0];
    h[1][2] = h[2][1] = S[0][1] + S[1][0];
    h[1][3] = h[3][1] = S[2][0] + S[0][2];
    h[2][3] = h[3][2] = S[1][2] + S[2][1];
    double q[4];
    sc_largest_eigenpair(h, q);
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    double R[3][3];
    R[0][0] = w * w + x * x - y * y - z * z; R[0][1] = 2.0 * (x * y - w * z); R[0][2] = 2.0 * (x * z + w * y);
    R[1][0] = 2.0 * (x * y + w * z); R[1][1] = w * w - x * x + y * y - z * z; R[1][2] = 2.0 * (y * z - w * x);
    R[2][0] = 2.0 * (x * z - w * y); R[2][1] = 2.0 * (y * z + w * x); R[2][2] = w * w - x * x - y * y + z * z;
    // sum_a p_j[a] . (R p_i[a]) = sum_jk R[k][j] C[j][k]: the diagonal, then each off-diagonal couple
    double cross = rm_add(rm_add(rm_mul(R[0][0], C[0][0]), rm_mul(R[1][1], C[1][1])), rm_mul(R[2][2], C[2][2]));
    cross = rm_add(cross, rm_add(rm_mul(R[1][0], C[0][1]), rm_mul(R[0][1], C[1][0])));
    cross = rm_add(cross, rm_add(rm_mul(R[2][0], C[0][2]), rm_mul(R[0][2], C[2][0])));
    cross = rm_add(cross, rm_add(rm_mul(R[2][1], C[1][2]), rm_mul(R[1][2], C[2][1])));
    const double r2 = (ai + aj) - 2.0 * cross;
    return sqrt((r2 > 0.0 ? r2 : 0.0) / (double)n_rms);
}

// the atom (p of pose i, q of pose j) into the pair's sums
DEV void rm_atom(double (&acc)[3][3], const double* p, const double* q) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[j][k] = RM_FMA(p[j], q[k], acc[j][k]);
}
DEV void rm_atom_diff(double& dd, const double* p, const double* q) {
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    dd += dx * dx + dy * dy + dz * dz;
}

DEV void rm_write(const RmsdArgs& a, int i, int j, double v) {
    if (i >= a.n_a || j >= a.n_b) return;
    if (!a.same) { a.d[(int64_t)i * a.n_b + j] = v; return; }
    if (i == j) a.d[(int64_t)i * a.n_b + j] = 0.0;
    else if (i < j) { a.d[(int64_t)i * a.n_b + j] = v; a.d[(int64_t)j * a.n_b + i] = v; }
}

// ---- pairs ----------------------------------------------------------------------------------------------------------
#ifndef DRGNN_EMU
// `n` atoms at record offset `ob` of the tile's poses through LDS, into the lane's sums
DEV void rm_pass(const RmsdArgs& a, int i0, int j0, int64_t ob, int n, bool diff, double (&acc)[3][3], double& dd, RmsdPairShared& s) {
    const int y = (int)threadIdx.x / RM_TILE, x = (int)threadIdx.x % RM_TILE;
    const int64_t L = rm_record(a);
    for (int k0 = 0; k0 < n; k0 += RM_K) {
        const int nk = imin(RM_K, n - k0);
        FOR_TID(e, 2 * RM_TILE * 3 * RM_K) {                           // consecutive lanes: consecutive doubles of one pose
            const int side = e / (RM_TILE * 3 * RM_K), row = (e / (3 * RM_K)) % RM_TILE, k = e % (3 * RM_K);
            const int pose = (side ? j0 : i0) + row;
            double v = 0.0;
            if (k < 3 * nk && pose < (side ? a.n_b : a.n_a)) v = (side ? a.rec_b : a.rec_a)[(int64_t)pose * L + ob + 3 * (int64_t)k0 + k];
            if (side) s.b[row][k] = v; else s.a[row][k] = v;
        }
        BARRIER();
        if (diff) for (int k = 0; k < nk; ++k) rm_atom_diff(dd, &s.a[y][3 * k], &s.b[x][3 * k]);
        else for (int k = 0; k < nk; ++k) rm_atom(acc, &s.a[y][3 * k], &s.b[x][3 * k]);
        BARRIER();
    }
}
#endif

// One workgroup: the pairs (RM_TILE * ti + y, RM_TILE * tj + x)
DEV void rm_pairs(const RmsdArgs& a, int ti, int tj, RmsdPairShared& s) {
    if (a.same && ti > tj) return;                                     // (the whole workgroup)
    const int i0 = ti * RM_TILE, j0 = tj * RM_TILE, nF = a.n_fit, nR = a.n_rms;
    const int64_t L = rm_record(a);
#ifdef DRGNN_EMU
    (void)s;
    for (int i = i0; i < imin(i0 + RM_TILE, a.n_a); ++i)
        for (int j = j0; j < imin(j0 + RM_TILE, a.n_b); ++j) {
            const double* ri = a.rec_a + i * L;
            const double* rj = a.rec_b + j * L;
            double S[3][3] = {{0.0}}, C[3][3] = {{0.0}}, dd = 0.0;
            if (nF == 0) {
                for (int k = 0; k < nR; ++k) rm_atom_diff(dd, ri + 3 * k, rj + 3 * k);
                rm_write(a, i, j, sqrt(dd / (double)nR));
            } else {
                for (int k = 0; k < nF; ++k) rm_atom(S, ri + 3 * k, rj + 3 * k);
                for (int k = 0; k < nR; ++k) rm_atom(C, ri + 3 * (int64_t)(nF + k), rj + 3 * (int64_t)(nF + k));
                rm_write(a, i, j, rm_distance(S, C, ri[L - 1], rj[L - 1], nR));
            }
        }
#else
    const int i = i0 + (int)threadIdx.x / RM_TILE, j = j0 + (int)threadIdx.x % RM_TILE;
    double S[3][3], C[3][3], dd = 0.0;
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) { S[u][v] = 0.0; C[u][v] = 0.0; }
    if (nF == 0) {
        rm_pass(a, i0, j0, 0, nR, true, C, dd, s);
        rm_write(a, i, j, sqrt(dd / (double)nR));
    } else {
        rm_pass(a, i0, j0, 0, nF, false, S, dd, s);
        rm_pass(a, i0, j0, 3 * (int64_t)nF, nR, false, C, dd, s);
        const double ai = i < a.n_a ? a.rec_a[(int64_t)i * L + L - 1] : 0.0, aj = j < a.n_b ? a.rec_b[(int64_t)j * L + L - 1] : 0.0;
        rm_write(a, i, j, rm_distance(S, C, ai, aj, nR));
    }
#endif
}

// ---- neighbour relation ---------------------------------------------------------------------------------------------
// bits of pose pair (i, j): 1 j is a neighbour of i, 2 i is a neighbour of j (the rule pc_relation asks)
DEV int related(const DistRule& a, int i, int j) {
    if (i == j) return 0;
    return (a.d[(int64_t)i * a.n + j] <= a.cutoff ? 1 : 0) | (a.d[(int64_t)j * a.n + i] <= a.cutoff ? 2 : 0);
}
