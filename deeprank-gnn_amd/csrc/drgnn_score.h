// drgnn_score.h -- docking scores of M poses of one topology against a reference structure: the targets the reference
// writes in Graph.get_score (Graph.py:27-59): irmsd, lrmsd, fnat, dockQ, bin_class, capri_class.
//
// The topology work is done once per complex on the host (deeprank_gnn_amd.interface.ScoreReference): which decoy atoms
// correspond to which reference atoms, the three atom zones and the reference's residue pairs.  The kernel reduces
// those fixed correspondences over the M coordinate sets, one workgroup per pose, one launch per call:
//     zones        atom lists zone_atom[zone_ptr[z] .. zone_ptr[z + 1]) into the pose, with the matched reference
//                  coordinates zone_ref: z = 0 the interface zone, 1 the long chain, 2 the short chain (backbone atoms)
//     irmsd        the RMSD of zone 0 after the optimal proper rotation + translation of the decoy onto the reference
//     lrmsd        the RMSD of zone 2 under the optimal transform of zone 1
//     fnat         n_preserved / n_ref_pairs: a reference residue pair (pair_res) is preserved when an atom pair of the
//                  decoy's two residues lies at d^2 <= fnat_cutoff^2, d^2 from fp32 differences (if_d2)
//     dockQ        (fnat + 1 / (1 + (irmsd / 1.5)^2) + 1 / (1 + (lrmsd / 8.5)^2)) / 3
//     binclass     irmsd < 4.0;  capri_class 5, 4, 3, 2, 1 as irmsd falls below 6.0, 4.0, 2.0, 1.0
//
// Phases of a workgroup:
//   1 fnat      work items stride over (pair, atom of a) in chunks of SC_PCHUNK pairs; each walks the atoms of b; an
//               integer flag per pair in LDS (OR), then an integer count (ADD): order-free
//   2 moments   one pass over the gathered atoms of the three zones at once.  Slot s of zone z takes the atoms
//               s, s + SC_SLOTS, .. of the zone in that order and keeps 17 fp64 sums: sum p [3], sum q [3], sum |p|^2,
//               sum |q|^2, sum p q^T [9] (p the decoy f32 -> f64, q the reference); n is the zone's length
//   3 tree      the slots of every sum are added pairwise, slot j += slot j + h for h = SC_SLOTS / 2 .. 1
//   4 fit       lanes 0 and 1: zones 0 and 1.  The centred covariance and E0 = sum |p'|^2 + sum |q'|^2 come from the
//               moments; the optimal proper rotation is the eigenvector of the largest eigenvalue of Horn's symmetric
//               4 x 4 matrix (cyclic Jacobi, fp64, unrolled over registers: no run-time index into a local array);
//               residual = max(0, E0 - 2 lambda)
//   5 scores    one lane: irmsd; the rotation matrix of zone 1's quaternion applied to zone 2's moments taken about
//               zone 1's two centroids: sum |p''|^2 + sum |q''|^2 - 2 sum_ij R_ij C_ji; dockQ; the classes
// The slot an atom falls into, the order within a slot and the tree depend on the zone tables only, so a pose's result
// does not depend on M, on its place in the batch or on the run.  No floating-point atomics.
// Uncentred fp64 moments: coordinates ~1e2, sums ~1e7, eps 1e-16: the cancellation error is ~1e-9 A^2 per atom.
// Host emulation (DRGNN_EMU): the work items of a phase run one after another.
#pragma once
#include "drgnn_rt.h"
#include "drgnn_iface.h"

#define SC_LOG_SLOTS 7
#define SC_SLOTS (1 << SC_LOG_SLOTS)  // accumulation slots per zone
#define SC_NSUM 17                   // fp64 sums per slot
#define SC_PCHUNK 1024               // reference pairs flagged at a time
#define SC_MOM_WORDS (3 * SC_NSUM * SC_SLOTS)                     // doubles
#define SC_LDS_DOUBLES (SC_MOM_WORDS + 16)                        // + fit[2][8]: lambda, E0, n, -, quaternion
#define SC_LDS_BYTES (SC_LDS_DOUBLES * 8 + (SC_PCHUNK + 4) * 4)

struct ScoreArgs {
    const float* xyz;                // [M, T, 3]
    const int32_t* zone_atom;        // [Z]
    const double* zone_ref;          // [Z, 3]
    const int32_t* pair_res;         // [P, 2]
    const int32_t* atom_ptr;         // [R + 1]
    int zp[4];                       // zone_ptr
    int n_atoms, n_pairs, n_ref_pairs, amax;     // amax: the most atoms of a pair's first residue
    float cut2;                      // fnat_cutoff^2
    double* scores;                  // [M, 4] irmsd, lrmsd, fnat, dockQ
    int32_t* classes;                // [M, 2] binclass, capri_class
    int32_t* n_preserved;            // [M]
};

// One Jacobi rotation of the symmetric 4 x 4 matrix a (both triangles kept) in the (P, Q) plane, accumulated into the
// eigenvector matrix v.  P, Q and every loop bound are compile-time constants.
template <int P, int Q> DEV void sc_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != P && k != Q) {
            const double akp = a[k][P], akq = a[k][Q];
            const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
            a[k][P] = np_; a[P][k] = np_;
            a[k][Q] = nq_; a[Q][k] = nq_;
        }
    }
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = 0.0; a[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
}

// the largest eigenvalue of the symmetric a and its unit eigenvector q
DEV double sc_largest_eigenpair(double (&a)[4][4], double (&q)[4]) {
    double v[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] + a[1][2] * a[1][2] +
                           a[1][3] * a[1][3] + a[2][3] * a[2][3];
        const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2] + a[3][3] * a[3][3];
        if (off <= 1e-34 * dia) break;
        sc_rotate<0, 1>(a, v); sc_rotate<0, 2>(a, v); sc_rotate<0, 3>(a, v);
        sc_rotate<1, 2>(a, v); sc_rotate<1, 3>(a, v); sc_rotate<2, 3>(a, v);
    }
    double best = a[0][0];
    q[0] = v[0][0]; q[1] = v[1][0]; q[2] = v[2][0]; q[3] = v[3][0];
#define SC_TAKE(K) if (a[K][K] > best) { best = a[K][K]; q[0] = v[0][K]; q[1] = v[1][K]; q[2] = v[2][K]; q[3] = v[3][K]; }
    SC_TAKE(1) SC_TAKE(2) SC_TAKE(3)
#undef SC_TAKE
    const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (nrm > 0.0) { q[0] /= nrm; q[1] /= nrm; q[2] /= nrm; q[3] /= nrm; }
    else { q[0] = 1.0; q[1] = 0.0; q[2] = 0.0; q[3] = 0.0; }
    return best;
}

// the reduced sum k of zone z (slot 0 after the tree)
#define SC_MOM(mom, z, k) ((mom)[((z) * SC_NSUM + (k)) * SC_SLOTS])

// phase 4: fit of zone z from its moments -> out[0] = lambda, out[1] = E0, out[2] = n, out[4..8) = quaternion (w, x, y, z)
DEV void sc_fit(const double* mom, int z, int n_atoms, double* out) {
    const double n = (double)n_atoms;
    double sp[3], sq[3], S[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { sp[j] = SC_MOM(mom, z, j); sq[j] = SC_MOM(mom, z, 3 + j); }
    const double pp = SC_MOM(mom, z, 6), qq = SC_MOM(mom, z, 7);
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) S[j][k] = SC_MOM(mom, z, 8 + 3 * j + k) - sp[j] * sq[k] / n;
    const double e0 = (pp - (sp[0] * sp[0] + sp[1] * sp[1] + sp[2] * sp[2]) / n) +
                      (qq - (sq[0] * sq[0] + sq[1] * sq[1] + sq[2] * sq[2]) / n);
    double a[4][4];
    a[0][0] = S[0][0] + S[1][1] + S[2][2];
    a[1][1] = S[0][0] - S[1][1] - S[2][2];
    a[2][2] = -S[0][0] + S[1][1] - S[2][2];
    a[3][3] = -S[0][0] - S[1][1] + S[2][2];
    a[0][1] = a[1][0] = S[1][2] - S[2][1];
    a[0][2] = a[2][0] = S[2][0] - S[0][2];
    a[0][3] = a[3][0] = S[0][1] - S[1][0];
    a[1][2] = a[2][1] = S[0][1] + S[1][0];
    a[1][3] = a[3][1] = S[2][0] + S[0][2];
    a[2][3] = a[3][2] = S[1][2] + S[2][1];
    double q[4];
    const double lam = sc_largest_eigenpair(a, q);
    out[0] = lam; out[1] = e0; out[2] = n; out[3] = 0.0;
    out[4] = q[0]; out[5] = q[1]; out[6] = q[2]; out[7] = q[3];
}

// phase 5
DEV void sc_finish(const ScoreArgs& a, int64_t m, const double* mom, const double* fit, int preserved) {
    const double r0 = fit[1] - 2.0 * fit[0];
    const double irmsd = sqrt((r0 > 0.0 ? r0 : 0.0) / fit[2]);
    // zone 2 under zone 1's transform: p'' = p - mean p of zone 1, q'' = q - mean q of zone 1
    const double* f1 = fit + 8;
    const double nl = f1[2], ns = (double)(a.zp[3] - a.zp[2]);
    double ca[3], cb[3], sp[3], sq[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ca[j] = SC_MOM(mom, 1, j) / nl; cb[j] = SC_MOM(mom, 1, 3 + j) / nl;
        sp[j] = SC_MOM(mom, 2, j); sq[j] = SC_MOM(mom, 2, 3 + j);
    }
    const double pp = SC_MOM(mom, 2, 6) - 2.0 * (ca[0] * sp[0] + ca[1] * sp[1] + ca[2] * sp[2]) +
                      ns * (ca[0] * ca[0] + ca[1] * ca[1] + ca[2] * ca[2]);
    const double qq = SC_MOM(mom, 2, 7) - 2.0 * (cb[0] * sq[0] + cb[1] * sq[1] + cb[2] * sq[2]) +
                      ns * (cb[0] * cb[0] + cb[1] * cb[1] + cb[2] * cb[2]);
    const double w = f1[4], x = f1[5], y = f1[6], z = f1[7];
    double R[3][3];
    R[0][0] = w * w + x * x - y * y - z * z; R[0][1] = 2.0 * (x * y - w * z); R[0][2] = 2.0 * (x * z + w * y);
    R[1][0] = 2.0 * (x * y + w * z); R[1][1] = w * w - x * x + y * y - z * z; R[1][2] = 2.0 * (y * z - w * x);
    R[2][0] = 2.0 * (x * z - w * y); R[2][1] = 2.0 * (y * z + w * x); R[2][2] = w * w - x * x - y * y + z * z;
    double cross = 0.0;                                   // sum_i q''_i . (R p''_i) = sum_jk R[k][j] C[j][k]
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double c = SC_MOM(mom, 2, 8 + 3 * j + k) - ca[j] * sq[k] - sp[j] * cb[k] + ns * ca[j] * cb[k];
            cross += R[k][j] * c;
        }
    const double r2 = pp + qq - 2.0 * cross;
    const double lrmsd = sqrt((r2 > 0.0 ? r2 : 0.0) / ns);
    const double fnat = (double)preserved / (double)a.n_ref_pairs;
    const double ti = irmsd / 1.5, tl = lrmsd / 8.5;
    const double dockq = (fnat + 1.0 / (1.0 + ti * ti) + 1.0 / (1.0 + tl * tl)) / 3.0;
    a.scores[4 * m] = irmsd; a.scores[4 * m + 1] = lrmsd; a.scores[4 * m + 2] = fnat; a.scores[4 * m + 3] = dockq;
    int capri = 5;
    if (irmsd < 6.0) capri = 4;
    if (irmsd < 4.0) capri = 3;
    if (irmsd < 2.0) capri = 2;
    if (irmsd < 1.0) capri = 1;
    a.classes[2 * m] = irmsd < 4.0 ? 1 : 0;
    a.classes[2 * m + 1] = capri;
    a.n_preserved[m] = preserved;
}

// One workgroup: pose m.  lds: SC_LDS_BYTES, 8-byte aligned
DEV void score_pose(const ScoreArgs& a, int64_t m, double* lds) {
    double* mom = lds;
    double* fit = lds + SC_MOM_WORDS;
    int* flag = (int*)(lds + SC_LDS_DOUBLES);
    int* count = flag + SC_PCHUNK;
    const float* X = a.xyz + m * (int64_t)a.n_atoms * 3;
    // ---- 1 fnat
    FOR_TID(i, 1) { count[0] = 0; }
    const FastDiv fd = fastdiv_make(a.amax);
    for (int p0 = 0; p0 < a.n_pairs; p0 += SC_PCHUNK) {
        const int np = imin(SC_PCHUNK, a.n_pairs - p0);
        FOR_TID(i, np) { flag[i] = 0; }
        BARRIER();
        FOR_TID(it, np * a.amax) {
            const int pl = fastdiv(fd, it), ia = fastmod(fd, it, pl);
            const int ra = a.pair_res[2 * (p0 + pl)], rb = a.pair_res[2 * (p0 + pl) + 1];
            const int a0 = a.atom_ptr[ra], na = a.atom_ptr[ra + 1] - a0;
            if (ia < na) {
                const float* pa = X + 3 * (int64_t)(a0 + ia);
                const float ax = pa[0], ay = pa[1], az = pa[2];
                const int b0 = a.atom_ptr[rb], b1 = a.atom_ptr[rb + 1];
                bool hit = false;
                for (int b = b0; b < b1 && !hit; ++b) {
                    const float* pb = X + 3 * (int64_t)b;
                    hit = if_d2(ax, ay, az, pb[0], pb[1], pb[2]) <= a.cut2;
                }
                if (hit) ATOMIC_OR(&flag[pl], 1);
            }
        }
        BARRIER();
        FOR_TID(i, np) { if (flag[i]) ATOMIC_ADD(count, 1); }
        BARRIER();
    }
    // ---- 2 moments
    FOR_TID(t, 3 * SC_SLOTS) {
        const int z = t / SC_SLOTS, s = t % SC_SLOTS;
        double acc[SC_NSUM];
#pragma unroll
        for (int k = 0; k < SC_NSUM; ++k) acc[k] = 0.0;
        for (int i = a.zp[z] + s; i < a.zp[z + 1]; i += SC_SLOTS) {
            const float* pf = X + 3 * (int64_t)a.zone_atom[i];
            const double* qr = a.zone_ref + 3 * (int64_t)i;
            const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
            const double q[3] = {qr[0], qr[1], qr[2]};
#pragma unroll
            for (int j = 0; j < 3; ++j) { acc[j] += p[j]; acc[3 + j] += q[j]; }
            acc[6] += p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
            acc[7] += q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) acc[8 + 3 * j + k] += p[j] * q[k];
        }
#pragma unroll
        for (int k = 0; k < SC_NSUM; ++k) mom[(z * SC_NSUM + k) * SC_SLOTS + s] = acc[k];
    }
    BARRIER();
    // ---- 3 tree
    for (int h = SC_SLOTS / 2, sh = SC_LOG_SLOTS - 1; h >= 1; h >>= 1, --sh) {
        FOR_TID(i, 3 * SC_NSUM * h) {
            const int k = i >> sh, j = i & (h - 1);
            mom[k * SC_SLOTS + j] += mom[k * SC_SLOTS + j + h];
        }
        BARRIER();
    }
    // ---- 4 fit
    FOR_TID(z, 2) { sc_fit(mom, z, a.zp[z + 1] - a.zp[z], fit + 8 * z); }
    BARRIER();
    // ---- 5 scores
    FOR_TID(i, 1) { sc_finish(a, m, mom, fit, count[0]); }
}
