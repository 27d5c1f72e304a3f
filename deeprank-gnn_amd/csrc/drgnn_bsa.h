// drgnn_bsa.h -- buried surface area of residues: the reference's `bsa` node feature (tools/BSA.py through freesasa's
// Lee-Richards method) for chosen residues of a ragged batch of two-chain complexes.
//
//     bsa(residue) = SASA_unbound(residue) - SASA_complex(residue),   SASA = sum over the residue's atoms of their area
// An atom takes part in a state when its radius there is > 0 (rad_c: both chains together; rad_u: each chain alone);
// the expanded radius is R = r + probe.  Area of atom i among the atoms of a state: delta = 2 R_i / n_slices, slice k at
// z = z_i - R_i + delta (k + 1/2) cuts the circle r_i' = sqrt(R_i^2 - (z - z_i)^2) out of atom i; every other atom j with
// |z - z_j| < R_j cuts r_j' = sqrt(R_j^2 - (z - z_j)^2) at the in-plane distance d:
//     d >= r_i' + r_j'   no effect;      d + r_i' <= r_j'   the slice is buried (contributes 0);
//     d + r_j' <= r_i'   no effect;      otherwise j buries the arc [beta - alpha, beta + alpha], beta = atan2(dy, dx),
//                                        alpha = acos((r_i'^2 + d^2 - r_j'^2) / (2 r_i' d))
// and the slice contributes R_i delta (2 pi - measure of the union of the arcs).
//
// One workgroup per target residue, one launch per call.  Phases:
//   0 box         one lane: the bounding box of the residue's atoms and their largest radius
//   1 candidates  all lanes over the atoms of the complex: those within (largest R_i + R_j) of the box go to an LDS list
//                 (at most BS_CCAP) with their two expanded radii (the unbound one 0 for the other chain's atoms)
//   then, for every atom of the residue and each of the two states it takes part in, the whole workgroup:
//   2 neighbours  lanes over the candidates: d^2 < (R_i + R_j)^2 (with a relative margin of 1e-5) -> LDS list (at most
//                 BS_NCAP = 256 neighbours of one atom)
//   3 arcs        BS_SCH slices at a time, work items (slice, neighbour): the rule above; an arc goes to the slice's list
//   4 union       work items (slice, arc a): the end of a opens a gap of the union unless it lies inside another arc
//                 (an end that coincides with another arc's end: the arc of the higher atom index keeps it); the gap
//                 reaches to the nearest following arc start.  No sort.  A slice without arcs exposes 2 pi.
//   5 sum         one lane: area = R_i delta * (sum of the gaps); the residue's SASA of the state += area
// The lists are filled through integer LDS atomics, so their order varies from run to run.  Nothing depends on it: a
// gap is a minimum and a coverage test over the SET of arcs (ties broken by atom index), and the gaps are summed as
// 2^-40 rad fixed-point integers (exact, order-free integer adds).  The per-residue sums run over the atoms in their
// order on one lane.  So a residue's bits do not depend on the batch, the chunk, the target list or the run.  No
// floating-point atomics.  Arc arithmetic is fp32 (the slice rule is continuous in the coordinates), except for nearly
// tangent circles (bs_exact_pair); areas and sums fp64.
// A list that overflows sets bit 0 of *status, and the residue's three outputs become NaN: never a wrong area.
// Host emulation (DRGNN_EMU): the work items of a phase run one after another.
#pragma once
#include "drgnn_rt.h"

#define BS_CCAP 1024                 // candidate atoms of one residue (within ~2 R of its bounding box; 1ATN: at most 377)
#define BS_NCAP 256                  // neighbours of one atom, and arcs of one slice
#define BS_SCH 10                    // slices per pass of phases 3 - 4
#define BS_MAX_SLICES 4096           // (the fixed-point sum of an atom's gaps stays far below 2^63)
#define BS_MAX_TARGETS 4194303       // workgroups of one launch: 2^32 / 1024 lanes - 1, the grid's limit in x
#define BS_FIX 1099511627776.0       // 2^40
#define BS_TWO_PI 6.2831853071795864769f

struct BsaArgs {
    const float* xyz;                // [T, 3]
    const int32_t* atom_ptr;         // [R + 1]
    const int32_t* res_ptr;          // [M + 1]
    const int32_t* res_split;        // [M]
    const float* rad_c;              // [n_radii] radius in the complex, 0: absent; atom t reads entry t % n_radii
    const float* rad_u;              // [n_radii] radius in the unbound chain
    const int32_t* tgt_res;          // [K] residue (global index)
    const int32_t* tgt_cx;           // [K] its complex
    int n_radii, n_slices;
    float probe;
    double probe_d;                  // the same in fp64, for the pairs taken in fp64
    double* out;                     // [K, 3] sasa_unbound, sasa_complex, bsa
    int32_t* status;                 // [1] bit 0: a list overflowed
};

struct BsaShared {
    long long acc[BS_SCH];           // gaps of a slice column, 2^-40 rad
    double sasa[2];
    float cx[BS_CCAP], cy[BS_CCAP], cz[BS_CCAP], crc[BS_CCAP], cru[BS_CCAP];
    int cid[BS_CCAP];
    float nx[BS_NCAP], ny[BS_NCAP], nz[BS_NCAP], nr[BS_NCAP];
    int nid[BS_NCAP];
    float as[BS_SCH * BS_NCAP], ae[BS_SCH * BS_NCAP];
    int aid[BS_SCH * BS_NCAP];
    int cnt[BS_SCH], buried[BS_SCH];
    float box[8];                    // lo xyz, hi xyz, the largest expanded radius (-1: no atom takes part)
    int ncand, nnb;
};

// an angle in [-2 pi, 4 pi) brought to [0, 2 pi]
DEV float bs_wrap(float x) {
    if (x < 0.0f) x += BS_TWO_PI;
    else if (x >= BS_TWO_PI) x -= BS_TWO_PI;
    return x;
}
DEV long long bs_fix(float g) { return (long long)((double)g * BS_FIX); }

// Circles that nearly touch (from outside or from inside), and a neighbour whose sphere barely reaches the slice plane:
// alpha ~ sqrt(overlap), so the 1e-7 of fp32 in r_i', r_j' and d becomes 5e-4 rad, and an fp32 test of the rule may fall on
// the other side.  Those pairs (about one in 500) take the rule in fp64 from the atoms' coordinates and radii, as
// tests/bsa_ref.py states it.  Returns 0 no effect, 1 the slice is buried, 2 an arc of half-width *alpha.  An arc
// narrower than BS_MIN_ARC, or wider than 2 pi less that, is taken to its limit (no effect, buried): phase 4 works on
// arc ends rounded to fp32 and could not tell such an arc from its complement.
#define BS_NEAR_R2 1.0e-2f           // |r_j'^2| below this (A^2): r_j' < 0.1 A
#define BS_NEAR_D 1.0e-3f            // |d - (r_i' + r_j')| or |d - |r_i' - r_j'|| below this (A)
#define BS_MIN_ARC 2.0e-6f           // rad
DEV int bs_exact_pair(const BsaArgs& a, int t, int j, int st, int k, float* alpha) {
    const float* rad = st == 0 ? a.rad_u : a.rad_c;
    const double Ri = (double)rad[t % a.n_radii] + a.probe_d, Rj = (double)rad[j % a.n_radii] + a.probe_d;
    const float* pi = a.xyz + 3 * (int64_t)t;
    const float* pj = a.xyz + 3 * (int64_t)j;
    const double dx = (double)pj[0] - (double)pi[0], dy = (double)pj[1] - (double)pi[1], dz = (double)pj[2] - (double)pi[2];
    const double delta = 2.0 * Ri / (double)a.n_slices;
    const double zo = -Ri + delta * ((double)k + 0.5);
    const double ri2 = Ri * Ri - zo * zo, h = zo - dz;
    if (!(fabs(h) < Rj) || !(ri2 > 0.0)) return 0;
    const double rj2 = Rj * Rj - h * h, ri = sqrt(ri2), rj = sqrt(rj2);
    const double dp2 = dx * dx + dy * dy, dp = sqrt(dp2);
    if (dp >= ri + rj) return 0;
    if (dp + ri <= rj) return 1;
    if (dp + rj <= ri) return 0;
    // alpha by the half angle, tan^2(alpha / 2) = (1 - cos) / (1 + cos) with both sides factored: the small factor is a
    // difference of fp64 values, so rounding the two products to fp32 keeps alpha's relative accuracy (no fp64 acos)
    const double num = (rj - ri + dp) * (rj + ri - dp), den = (ri + dp - rj) * (ri + dp + rj);
    const float al = 2.0f * atan2f(sqrtf((float)num), sqrtf((float)den));
    if (al < BS_MIN_ARC) return 0;
    if (al > 3.14159265358979f - BS_MIN_ARC) return 1;
    *alpha = al;
    return 2;
}

// One workgroup: target k.  s: the workgroup's LDS
// (no contraction into fused multiply-adds, as in if_d2: r_i'^2 = R_i^2 - h^2 and r_j'^2 = R_j^2 - h^2 round alike, so
// the <= tests of the rule see equal circles as equal, on the device as in the emulation)
DEV void bsa_residue(const BsaArgs& a, int64_t k, BsaShared& s) {
#ifndef DRGNN_EMU
#pragma clang fp contract(off)
#endif
    const int r = a.tgt_res[k], c = a.tgt_cx[k];
    const int sp = a.res_split[c];
    const int A0 = a.atom_ptr[a.res_ptr[c]], A1 = a.atom_ptr[a.res_ptr[c + 1]], As = a.atom_ptr[sp];
    const int t0 = a.atom_ptr[r], t1 = a.atom_ptr[r + 1];
    const int u0 = r < sp ? A0 : As, u1 = r < sp ? As : A1;          // the atoms of the residue's own chain
    const float probe = a.probe;
    const int S = a.n_slices;
    // ---- 0 box
    FOR_TID(i, 1) {
        float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, rmax = -1.0f;
        for (int t = t0; t < t1; ++t) {
            const float rc = a.rad_c[t % a.n_radii], ru = a.rad_u[t % a.n_radii];
            const float rm = rc > ru ? rc : ru;
            if (rm > 0.0f) {
                rmax = rm + probe > rmax ? rm + probe : rmax;
                for (int j = 0; j < 3; ++j) {
                    const float v = a.xyz[3 * (int64_t)t + j];
                    lo[j] = v < lo[j] ? v : lo[j];
                    hi[j] = v > hi[j] ? v : hi[j];
                }
            }
        }
        for (int j = 0; j < 3; ++j) { s.box[j] = lo[j]; s.box[3 + j] = hi[j]; }
        s.box[6] = rmax;
        s.ncand = 0; s.nnb = 0;
        s.sasa[0] = 0.0; s.sasa[1] = 0.0;
    }
    FOR_TID(i, BS_SCH) { s.acc[i] = 0; s.cnt[i] = 0; s.buried[i] = 0; }
    BARRIER();
    // ---- 1 candidates
    {
        const float rmax = s.box[6];
        FOR_TID(jj, rmax > 0.0f ? A1 - A0 : 0) {
            const int j = A0 + jj;
            const float rc = a.rad_c[j % a.n_radii], ru = (j >= u0 && j < u1) ? a.rad_u[j % a.n_radii] : 0.0f;
            const float rm = rc > ru ? rc : ru;
            if (rm > 0.0f) {
                const float e = (rmax + rm + probe) * 1.0001f + 1.0e-3f;
                const float x = a.xyz[3 * (int64_t)j], y = a.xyz[3 * (int64_t)j + 1], z = a.xyz[3 * (int64_t)j + 2];
                if (x >= s.box[0] - e && x <= s.box[3] + e && y >= s.box[1] - e && y <= s.box[4] + e &&
                    z >= s.box[2] - e && z <= s.box[5] + e) {
                    const int slot = ATOMIC_ADD(&s.ncand, 1);
                    if (slot < BS_CCAP) {
                        s.cx[slot] = x; s.cy[slot] = y; s.cz[slot] = z;
                        s.crc[slot] = rc > 0.0f ? rc + probe : 0.0f;
                        s.cru[slot] = ru > 0.0f ? ru + probe : 0.0f;
                        s.cid[slot] = j;
                    }
                }
            }
        }
    }
    BARRIER();
    const int ncand = s.ncand;
    bool overflow = ncand > BS_CCAP;
    for (int t = t0; t < t1 && !overflow; ++t) {
        for (int st = 0; st < 2 && !overflow; ++st) {               // 0 unbound, 1 complex
            const float rr = (st == 0 ? a.rad_u : a.rad_c)[t % a.n_radii];
            if (!(rr > 0.0f)) continue;
            const float Ri = rr + probe;
            const float xi = a.xyz[3 * (int64_t)t], yi = a.xyz[3 * (int64_t)t + 1], zi = a.xyz[3 * (int64_t)t + 2];
            const float delta = 2.0f * Ri / (float)S;
            // ---- 2 neighbours
            FOR_TID(ci, ncand) {
                const float Rj = st == 0 ? s.cru[ci] : s.crc[ci];
                const int id = s.cid[ci];
                if (Rj > 0.0f && id != t) {
                    const float dx = s.cx[ci] - xi, dy = s.cy[ci] - yi, dz = s.cz[ci] - zi;
                    const float reach = Ri + Rj;
                    if (dx * dx + dy * dy + dz * dz < reach * reach * 1.00001f) {
                        const int slot = ATOMIC_ADD(&s.nnb, 1);
                        if (slot < BS_NCAP) { s.nx[slot] = dx; s.ny[slot] = dy; s.nz[slot] = dz; s.nr[slot] = Rj; s.nid[slot] = id; }
                    }
                }
            }
            BARRIER();
            const int n = s.nnb;
            if (n > BS_NCAP) { overflow = true; break; }
            const int nn = n > 0 ? n : 1;
            const FastDiv fd = fastdiv_make(nn);
            for (int k0 = 0; k0 < S; k0 += BS_SCH) {
                const int ns = imin(BS_SCH, S - k0);
                // ---- 3 arcs
                FOR_TID(it, ns * n) {
                    const int kk = fastdiv(fd, it), ai = fastmod(fd, it, kk);
                    const float zo = -Ri + delta * ((float)(k0 + kk) + 0.5f);
                    const float ri2 = Ri * Ri - zo * zo;
                    const float h = zo - s.nz[ai], Rj = s.nr[ai];
                    const float rj2 = Rj * Rj - h * h;
                    int kind = 0;                                          // 0 no effect, 1 the slice is buried, 2 an arc
                    float alpha = 0.0f;
                    if (ri2 > 0.0f) {
                        const float dx = s.nx[ai], dy = s.ny[ai];
                        bool close = fabsf(rj2) < BS_NEAR_R2;               // the neighbour's sphere barely reaches the plane
                        if (!close && rj2 > 0.0f) {
                            const float ri = sqrtf(ri2), rj = sqrtf(rj2);
                            const float dp2 = dx * dx + dy * dy, dp = sqrtf(dp2);
                            close = fabsf(dp - (ri + rj)) < BS_NEAR_D || fabsf(dp - fabsf(ri - rj)) < BS_NEAR_D;
                            if (!close && dp < ri + rj) {
                                if (dp + ri <= rj) kind = 1;
                                else if (!(dp + rj <= ri)) {
                                    kind = 2;                              // (|cos| < 1 by a margin: BS_NEAR_D)
                                    alpha = acosf((ri2 + dp2 - rj2) / (2.0f * ri * dp));
                                }
                            }
                        }
                        if (close) kind = bs_exact_pair(a, t, s.nid[ai], st, k0 + kk, &alpha);
                        if (kind == 1) {
                            ATOMIC_OR(&s.buried[kk], 1);
                        } else if (kind == 2) {
                            const float beta = atan2f(dy, dx);
                            const int slot = ATOMIC_ADD(&s.cnt[kk], 1);              // (< BS_NCAP: one per neighbour at most)
                            s.as[kk * BS_NCAP + slot] = bs_wrap(beta - alpha);      // both ends in [0, 2 pi]:
                            s.ae[kk * BS_NCAP + slot] = bs_wrap(beta + alpha);      // their differences in [-2 pi, 2 pi]
                            s.aid[kk * BS_NCAP + slot] = s.nid[ai];
                        }
                    }
                }
                BARRIER();
                // ---- 4 union
                FOR_TID(it, ns * nn) {
                    const int kk = fastdiv(fd, it), sl = fastmod(fd, it, kk);
                    const int m = s.cnt[kk];
                    const float zo = -Ri + delta * ((float)(k0 + kk) + 0.5f);
                    if (!s.buried[kk] && Ri * Ri - zo * zo > 0.0f) {
                        if (m == 0) {
                            if (sl == 0) ATOMIC_ADD64(&s.acc[kk], bs_fix(BS_TWO_PI));
                        } else if (sl < m) {
                            const float* as = s.as + kk * BS_NCAP;
                            const float* ae = s.ae + kk * BS_NCAP;
                            const int* aid = s.aid + kk * BS_NCAP;
                            const float ea = ae[sl];
                            const int ida = aid[sl];
                            bool covered = false;
                            float gap = BS_TWO_PI;
                            for (int b = 0; b < m && !covered; ++b) {
                                const float sb = as[b];
                                if (b != sl) {
                                    const float tt = bs_wrap(ea - sb), len = bs_wrap(ae[b] - sb);
                                    covered = tt < len || (tt == len && aid[b] > ida);
                                }
                                const float g = bs_wrap(sb - ea);          // (b == sl: 2 pi - the arc's own length)
                                gap = g < gap ? g : gap;
                            }
                            if (!covered) ATOMIC_ADD64(&s.acc[kk], bs_fix(gap));
                        }
                    }
                }
                BARRIER();
                FOR_TID(i, BS_SCH) { s.cnt[i] = 0; s.buried[i] = 0; }
                BARRIER();
            }
            // ---- 5 sum
            FOR_TID(i, 1) {
                long long tot = 0;
                for (int j = 0; j < BS_SCH; ++j) { tot += s.acc[j]; s.acc[j] = 0; }
                s.sasa[st] += (double)Ri * (double)delta * ((double)tot / BS_FIX);
                s.nnb = 0;
            }
            BARRIER();
        }
    }
    FOR_TID(i, 1) {
        if (overflow) {
            const double nan = __builtin_nan("");
            a.out[3 * k] = nan; a.out[3 * k + 1] = nan; a.out[3 * k + 2] = nan;
            ATOMIC_OR(a.status, 1);
        } else {
            a.out[3 * k] = s.sasa[0]; a.out[3 * k + 1] = s.sasa[1]; a.out[3 * k + 2] = s.sasa[0] - s.sasa[1];
        }
    }
}
