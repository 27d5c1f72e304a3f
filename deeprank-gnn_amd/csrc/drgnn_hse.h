// drgnn_hse.h -- half-sphere exposure of residues: the reference's `hse` node feature (Biopython's HSExposureCA with
// radius 12 A and offset 0, recorded as up, down, angle) for chosen residues of a ragged batch of complexes, and
// HSExposureCB (direction 1).  tests/hse_ref.py states the rule in numpy float64.
//
// The per-residue table bb i32 [n_rows, 5] holds the offsets of N, CA, C, CB inside the residue (-1: absent) and flags
// (HS_STD a standard amino acid, HS_GLY, HS_START the first residue of its chain); residue r reads row r % n_rows.
//   links     r, r+1 are linked iff both are standard and have a CA, r+1 does not start a chain, atom con_a of r and
//             atom con_b of r+1 exist and lie closer than the cutoff
//   members   the residues with a link on at least one side; only members are counted
//   value     direction 0: r is linked on both sides; b = unit(unit(c2 - c1) + unit(c2 - c3)) over the CAs of r-1, r, r+1
//             (the zero sum stays zero).  direction 1: r is a member with a CB (b = CB - CA) or a GLY with N and C
//             (b = Rot(-120 degrees, axis C - CA)(N - CA))
//   counts    every member o outside the stretch of r's peptide within `offset` positions of r, d = CA(o) - CA(r),
//             |d|^2 < radius^2: up when d.b > 0, else down (d.b = 0, d = 0, b = 0 and NaN: down)
//   angle     direction 0: acos(clip(u.b / (|u||b|), -1, 1)), u = CB - CA, or the rotated N of a GLY, else 0; direction 1: 0
//
// One workgroup per tile of targets of ONE complex, one launch per call.  Phases:
//   0 stage     lanes over the residues of the complex: the CA into LDS, the link to the next residue
//   1 members   lanes over the residues: linked on either side
//   2 targets   one wave per target, lanes across the residues of the complex, 64 at a time; the counts are the
//               popcounts of the wave's ballots (integers: no order, no floating-point atomics)
// Every decision (link, radius, side) and the angle are fp64 on the fp32 coordinates, IEEE sqrt and division, no
// contraction into fused multiply-adds: a difference of two fp32 numbers is exact in fp64, so the kernel and hse_ref part
// only on ties within rounding.  A target's bits depend on its complex alone: not on the batch, the tile, the target
// list, the place of the complex or the run.
// A complex of more than HS_RCAP residues sets bit 0 of *status and its targets become NaN rows: never a wrong count.
// Host emulation (DRGNN_EMU): a "wave" is one lane that walks all residues.
#pragma once
#include "drgnn_rt.h"

#define HS_RCAP 4096                 // residues of one complex (their CAs sit in LDS)
#define HS_MAX_TILES 4194303         // workgroups of one launch: 2^32 / 1024 lanes - 1, the grid's limit in x
#define HS_STD 1
#define HS_GLY 2
#define HS_START 4

struct HseArgs {
    const float* xyz;                // [T, 3]
    const int32_t* atom_ptr;         // [R + 1]
    const int32_t* res_ptr;          // [M + 1]
    const int32_t* bb;               // [n_rows, 5]
    const int32_t* tgt_res;          // [K] residue (global index)
    const int32_t* tgt_cx;           // [K] its complex
    const int32_t* tile_ptr;         // [n_tiles + 1] targets of a tile: all of one complex
    int n_rows, offset, con_a, con_b, direction;
    double radius2, cut2;
    double* out;                     // [K, 3] up, down, angle
    int32_t* status;                 // [1] bit 0: a complex beyond HS_RCAP residues
};

struct HseShared {
    float x[HS_RCAP], y[HS_RCAP], z[HS_RCAP];     // the CA of every residue of the complex (0 where there is none)
    unsigned char link[HS_RCAP];                  // linked to the next residue
    unsigned char member[HS_RCAP];                // linked on either side
};

// (HS_NOFMA opens every function that computes: the pragma does not reach into the functions a body calls)
#ifdef DRGNN_EMU
#define HS_LANES 1
#define HS_COUNT(p) ((p) ? 1 : 0)
#define HS_NOFMA
#else
#define HS_LANES DRGNN_WAVE
#define HS_COUNT(p) __popcll(__ballot(p))
#define HS_NOFMA _Pragma("clang fp contract(off)")
#endif

struct HsVec { double x, y, z; };
DEV HsVec hs_atom(const HseArgs& a, int t) {
    const float* p = a.xyz + 3 * (int64_t)t;
    return HsVec{(double)p[0], (double)p[1], (double)p[2]};
}
DEV HsVec hs_sub(HsVec a, HsVec b) { return HsVec{a.x - b.x, a.y - b.y, a.z - b.z}; }
DEV double hs_dot(HsVec a, HsVec b) { HS_NOFMA return a.x * b.x + a.y * b.y + a.z * b.z; }
DEV HsVec hs_unit(HsVec v) {
    HS_NOFMA
    const double n = sqrt(hs_dot(v, v));
    return HsVec{v.x / n, v.y / n, v.z / n};
}
DEV double hs_angle(HsVec u, HsVec v) {
    HS_NOFMA
    double c = hs_dot(u, v) / (sqrt(hs_dot(u, u)) * sqrt(hs_dot(v, v)));
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);                       // (NaN stays NaN)
    return acos(c);
}
// Rot(-120 degrees, axis c - ca)(n - ca): v cos + (k x v) sin + k (k.v)(1 - cos)
DEV HsVec hs_rotated_n(HsVec n, HsVec ca, HsVec c) {
    HS_NOFMA
    const double co = -0.5, si = -0.8660254037844386;
    const HsVec k = hs_unit(hs_sub(c, ca)), v = hs_sub(n, ca);
    const HsVec kxv = HsVec{k.y * v.z - k.z * v.y, k.z * v.x - k.x * v.z, k.x * v.y - k.y * v.x};
    const double kv = hs_dot(k, v) * (1.0 - co);
    return HsVec{v.x * co + kxv.x * si + k.x * kv, v.y * co + kxv.y * si + k.y * kv, v.z * co + kxv.z * si + k.z * kv};
}

// target k of a complex whose residues [R0, R0 + n) are staged in s; `lane` of HS_LANES walks the residues
DEV void hse_target(const HseArgs& a, int64_t k, int R0, int n, const HseShared& s, int lane) {
    HS_NOFMA
    const double nan = __builtin_nan("");
    const int r = a.tgt_res[k], i = r - R0;
    const int32_t* row = a.bb + 5 * (int64_t)(r % a.n_rows);
    const int t0 = a.atom_ptr[r];
    const bool before = i > 0 && s.link[i - 1], after = s.link[i] != 0;
    const HsVec c2 = HsVec{(double)s.x[i], (double)s.y[i], (double)s.z[i]};
    bool side = false;                                               // the side-chain direction exists
    HsVec u = HsVec{0.0, 0.0, 0.0};
    if (before || after) {
        if (row[3] >= 0) {
            u = hs_sub(hs_atom(a, t0 + row[3]), c2);
            side = true;
        } else if ((row[4] & HS_GLY) && row[0] >= 0 && row[2] >= 0) {
            u = hs_rotated_n(hs_atom(a, t0 + row[0]), c2, hs_atom(a, t0 + row[2]));
            side = true;
        }
    }
    bool valued;
    HsVec b = u;
    double angle = 0.0;
    if (a.direction == 0) {
        valued = before && after;
        if (valued) {
            const HsVec c1 = HsVec{(double)s.x[i - 1], (double)s.y[i - 1], (double)s.z[i - 1]};
            const HsVec c3 = HsVec{(double)s.x[i + 1], (double)s.y[i + 1], (double)s.z[i + 1]};
            const HsVec u1 = hs_unit(hs_sub(c2, c1)), u3 = hs_unit(hs_sub(c2, c3));
            b = HsVec{u1.x + u3.x, u1.y + u3.y, u1.z + u3.z};
            if (b.x != 0.0 || b.y != 0.0 || b.z != 0.0) b = hs_unit(b);
            if (side) angle = hs_angle(u, b);
        }
    } else {
        valued = side;
    }
    if (!valued) {
        if (lane == 0) { a.out[3 * k] = nan; a.out[3 * k + 1] = nan; a.out[3 * k + 2] = nan; }
        return;
    }
    int lo = i, hi = i;                                              // the stretch of the peptide that is not counted
    while (i - lo < a.offset && lo > 0 && s.link[lo - 1]) --lo;
    while (hi - i < a.offset && s.link[hi]) ++hi;        // (the last residue of a complex has no link)
    int up = 0, down = 0;
    for (int o0 = 0; o0 < n; o0 += HS_LANES) {
        const int o = o0 + lane;
        bool inside = false, above = false;
        if (o < n && s.member[o] && (o < lo || o > hi)) {
            const HsVec d = HsVec{(double)s.x[o] - c2.x, (double)s.y[o] - c2.y, (double)s.z[o] - c2.z};
            inside = hs_dot(d, d) < a.radius2;
            above = hs_dot(d, b) > 0.0;
        }
        up += HS_COUNT(inside && above);
        down += HS_COUNT(inside && !above);
    }
    if (lane == 0) { a.out[3 * k] = (double)up; a.out[3 * k + 1] = (double)down; a.out[3 * k + 2] = angle; }
}

// One workgroup: the targets of tile `tile`.  s: the workgroup's LDS
DEV void hse_tile(const HseArgs& a, int tile, HseShared& s) {
    HS_NOFMA
    const int k0 = a.tile_ptr[tile], k1 = a.tile_ptr[tile + 1];
    if (k1 <= k0) return;
    const int c = a.tgt_cx[k0];
    const int R0 = a.res_ptr[c], n = a.res_ptr[c + 1] - R0;
    if (n > HS_RCAP) {
        const double nan = __builtin_nan("");
        FOR_TID(j, 3 * (k1 - k0)) a.out[3 * (int64_t)k0 + j] = nan;
        FOR_TID(j, 1) ATOMIC_OR(a.status, 1);
        return;
    }
    // ---- 0 stage
    FOR_TID(i, n) {
        const int r = R0 + i;
        const int32_t* row = a.bb + 5 * (int64_t)(r % a.n_rows);
        const int t0 = a.atom_ptr[r];
        const bool ok = (row[4] & HS_STD) && row[1] >= 0;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (row[1] >= 0) {
            const float* p = a.xyz + 3 * (int64_t)(t0 + row[1]);
            x = p[0]; y = p[1]; z = p[2];
        }
        s.x[i] = x; s.y[i] = y; s.z[i] = z;
        bool link = false;
        if (ok && i + 1 < n) {
            const int32_t* next = a.bb + 5 * (int64_t)((r + 1) % a.n_rows);
            if ((next[4] & HS_STD) && !(next[4] & HS_START) && next[1] >= 0 && row[a.con_a] >= 0 && next[a.con_b] >= 0) {
                const HsVec d = hs_sub(hs_atom(a, a.atom_ptr[r + 1] + next[a.con_b]), hs_atom(a, t0 + row[a.con_a]));
                link = hs_dot(d, d) < a.cut2;
            }
        }
        s.link[i] = link ? 1 : 0;
    }
    BARRIER();
    // ---- 1 members
    FOR_TID(i, n) s.member[i] = (s.link[i] || (i > 0 && s.link[i - 1])) ? 1 : 0;
    BARRIER();
    // ---- 2 targets
#ifdef DRGNN_EMU
    for (int k = k0; k < k1; ++k) hse_target(a, k, R0, n, s, 0);
#else
    const int wave = (int)threadIdx.x / DRGNN_WAVE, lane = (int)threadIdx.x % DRGNN_WAVE;
    for (int k = k0 + wave; k < k1; k += DRGNN_NWAVES) hse_target(a, k, R0, n, s, lane);
#endif
}
