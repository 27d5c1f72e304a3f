// drgnn_iface.h -- residue-level interface graphs of a ragged batch of complexes, from atom coordinates: the
// geometric half of the reference's graph generation (ResidueGraph.get_graph, ResidueGraph.py:108-145, the contact
// search behind it, :272-316, and the minimum atom distance of an edge, :364-381).
//
// The rule, per complex with chains A and B, over every atom given:
//     interface pair   residues a in A, b in B with an atom pair at d^2 < contact_distance^2 (strict); its `dist` is
//                      the smallest atom-atom distance of the pair
//     node             a standard residue (res_type >= 0) in at least one interface pair whose partner is standard
//                      too: a pair with a non-standard residue is dropped as a whole
//     internal edge    two nodes i < j of one chain with an atom pair at d^2 < internal_contact_distance^2 (strict)
// Canonical order (the reference's is networkx insertion order): nodes by (chain, residue position), interface edges
// (A node, B node) sorted by that pair, internal edges (i < j) sorted by (i, j).  Node ids are local to the complex.
//
// d^2 is formed from coordinate differences in fp32 with every product and sum rounded on its own (no contraction
// into fused multiply-adds, in either build), so the device and the host emulation agree bit for bit; a minimum does
// not depend on the order of its operands, hence neither does any result on how lanes, waves and tiles split the work.
//
// Launches (count: 1 - 5, fill: 6):
//   1 sphere     one lane per residue: centroid (an fp64 sum in atom order, rounded once: it is also `pos`) and the
//                radius of the residue's atoms around it; clears the node flag
//   2 pairs      one workgroup per (complex, IF_AB residues of A); the B chain's atoms pass through LDS in tiles of
//                whole residues; one wave takes one A residue at a time: its lanes test the bounding spheres of 64 B
//                residues at once (|c_a - c_b| < cutoff + r_a + r_b, with a margin that covers the rounding of the
//                centroids), then take the atom pairs of each surviving residue pair; the minimum is a wave
//                reduction.  Result: the dense [maxA x maxB] min-d^2 matrix of the complex (+inf: no contact), the
//                row counts, the node flags (integer OR)
//   3 rows       (count mode) one wave per node: internal partners j > i of the same chain under the 3 A sphere
//                test, reduced the same way; per-row counts
//   4 scan       one workgroup per complex: exclusive scans of the node flags and of both row counts
//   5 offsets    one workgroup: exclusive scans across complexes -> node_ptr, edge_ptr, iedge_ptr
//   6 rows       (fill mode) node records, the compacted rows of the matrix, the internal edges recomputed by the
//                code of launch 3, each at its scanned offset
// Host emulation (DRGNN_EMU): the lanes of a wave and the waves of a workgroup run one after another.
#pragma once
#include "drgnn_rt.h"
#include "../../include/drgnn.h"

#define IF_NT 256                    // threads of a pairs / rows workgroup
#define IF_NW (IF_NT / DRGNN_WAVE)
#define IF_AB 16                     // residues per pairs / rows workgroup
#define IF_TILE_DEFAULT 4096         // B atoms staged at a time (48 KiB)
#define IF_INF __builtin_inff()

struct IfaceArgs {
    const float* xyz;                // [T, 3]
    const int32_t* atom_ptr;         // [R + 1]
    const int32_t* res_ptr;          // [M + 1]
    const int32_t* res_split;        // [M]
    const int32_t* res_type;         // [R]
    int n_complexes, n_residues, maxA, maxB, tile_atoms;
    float cut, cut2, icut, icut2;
    // workspace (iface_layout)
    float* D;                        // [M, maxA, maxB] min d^2 of the interface pairs
    float* sphere;                   // [R, 4] centroid, radius
    int* flag;                       // [R] node?
    int* nloc;                       // [R] node id within the complex
    int* eoff;                       // [R] interface edges of an A row: count, then offset within the complex
    int* ioff;                       // [R] internal edges (i, j > i) of a row: count, then offset
    int* cnt;                        // [M, 3] nodes, interface edges, internal edges of a complex
    int32_t* node_ptr;               // [M + 1] out
    int32_t* edge_ptr;
    int32_t* iedge_ptr;
    // fill
    int32_t* node_residue;
    float* pos;
    int32_t* chain;
    int32_t* type;
    int64_t* edge_index;
    float* dist;
    int64_t* iedge_index;
    float* idist;
    int64_t n_nodes, n_edges, n_iedges;          // capacities of the output arrays: nothing is written beyond
};

// byte offsets of D | sphere | flag | nloc | eoff | ioff | cnt | end
HD void iface_layout(int64_t M, int64_t maxA, int64_t maxB, int64_t R, int64_t off[8]) {
    int64_t at = 0;
    off[0] = at; at += ((M * maxA * maxB * 4 + 15) / 16) * 16;
    off[1] = at; at += R * 16;
    for (int k = 2; k < 6; ++k) { off[k] = at; at += ((R * 4 + 15) / 16) * 16; }
    off[6] = at; at += ((M * 12 + 15) / 16) * 16;
    off[7] = at;
}
HD int64_t iface_pairs_lds_bytes(int tile_atoms) { return 4 * (3 * (int64_t)tile_atoms + IF_AB); }

#ifdef DRGNN_EMU
#define IF_THREADS(t) for (int t = 0; t < IF_NT; ++t)
#define IF_WAVES(w) for (int w = 0; w < IF_NW; ++w)
#define IF_LANE0 (true)
#define IF_TID0 (true)
#else
#define IF_THREADS(t) for (int t = (int)threadIdx.x, t##_once = 1; t##_once; t##_once = 0)
#define IF_WAVES(w) for (int w = (int)(threadIdx.x >> 6), w##_once = 1; w##_once; w##_once = 0)
#define IF_LANE0 ((threadIdx.x & 63) == 0)
#define IF_TID0 (threadIdx.x == 0)
#endif
#define IF_SQRT(v) sqrtf(v)                  // correctly rounded in both builds (__fsqrt_rn is the native approximation)

// squared distance from differences; each product and sum rounds on its own: contraction into fused multiply-adds is
// switched off for this function in both builds, whatever the target and the flags of the build
#ifdef DRGNN_EMU
#if defined(__clang__)
#define IF_NO_CONTRACT
#else
#define IF_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#endif
static inline IF_NO_CONTRACT float if_d2(float ax, float ay, float az, float bx, float by, float bz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#else
DEV float if_d2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
#endif
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float s = xx + yy;
    return s + zz;
}

// can residues with these spheres have atoms closer than `cut`?  The margin (1e-4 relative, 0.01 A) is far above the
// rounding of centroids, radii and this test at PDB coordinate magnitudes (|x| < 10^4: one fp32 step is 1e-3), so
// the test never rejects a true contact.
DEV bool if_spheres_near(const float* sa, const float* sb, float cut) {
    const float thr = (cut + sa[3] + sb[3]) * 1.0001f + 0.01f;
    return if_d2(sa[0], sa[1], sa[2], sb[0], sb[1], sb[2]) < thr * thr;
}

// smallest d^2 over the atom pairs of A [na, 3] x B [nb, 3], the same value on every lane of the wave.  The lanes
// form a (64 / nbp) x nbp grid over (A atom, B atom), nbp = nb rounded up to a power of two (at most 64).
DEV float if_pair_min(const float* A, int na, const float* B, int nb) {
    float m = IF_INF;
#ifdef DRGNN_EMU
    for (int ia = 0; ia < na; ++ia)
        for (int ib = 0; ib < nb; ++ib) {
            const float d = if_d2(A[3 * ia], A[3 * ia + 1], A[3 * ia + 2], B[3 * ib], B[3 * ib + 1], B[3 * ib + 2]);
            m = d < m ? d : m;
        }
#else
    const int lane = threadIdx.x & 63;
    int sh = 0;
    while ((1 << sh) < nb && sh < 6) ++sh;
    const int nbp = 1 << sh, ib0 = lane & (nbp - 1), step = 64 >> sh;
    for (int ia = lane >> sh; ia < na; ia += step) {
        const float ax = A[3 * ia], ay = A[3 * ia + 1], az = A[3 * ia + 2];
        for (int ib = ib0; ib < nb; ib += nbp) {
            const float d = if_d2(ax, ay, az, B[3 * ib], B[3 * ib + 1], B[3 * ib + 2]);
            m = d < m ? d : m;
        }
    }
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) {
        const float o = __shfl_xor(m, x, 64);
        m = o < m ? o : m;
    }
#endif
    return m;
}

// One wave, residue i (atoms A [na, 3], sphere sa) against the n <= 64 residues j0 .. j0 + n - 1, whose atoms are at
// B + 3 * (atom_ptr[j] - bbase).  A partner takes part when ok[j] >= okmin and the spheres are near.  Lane l holds
// j0 + l: emit(j, v, rank) is called once per partner with v = the pair's min d^2 when below cut2, else +inf, and
// rank = the number of partners before j in this call with v < +inf.  Returns the number of those.
template <class Emit>
DEV int if_chunk(const IfaceArgs& a, const float* A, int na, const float* sa, int j0, int n, const float* B, int bbase,
                 const int* ok, int okmin, float cut, float cut2, Emit emit) {
#ifdef DRGNN_EMU
    int cnt = 0;
    for (int l = 0; l < n; ++l) {
        const int j = j0 + l;
        float v = IF_INF;
        if (ok[j] >= okmin && if_spheres_near(sa, a.sphere + 4 * j, cut)) {
            const int p = a.atom_ptr[j];
            const float m = if_pair_min(A, na, B + 3 * (int64_t)(p - bbase), a.atom_ptr[j + 1] - p);
            if (m < cut2) v = m;
        }
        emit(j, v, cnt);
        cnt += (v < IF_INF) ? 1 : 0;
    }
    return cnt;
#else
    const int lane = threadIdx.x & 63;
    const int j = j0 + lane;
    bool near = false;
    if (lane < n && ok[j] >= okmin) {
        const float4 sb = *(const float4*)(a.sphere + 4 * j);
        const float s[4] = {sb.x, sb.y, sb.z, sb.w};
        near = if_spheres_near(sa, s, cut);
    }
    unsigned long long todo = __ballot(near);
    float v = IF_INF;
    while (todo) {                                     // (wave-uniform)
        const int k = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const int p = a.atom_ptr[j0 + k];
        const float m = if_pair_min(A, na, B + 3 * (int64_t)(p - bbase), a.atom_ptr[j0 + k + 1] - p);
        if (lane == k && m < cut2) v = m;
    }
    const unsigned long long hit = __ballot(v < IF_INF);
    if (lane < n) emit(j, v, __popcll(hit & ((1ull << lane) - 1ull)));
    return __popcll(hit);
#endif
}

// launch 1
DEV void iface_sphere_item(const IfaceArgs& a, int r) {
    const int p0 = a.atom_ptr[r], p1 = a.atom_ptr[r + 1];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int p = p0; p < p1; ++p) { sx += a.xyz[3 * (int64_t)p]; sy += a.xyz[3 * (int64_t)p + 1]; sz += a.xyz[3 * (int64_t)p + 2]; }
    const double n = (double)(p1 - p0);
    const float cx = p1 > p0 ? (float)(sx / n) : 0.f, cy = p1 > p0 ? (float)(sy / n) : 0.f, cz = p1 > p0 ? (float)(sz / n) : 0.f;
    float m = 0.f;
    for (int p = p0; p < p1; ++p) {
        const float d = if_d2(a.xyz[3 * (int64_t)p], a.xyz[3 * (int64_t)p + 1], a.xyz[3 * (int64_t)p + 2], cx, cy, cz);
        m = d > m ? d : m;
    }
    float* s = a.sphere + 4 * (int64_t)r;
    s[0] = cx; s[1] = cy; s[2] = cz; s[3] = IF_SQRT(m);
    a.flag[r] = 0;
}

// launch 2: complex c, A residues [blk * IF_AB, +IF_AB).  lds: tile [3 * tile_atoms] | rowcnt [IF_AB]
DEV void iface_pairs_block(const IfaceArgs& a, int c, int blk, float* lds) {
    const int r0 = a.res_ptr[c], rs = a.res_split[c], r1 = a.res_ptr[c + 1];
    const int RA = rs - r0, RB = r1 - rs;
    const int a0 = blk * IF_AB;
    if (a0 >= RA) return;
    const int a1 = imin(a0 + IF_AB, RA);
    float* tile = lds;
    int* rowcnt = (int*)(lds + 3 * (int64_t)a.tile_atoms);
    float* Dc = a.D + (int64_t)c * a.maxA * a.maxB;
    IF_THREADS(t) { if (t < IF_AB) rowcnt[t] = 0; }
    int b0 = 0;
    while (b0 < RB) {
        // the tile: the longest run of whole residues from b0 within tile_atoms atoms (the host made sure that every
        // single residue fits)
        const int base = a.atom_ptr[rs + b0];
        int lo = b0 + 1, hi = RB;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.atom_ptr[rs + mid] - base <= a.tile_atoms) lo = mid; else hi = mid - 1;
        }
        const int b1 = lo;
        const int nat = imin(a.atom_ptr[rs + b1] - base, a.tile_atoms);
        BARRIER();                                    // (the readers of the tile before this one)
        IF_THREADS(t) { for (int i = t; i < 3 * nat; i += IF_NT) tile[i] = a.xyz[3 * (int64_t)base + i]; }
        BARRIER();
        IF_WAVES(w) {
            for (int ra = a0 + w; ra < a1; ra += IF_NW) {
                const int r = r0 + ra;
                if (a.res_type[r] < 0) {              // a non-standard residue has no pairs
                    for (int bb = b0; bb < b1; bb += DRGNN_WAVE) {
#ifdef DRGNN_EMU
                        for (int l = 0; l < imin(DRGNN_WAVE, b1 - bb); ++l) Dc[(int64_t)ra * a.maxB + bb + l] = IF_INF;
#else
                        const int b = bb + (int)(threadIdx.x & 63);
                        if (b < b1) Dc[(int64_t)ra * a.maxB + b] = IF_INF;
#endif
                    }
                    continue;
                }
                const int pa = a.atom_ptr[r], na = a.atom_ptr[r + 1] - pa;
                const float* sa = a.sphere + 4 * (int64_t)r;
                const float sav[4] = {sa[0], sa[1], sa[2], sa[3]};
                int cnt = 0;
                for (int bb = b0; bb < b1; bb += DRGNN_WAVE) {
                    cnt += if_chunk(a, a.xyz + 3 * (int64_t)pa, na, sav, rs + bb, imin(DRGNN_WAVE, b1 - bb), tile, base,
                                    a.res_type, 0, a.cut, a.cut2, [&](int j, float v, int rank) {
                                        Dc[(int64_t)ra * a.maxB + (j - rs)] = v;
                                        if (v < IF_INF) ATOMIC_OR(&a.flag[j], 1);
                                    });
                }
                if (IF_LANE0) rowcnt[ra - a0] += cnt;
            }
        }
        b0 = b1;
    }
    BARRIER();
    IF_THREADS(t) {
        if (t < a1 - a0) {
            const int n = rowcnt[t];
            a.eoff[r0 + a0 + t] = n;
            if (n > 0) a.flag[r0 + a0 + t] = 1;      // (A flags are written here only)
        }
    }
}

// launches 3 and 6: complex c, residues [blk * IF_AB, +IF_AB) of it, one wave per residue.
// count mode (write = false): ioff[r] = internal edges (r, j > r).  fill mode: the node record, the interface row, the
// internal row of every node.
DEV void iface_rows_block(const IfaceArgs& a, int c, int blk, bool write) {
    const int r0 = a.res_ptr[c], rs = a.res_split[c], r1 = a.res_ptr[c + 1];
    const int i0 = r0 + blk * IF_AB;
    if (i0 >= r1) return;
    const int i1 = imin(i0 + IF_AB, r1);
    const int RB = r1 - rs;
    const float* Dc = a.D + (int64_t)c * a.maxA * a.maxB;
    IF_WAVES(w) {
        for (int r = i0 + w; r < i1; r += IF_NW) {
            if (a.flag[r] == 0) {
                if (!write && IF_LANE0) a.ioff[r] = 0;
                continue;
            }
            const int me = a.nloc[r];                 // (count mode: not scanned yet, not used)
            if (write) {
                const int64_t n = (int64_t)a.node_ptr[c] + me;
                if (IF_LANE0 && n < a.n_nodes) {
                    a.node_residue[n] = r;
                    a.pos[3 * n] = a.sphere[4 * (int64_t)r];
                    a.pos[3 * n + 1] = a.sphere[4 * (int64_t)r + 1];
                    a.pos[3 * n + 2] = a.sphere[4 * (int64_t)r + 2];
                    a.chain[n] = r >= rs ? 1 : 0;
                    a.type[n] = a.res_type[r];
                }
                if (r < rs) {                         // the row of the matrix, compacted
                    const float* row = Dc + (int64_t)(r - r0) * a.maxB;
                    int64_t e = (int64_t)a.edge_ptr[c] + a.eoff[r];
                    for (int bb = 0; bb < RB; bb += DRGNN_WAVE) {
#ifdef DRGNN_EMU
                        for (int l = 0; l < imin(DRGNN_WAVE, RB - bb); ++l) {
                            const float v = row[bb + l];
                            if (v < IF_INF) {
                                if (e < a.n_edges) {
                                    a.edge_index[2 * e] = me;
                                    a.edge_index[2 * e + 1] = a.nloc[rs + bb + l];
                                    a.dist[e] = IF_SQRT(v);
                                }
                                ++e;
                            }
                        }
#else
                        const int lane = threadIdx.x & 63, b = bb + lane;
                        const float v = b < RB ? row[b] : IF_INF;
                        const unsigned long long hit = __ballot(v < IF_INF);
                        const int64_t at = e + __popcll(hit & ((1ull << lane) - 1ull));
                        if (v < IF_INF && at < a.n_edges) {
                            a.edge_index[2 * at] = me;
                            a.edge_index[2 * at + 1] = a.nloc[rs + b];
                            a.dist[at] = IF_SQRT(v);
                        }
                        e += __popcll(hit);
#endif
                    }
                }
            }
            // internal partners: the nodes after r in its chain
            const int jend = r < rs ? rs : r1;
            const int pa = a.atom_ptr[r], na = a.atom_ptr[r + 1] - pa;
            const float* sa = a.sphere + 4 * (int64_t)r;
            const float sav[4] = {sa[0], sa[1], sa[2], sa[3]};
            const int64_t e0 = write ? (int64_t)a.iedge_ptr[c] + a.ioff[r] : 0;
            int run = 0;
            for (int j0 = r + 1; j0 < jend; j0 += DRGNN_WAVE) {
                const int64_t first = e0 + run;
                const int got = if_chunk(a, a.xyz + 3 * (int64_t)pa, na, sav, j0, imin(DRGNN_WAVE, jend - j0), a.xyz, 0,
                                         a.flag, 1, a.icut, a.icut2, [&](int j, float v, int rank) {
                                             const int64_t at = first + rank;
                                             if (write && v < IF_INF && at < a.n_iedges) {
                                                 a.iedge_index[2 * at] = me;
                                                 a.iedge_index[2 * at + 1] = a.nloc[j];
                                                 a.idist[at] = IF_SQRT(v);
                                             }
                                         });
                run += got;
            }
            if (!write && IF_LANE0) a.ioff[r] = run;
        }
    }
}

// launch 4: one DRGNN_NTHREADS workgroup per complex.  part: DRGNN_NTHREADS + 1 ints
DEV void iface_scan_block(const IfaceArgs& a, int c, int* part) {
    const int r0 = a.res_ptr[c], rs = a.res_split[c], r1 = a.res_ptr[c + 1];
    FOR_TID(i, r1 - r0) { a.nloc[r0 + i] = a.flag[r0 + i]; }
    BARRIER();
    const int n = wg_exscan(a.nloc + r0, r1 - r0, part);
    const int e = wg_exscan(a.eoff + r0, rs - r0, part);
    const int ie = wg_exscan(a.ioff + r0, r1 - r0, part);
    if (IF_TID0) { a.cnt[3 * c] = n; a.cnt[3 * c + 1] = e; a.cnt[3 * c + 2] = ie; }
}

// launch 5: one DRGNN_NTHREADS workgroup
DEV void iface_offsets_block(const IfaceArgs& a, int* part) {
    const int M = a.n_complexes;
    FOR_TID(i, M + 1) {
        a.node_ptr[i] = i < M ? a.cnt[3 * i] : 0;
        a.edge_ptr[i] = i < M ? a.cnt[3 * i + 1] : 0;
        a.iedge_ptr[i] = i < M ? a.cnt[3 * i + 2] : 0;
    }
    BARRIER();
    wg_exscan(a.node_ptr, M + 1, part);
    wg_exscan(a.edge_ptr, M + 1, part);
    wg_exscan(a.iedge_ptr, M + 1, part);
}
