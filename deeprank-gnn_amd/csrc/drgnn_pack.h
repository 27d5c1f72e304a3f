// drgnn_pack.h -- the interface builder's output (drgnn_iface.h, with the optional drgnn_bsa.h / drgnn_hse.h / drgnn_depth.h rows) packed
// into the arrays a resident graph set holds (drgnn_collate.h), without leaving the device: what
// GraphDataSet.load_one_graph + ResidentGraphSet.__init__ assemble per graph on the host.
//
//   x          [N, F]     column f of node i comes from source cols[f][0], column cols[f][1] of it:
//                PK_TYPE   type_table[type[i]]          f32 [20, Wt]: every column that depends on the residue type alone
//                PK_POS    pos[i]                       f32 [N, 3]
//                PK_CHAIN  chain[i]                     i32 [N]
//                PK_BSA    bsa[i]                       f64 [N, 3], rounded once to f32
//                PK_HSE    hse[i]                       f64 [N, 3], rounded once; a row whose first entry is NaN reads 0, 0, 0
//                PK_RES    res_feat[node_residue[i] % n_rows]   f32 [n_rows, W]
//                PK_DEPTH  depth[i]                     f64 [N], rounded once to f32
//   edge_index_out [2, 2E]  graph k's columns 2 edge_ptr[k] .. 2 edge_ptr[k+1]: its pairs, then the same pairs reversed
//   edge_attr      [2E]     mode 0 the distance, mode 1 tanh(-d/2 + 2) + 1 in fp64 on the f32 distance, rounded once
//   iedge_index_out [2, 2Ei] the same layout, node ids + node_ptr[k] (batch-global: what precluster() reads)
//   batch          [N]      the complex of every node
//
// One workgroup of PK_NT lanes per complex, one launch.  cols and type_table are staged in LDS once per workgroup; the
// lanes then run flat over n_k * F, so consecutive lanes write consecutive floats.  Every output element has one writer:
// no atomics, nothing crosses workgroups, the bits depend on the complex alone.
// The offset tables come from device memory, so the kernel clips them to the counts the host sized the outputs by.
// Host emulation (DRGNN_EMU): the lanes run one after another.
#pragma once
#include "drgnn_rt.h"

#define PK_NT 256                    // lanes of a workgroup
#define PK_FCAP 256                  // output columns F (the staged descriptor)
#define PK_TCAP 64                   // columns Wt of the type table (the staged table: 20 rows)
#define PK_TYPES 20
#define PK_MAX_COMPLEXES 65535       // one workgroup each: the builder's own limit
#define PK_TYPE 0
#define PK_POS 1
#define PK_CHAIN 2
#define PK_BSA 3
#define PK_HSE 4
#define PK_RES 5
#define PK_DEPTH 6
#define PK_NSRC 7

struct PackArgs {
    const int32_t *node_ptr, *edge_ptr, *iedge_ptr;      // [M + 1]
    const int32_t *node_residue, *chain, *type;          // [N]
    const float* pos;                                    // [N, 3]
    const int64_t* edge_index;                           // [E, 2] local ids
    const float* dist;                                   // [E]
    const int64_t* iedge_index;                          // [Ei, 2] local ids
    const double *bsa, *hse;                             // [N, 3] or null
    const double* depth;                                 // [N] or null
    const float* res_feat;                               // [n_rows, W] or null
    const float* type_table;                             // [20, Wt] or null
    const int32_t* cols;                                 // [F, 2]
    int n_rows, W, Wt, F, edge_mode;
    int N, E, Ei;
    float* x;                                            // [N, F] or null
    int64_t* edge_index_out;                             // [2, 2E] or null
    float* edge_attr;                                    // [2E] or null
    int64_t* iedge_index_out;                            // [2, 2Ei] or null
    int64_t* batch;                                      // [N] or null
};

struct PackShared {
    int32_t cols[2 * PK_FCAP];
    float table[PK_TYPES * PK_TCAP];
};

#ifdef DRGNN_EMU
#define PK_FOR(i, n) for (int i = 0; i < (int)(n); ++i)
#else
#define PK_FOR(i, n) for (int i = (int)threadIdx.x; i < (int)(n); i += PK_NT)
#endif

// [lo, hi) of entry k of an offset table, clipped to [0, total]
DEV void pk_range(const int32_t* ptr, int k, int total, int& lo, int& hi) {
    lo = imax(0, imin(ptr[k], total));
    hi = imax(lo, imin(ptr[k + 1], total));
}

DEV float pk_value(const PackArgs& a, const PackShared& s, int src, int c, int64_t node) {
    switch (src) {
    case PK_TYPE: {
        const int t = a.type[node];
        return (unsigned)t < (unsigned)PK_TYPES ? s.table[t * a.Wt + c] : 0.0f;
    }
    case PK_POS: return a.pos[3 * node + c];
    case PK_CHAIN: return (float)a.chain[node];
    case PK_BSA: return (float)a.bsa[3 * node + c];
    case PK_DEPTH: return (float)a.depth[node];
    case PK_HSE: {
        const double head = a.hse[3 * node];
        return head != head ? 0.0f : (float)a.hse[3 * node + c];
    }
    default: {
        const int r = imax(a.node_residue[node], 0) % a.n_rows;
        return a.res_feat[(int64_t)r * a.W + c];
    }
    }
}

// One workgroup: complex k.  s: the workgroup's LDS
DEV void pack_block(const PackArgs& a, int k, PackShared& s) {
    int n0, n1, e0, e1, i0, i1;
    pk_range(a.node_ptr, k, a.N, n0, n1);
    pk_range(a.edge_ptr, k, a.E, e0, e1);
    pk_range(a.iedge_ptr, k, a.Ei, i0, i1);
    const int n = n1 - n0, ne = e1 - e0, ni = i1 - i0;
    if (a.x && n > 0) {
        PK_FOR(i, 2 * a.F) s.cols[i] = a.cols[i];
        if (a.type_table) { PK_FOR(i, PK_TYPES * a.Wt) s.table[i] = a.type_table[i]; }
        BARRIER();
        float* x = a.x + (int64_t)n0 * a.F;
#ifdef DRGNN_EMU
        PK_FOR(j, n * a.F) {
            const int i = j / a.F, f = j % a.F;
            x[j] = pk_value(a, s, s.cols[2 * f], s.cols[2 * f + 1], (int64_t)n0 + i);
        }
#else
        // (node, column) of a lane's element advance by a fixed step: two divisions per lane, none per element
        const int di = PK_NT / a.F, df = PK_NT % a.F;
        int i = (int)threadIdx.x / a.F, f = (int)threadIdx.x % a.F;
        for (int j = (int)threadIdx.x; j < n * a.F; j += PK_NT) {
            x[j] = pk_value(a, s, s.cols[2 * f], s.cols[2 * f + 1], (int64_t)n0 + i);
            i += di; f += df;
            if (f >= a.F) { f -= a.F; ++i; }
        }
#endif
    }
    if (a.batch) { PK_FOR(i, n) a.batch[n0 + i] = (int64_t)k; }
    if (a.edge_index_out || a.edge_attr) {
        const int64_t row = 2 * (int64_t)a.E, at = 2 * (int64_t)e0;
        PK_FOR(e, ne) {
            const int64_t u = a.edge_index[2 * ((int64_t)e0 + e)], v = a.edge_index[2 * ((int64_t)e0 + e) + 1];
            if (a.edge_index_out) {
                a.edge_index_out[at + e] = u;            a.edge_index_out[row + at + e] = v;
                a.edge_index_out[at + ne + e] = v;       a.edge_index_out[row + at + ne + e] = u;
            }
            if (a.edge_attr) {
                const float d = a.dist[e0 + e];
                const float w = a.edge_mode == 1 ? (float)(tanh(-(double)d / 2.0 + 2.0) + 1.0) : d;
                a.edge_attr[at + e] = w;
                a.edge_attr[at + ne + e] = w;
            }
        }
    }
    if (a.iedge_index_out) {
        const int64_t row = 2 * (int64_t)a.Ei, at = 2 * (int64_t)i0;
        PK_FOR(e, ni) {
            const int64_t u = a.iedge_index[2 * ((int64_t)i0 + e)] + n0, v = a.iedge_index[2 * ((int64_t)i0 + e) + 1] + n0;
            a.iedge_index_out[at + e] = u;               a.iedge_index_out[row + at + e] = v;
            a.iedge_index_out[at + ni + e] = v;          a.iedge_index_out[row + at + ni + e] = u;
        }
    }
}
