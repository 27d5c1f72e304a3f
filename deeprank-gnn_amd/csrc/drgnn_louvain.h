// drgnn_louvain.h -- deterministic Louvain community detection of every graph of a batch (offline
// preprocessing, the reference's community_detection(..., method='louvain'), community_pooling.py:95-158, which
// runs python-louvain's best_partition on the unweighted internal-contact graph inside PreCluster, DataSet.py:45-88).
//
// The algorithm is python-louvain's generate_dendrogram / __one_level at resolution 1 with two deliberate
// differences: nodes are visited in id order instead of a random order, ties between candidate communities go to
// the smallest community id, and labels are numbered by first appearance instead of through a set.  Every weight
// is an integer, so all arithmetic is exact int64:
//     A[u][v] = 1 per distinct pair {u, v}, A[u][u] = 2 per self-loop; k_u = sum_v A[u][v]; 2m = sum_u k_u
//     N(P) = sum_c (2m A_c - K_c^2),  Q = N / (2m)^2
//     a move of node i from `own` to c scores s(c) = 2m k_{i,c} - K_{c\i} k_i; the best c != own (ties: smallest
//     id) is taken when s(c) > s(own); passes repeat until a pass moves nothing or its gain is below threshold
//     (double)dN < (1e-7 (double)2m) (double)2m; a level after the first is recorded only when its N exceeds the
//     previous recorded N by at least that threshold; recorded communities are renumbered by first appearance and
//     become the nodes of the induced graph of the next level.
// tests/louvain_ref.py is the plain-Python statement of the same algorithm; the tests hold this kernel to it bit
// for bit (labels, level / pass counts, modularity).
//
// One 64-lane workgroup (one wave) per graph.  Node moves are sequential by definition, so the lanes split the
// current node's neighbour list (k_{i,c} by LDS integer atomics: order-independent, hence deterministic; the move
// by a wave arg-max on (s, then the smallest c)) and the whole-graph phases.  The working set lives in an LDS carve
// sized from the batch's largest graph: an induced level never has more nodes or CSR entries than level 0.
//     red64[64] redc[64] misc[4] | rpA[N+1] rpB[N+1] comm[N] K[N+1] acc[N] map[N] | colA[S] wA[S] colB[S] wB[S]
// with S = 2 * max_edges.  A is the current weighted CSR (rows deduplicated, entries in no particular order: no
// result depends on it), B the staging area an edge list or an induced graph is scattered into before it is merged
// row by row into A.  `labels` (global) carries the composition of the recorded levels.
#pragma once
#include "drgnn_rt.h"
#include "../../include/drgnn.h"

#define LV_W 64

struct LouvainArgs {
    const int64_t* edge_index;   // [2, Etot] global node ids (one direction or both, any duplication)
    int64_t n_edges;
    const int32_t* node_ptr;     // [B+1]
    const int32_t* edge_ptr;     // [B+1]
    int n_graphs;
    int capN, capE;              // carve bounds: largest graph of the batch
    int64_t* labels;             // [Ntot] out: per-graph local labels
    int32_t* info;               // [B, 2] out: (recorded levels, total passes); (-1, -1): graph beyond capN / capE
    double* modularity;          // [B] out
};

HD int64_t louvain_lds_words(int capN, int capE) {
    const int64_t S = 2 * (int64_t)(capE > 0 ? capE : 1);
    return 2 * LV_W + LV_W + 4 + 6 * (int64_t)capN + 3 + 4 * S;
}

// lanes of the one wave: `l` is the lane; the emulation runs the 64 lanes of a phase one after another
#ifdef DRGNN_EMU
#define LV_LANES(l) for (int l = 0; l < LV_W; ++l)
DEV void lv_atomic_min(int* p, int v) { if (v < *p) *p = v; }
#else
#define LV_LANES(l) for (int l = (int)threadIdx.x, l##_once = 1; l##_once; l##_once = 0)
DEV void lv_atomic_min(int* p, int v) { atomicMin(p, v); }
#endif
// a strided item loop inside LV_LANES
#define LV_STRIDE(i, l, lo, hi) for (int i = (lo) + (l); i < (hi); i += LV_W)

// sum of red[0..64) (each lane's partial), the same value on every lane
DEV long long lv_sum64(const long long* red) {
#ifdef DRGNN_EMU
    long long s = 0;
    for (int l = 0; l < LV_W; ++l) s += red[l];
    return s;
#else
    long long s = red[threadIdx.x];
    for (int m = 1; m < LV_W; m <<= 1) s += __shfl_xor(s, m, LV_W);
    return s;
#endif
}

// the largest (rs[l], then the smallest rc[l]) over the 64 lanes, the same on every lane
DEV void lv_argmax(const long long* rs, const int* rc, long long* best_s, int* best_c) {
#ifdef DRGNN_EMU
    long long s = rs[0];
    int c = rc[0];
    for (int l = 1; l < LV_W; ++l)
        if (rs[l] > s || (rs[l] == s && rc[l] < c)) { s = rs[l]; c = rc[l]; }
#else
    long long s = rs[threadIdx.x];
    int c = rc[threadIdx.x];
    for (int m = 1; m < LV_W; m <<= 1) {
        const long long os = __shfl_xor(s, m, LV_W);
        const int oc = __shfl_xor(c, m, LV_W);
        if (os > s || (os == s && oc < c)) { s = os; c = oc; }
    }
#endif
    *best_s = s;
    *best_c = c;
}

// in-place exclusive scan of a[0..n), returns the total (every lane); ends with a barrier
DEV int lv_exscan(int* a, int n) {
#ifdef DRGNN_EMU
    int run = 0;
    for (int i = 0; i < n; ++i) { const int v = a[i]; a[i] = run; run += v; }
    return run;
#else
    const int l = threadIdx.x;
    const int chunk = (n + LV_W - 1) / LV_W;
    const int lo = imin(l * chunk, n), hi = imin(lo + chunk, n);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += a[i];
    const int inc = wave_incl_scan(s);
    const int total = __shfl(inc, LV_W - 1, LV_W);
    int run = inc - s;
    for (int i = lo; i < hi; ++i) { const int v = a[i]; a[i] = run; run += v; }
    __syncthreads();
    return total;
#endif
}

DEV bool lv_below(long long dN, long long two_m) {
    return (double)dN < (1e-7 * (double)two_m) * (double)two_m;
}

// N(P) of the current level: 2m * (weight inside communities) - sum_c K_c^2
DEV long long lv_quality(int n, long long two_m, const int* rp, const int* col, const int* w, const int* comm,
                         const int* K, long long* red) {
    LV_LANES(l) {
        long long part = 0;
        LV_STRIDE(u, l, 0, n) {
            const int cu = comm[u];
            long long in = 0;
            for (int e = rp[u]; e < rp[u + 1]; ++e) in += (comm[col[e]] == cu) ? w[e] : 0;
            part += two_m * in - (long long)K[u] * K[u];          // K[u]: community u (0 when empty)
        }
        red[l] = part;
    }
    BARRIER();
    const long long q = lv_sum64(red);
    BARRIER();
    return q;
}

// rows 0..nrows of the staging CSR (rpB, colB, wB) -> deduplicated rows of A.  sum: a repeated entry adds its
// weight (induced graphs); otherwise it is the same pair listed again and keeps its weight (level 0).  acc is all
// zero on entry and on exit.
DEV void lv_merge(int nrows, bool sum, const int* rpB, const int* colB, int* wB, int* rpA, int* colA, int* wA,
                  int* acc, int* slot) {
    int base = 0;
    for (int a = 0; a < nrows; ++a) {
        const int lo = rpB[a], hi = rpB[a + 1];
        LV_LANES(l) {
            LV_STRIDE(e, l, lo, hi) {
                const int w = wB[e];
                if (ATOMIC_ADD(&acc[colB[e]], w) == 0) wB[e] = -w;     // the first of its column in this row
            }
        }
        BARRIER();
        LV_LANES(l) {
            LV_STRIDE(e, l, lo, hi) {
                if (wB[e] < 0) {
                    const int b = colB[e], at = base + ATOMIC_ADD(slot, 1);
                    colA[at] = b;
                    wA[at] = sum ? acc[b] : -wB[e];
                }
            }
        }
        BARRIER();
        const int cnt = *slot;
        LV_LANES(l) {
            LV_STRIDE(e, l, lo, hi) { acc[colB[e]] = 0; }
            if (l == 0) { rpA[a] = base; *slot = 0; }
        }
        base += cnt;
        BARRIER();
    }
    LV_LANES(l) { if (l == 0) rpA[nrows] = base; }
    BARRIER();
}

DEV void louvain_graph(const LouvainArgs& a, int g, int* lds) {
    const int n0 = a.node_ptr[g], n_orig = a.node_ptr[g + 1] - n0;
    const int e0 = a.edge_ptr[g], E = a.edge_ptr[g + 1] - e0;
    int64_t* labels = a.labels + n0;
    if (n_orig > a.capN || E > a.capE || n_orig < 0 || E < 0) {       // the host sized the carve from other bounds
        LV_LANES(l) { if (l == 0) { a.info[2 * g] = -1; a.info[2 * g + 1] = -1; a.modularity[g] = 0.0; } }
        return;
    }
    const int capN = a.capN;
    const int S = 2 * (a.capE > 0 ? a.capE : 1);
    long long* red = (long long*)lds;                 // [64]
    int* redc = lds + 2 * LV_W;                        // [64]
    int* slot = redc + LV_W;                           // [4]
    int* rpA = slot + 4;                               // [capN + 1]
    int* rpB = rpA + capN + 1;                         // [capN + 1]
    int* comm = rpB + capN + 1;                        // [capN]
    int* K = comm + capN;                              // [capN + 1]  (also: placement cursors, first-member flags)
    int* acc = K + capN + 1;                           // [capN]      k_{i,c} / merge accumulator, zero between uses
    int* map = acc + capN;                             // [capN]
    int* colA = map + capN;
    int* wA = colA + S;
    int* colB = wA + S;
    int* wB = colB + S;
    const int64_t* src = a.edge_index + e0;
    const int64_t* dst = a.edge_index + a.n_edges + e0;

    // ---- level 0: the distinct pairs of the edge slice as a weighted CSR ----------------------------------
    LV_LANES(l) {
        LV_STRIDE(u, l, 0, n_orig + 1) { rpB[u] = 0; }
        LV_STRIDE(u, l, 0, n_orig) { acc[u] = 0; labels[u] = u; }
        if (l == 0) slot[0] = 0;
    }
    BARRIER();
    LV_LANES(l) {
        LV_STRIDE(e, l, 0, E) {
            const int64_t u = src[e] - n0, v = dst[e] - n0;
            if (u >= 0 && u < n_orig && v >= 0 && v < n_orig) {
                ATOMIC_ADD(&rpB[u], 1);
                if (u != v) ATOMIC_ADD(&rpB[v], 1);
            }
        }
    }
    BARRIER();
    lv_exscan(rpB, n_orig + 1);
    LV_LANES(l) { LV_STRIDE(u, l, 0, n_orig) { K[u] = rpB[u]; } }
    BARRIER();
    LV_LANES(l) {
        LV_STRIDE(e, l, 0, E) {
            const int64_t u = src[e] - n0, v = dst[e] - n0;
            if (u >= 0 && u < n_orig && v >= 0 && v < n_orig) {
                const int p = ATOMIC_ADD(&K[u], 1);
                colB[p] = (int)v;
                wB[p] = (u == v) ? 2 : 1;
                if (u != v) {
                    const int q = ATOMIC_ADD(&K[v], 1);
                    colB[q] = (int)u;
                    wB[q] = 1;
                }
            }
        }
    }
    BARRIER();
    lv_merge(n_orig, false, rpB, colB, wB, rpA, colA, wA, acc, slot);

    LV_LANES(l) {
        long long part = 0;
        LV_STRIDE(e, l, 0, rpA[n_orig]) { part += wA[e]; }
        red[l] = part;
    }
    BARRIER();
    const long long two_m = lv_sum64(red);
    BARRIER();
    if (two_m == 0) {                                  // no pairs: every node on its own, Q = 0
        LV_LANES(l) { if (l == 0) { a.info[2 * g] = 0; a.info[2 * g + 1] = 0; a.modularity[g] = 0.0; } }
        return;
    }

    int n = n_orig, levels = 0, passes = 0;
    long long n_rec = 0;
    for (;;) {
        // ---- one level: every node in its own community ------------------------------------------------
        LV_LANES(l) {
            LV_STRIDE(u, l, 0, n) {
                int k = 0;
                for (int e = rpA[u]; e < rpA[u + 1]; ++e) k += wA[e];
                comm[u] = u;
                K[u] = k;
            }
        }
        BARRIER();
        long long n_cur = lv_quality(n, two_m, rpA, colA, wA, comm, K, red);
        for (;;) {
            int moved = 0;
            for (int i = 0; i < n; ++i) {
                const int lo = rpA[i], hi = rpA[i + 1];
                LV_LANES(l) {                          // k_i and k_{i,c} of every neighbouring community
                    long long part = 0;
                    LV_STRIDE(e, l, lo, hi) {
                        const int j = colA[e], w = wA[e];
                        part += w;
                        if (j != i) ATOMIC_ADD(&acc[comm[j]], w);
                    }
                    red[l] = part;
                }
                BARRIER();
                const long long ki = lv_sum64(red);
                const int own = comm[i];
                const long long s_own = two_m * acc[own] - ((long long)K[own] - ki) * ki;
                LV_LANES(l) {                          // each lane's best other community
                    long long bs = LLONG_MIN;
                    int bc = INT_MAX;
                    LV_STRIDE(e, l, lo, hi) {
                        const int j = colA[e];
                        const int c = comm[j];
                        if (j == i || c == own) continue;
                        const long long s = two_m * acc[c] - (long long)K[c] * ki;
                        if (s > bs || (s == bs && c < bc)) { bs = s; bc = c; }
                    }
                    red[l] = bs;
                    redc[l] = bc;
                }
                BARRIER();
                long long best_s;
                int best_c;
                lv_argmax(red, redc, &best_s, &best_c);
                const int to = (best_c != INT_MAX && best_s > s_own) ? best_c : own;
                BARRIER();
                LV_LANES(l) {
                    LV_STRIDE(e, l, lo, hi) { if (colA[e] != i) acc[comm[colA[e]]] = 0; }
                    if (l == 0) { K[own] -= (int)ki; K[to] += (int)ki; comm[i] = to; }
                }
                moved += (to != own) ? 1 : 0;
                BARRIER();
            }
            ++passes;
            const long long n_new = lv_quality(n, two_m, rpA, colA, wA, comm, K, red);
            const long long gain = n_new - n_cur;
            n_cur = n_new;
            if (moved == 0 || lv_below(gain, two_m)) break;
        }
        if (levels > 0 && lv_below(n_cur - n_rec, two_m)) break;
        ++levels;
        n_rec = n_cur;

        // ---- record: renumber by first appearance, compose the labels, build the induced graph ---------------
        LV_LANES(l) { LV_STRIDE(c, l, 0, n) { map[c] = INT_MAX; } }
        BARRIER();
        LV_LANES(l) { LV_STRIDE(u, l, 0, n) { lv_atomic_min(&map[comm[u]], u); } }
        BARRIER();
        LV_LANES(l) {
            LV_STRIDE(u, l, 0, n) { K[u] = (map[comm[u]] == u) ? 1 : 0; }
            if (l == 0) K[n] = 0;
        }
        BARRIER();
        const int k = lv_exscan(K, n + 1);
        LV_LANES(l) { LV_STRIDE(u, l, 0, n) { if (K[u + 1] > K[u]) map[comm[u]] = K[u]; } }
        BARRIER();
        LV_LANES(l) {
            LV_STRIDE(v, l, 0, n_orig) { labels[v] = map[comm[labels[v]]]; }
            LV_STRIDE(c, l, 0, k + 1) { rpB[c] = 0; }
        }
        BARRIER();
        LV_LANES(l) { LV_STRIDE(u, l, 0, n) { ATOMIC_ADD(&rpB[map[comm[u]]], rpA[u + 1] - rpA[u]); } }
        BARRIER();
        lv_exscan(rpB, k + 1);
        LV_LANES(l) { LV_STRIDE(c, l, 0, k) { K[c] = rpB[c]; } }
        BARRIER();
        LV_LANES(l) {
            LV_STRIDE(u, l, 0, n) {
                const int cu = map[comm[u]];
                for (int e = rpA[u]; e < rpA[u + 1]; ++e) {
                    const int p = ATOMIC_ADD(&K[cu], 1);
                    colB[p] = map[comm[colA[e]]];
                    wB[p] = wA[e];
                }
            }
        }
        BARRIER();
        lv_merge(k, true, rpB, colB, wB, rpA, colA, wA, acc, slot);
        n = k;
    }
    LV_LANES(l) {
        if (l == 0) {
            a.info[2 * g] = levels;
            a.info[2 * g + 1] = passes;
            a.modularity[g] = (double)n_rec / ((double)two_m * (double)two_m);
        }
    }
}
