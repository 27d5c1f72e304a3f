// drgnn_capi_metrics.hip -- the entry point of metrics.py: the evaluation scores of a prediction vector on the device, with the
// __global__ wrappers it launches.  One of the drgnn_capi*.hip units (drgnn_capi.hip says how they are built and what an entry
// point looks like).
#include "drgnn_capi_common.h"
#include "drgnn_metrics.h"

#ifndef DRGNN_EMU
// evaluation scores (drgnn_metrics.h)
__global__ void __launch_bounds__(MT_NT) k_mt_reduce(MetricsArgs a, int centred) {
    __shared__ MtRedShared s;
    mt_reduce_block(a, blockIdx.x, centred, s);
}
__global__ void __launch_bounds__(MT_NT) k_mt_combine(MetricsArgs a, int centred) { mt_combine_block(a, centred); }
__global__ void __launch_bounds__(MT_NT) k_mt_keys(MetricsArgs a, int absres) { mt_keys_block(a, blockIdx.x, absres); }
__global__ void __launch_bounds__(MT_NT) k_mt_hist(MetricsArgs a, int pass) {
    __shared__ MtHistShared s;
    mt_hist_block(a, blockIdx.x, pass, s);
}
__global__ void __launch_bounds__(MT_SNT) k_mt_scan(MetricsArgs a) {
    __shared__ MtScanShared s;
    mt_exscan_block<int32_t>(a.hist, (int64_t)MT_RADIX * a.n_tiles, s);
}
__global__ void __launch_bounds__(MT_NT) k_mt_scatter(MetricsArgs a, int pass) {
    __shared__ MtScatterShared s;
    mt_scatter_block(a, blockIdx.x, pass, s);
}
__global__ void __launch_bounds__(64) k_mt_median(MetricsArgs a) {
    if (threadIdx.x == 0) mt_median(a);
}
__global__ void __launch_bounds__(MT_NT) k_mt_hit(MetricsArgs a, int write) {
    __shared__ MtHitShared s;
    mt_hit_block(a, blockIdx.x, write, s);
}
__global__ void __launch_bounds__(MT_SNT) k_mt_hit_scan(MetricsArgs a) {
    __shared__ MtScanShared s;
    mt_hit_scan_block(a, s);
}
#endif  // !DRGNN_EMU

extern "C" {

// ---- evaluation scores (drgnn_metrics.h) ---------------------------------------------------------
int64_t drgnn_metrics_workspace_bytes(int64_t n) {
    if (n < 0 || n > INT32_MAX) return -1;
    int64_t off[9];
    mt_layout(n, off);
    return off[8];
}

// stable ascending LSD sort of a.keys[0] (payload a.vals[0] when set): MT_PASSES digits, the result back in buffer 0
static int mt_sort(MetricsArgs& a, void* stream) {
    DRGNN_EMU_ONLY(std::unique_ptr<MtHistShared> hs(new MtHistShared); std::unique_ptr<MtScanShared> ss(new MtScanShared);
                   std::unique_ptr<MtScatterShared> xs(new MtScatterShared);)
    const Grid tiles = grid1(a.n_tiles, MT_NT);
    for (int pass = 0; pass < MT_PASSES; ++pass) {
        DRGNN_LAUNCH(k_mt_hist, tiles, stream, mt_hist_block(a, (int)bx, pass, *hs), a, pass);
        DRGNN_LAUNCH(k_mt_scan, grid1(1, MT_SNT), stream, mt_exscan_block<int32_t>(a.hist, (int64_t)MT_RADIX * a.n_tiles, *ss), a);
        DRGNN_LAUNCH(k_mt_scatter, tiles, stream, mt_scatter_block(a, (int)bx, pass, *xs), a, pass);
    }
    return 0;
}

int drgnn_metrics(const double* pred, const double* y, int64_t n, int32_t what, int32_t direction, double threshold,
                  int32_t label_lo, int32_t n_labels, void* workspace, int64_t workspace_bytes, int64_t* counts,
                  double* scores, int32_t* order, int64_t* hits, void* stream) {
    if (n < 1 || n > INT32_MAX || !pred || !y || !workspace || !counts || !scores) return DRGNN_E_ARG;
    if ((what & ~(DRGNN_METRICS_COUNTS | DRGNN_METRICS_REGRESSION | DRGNN_METRICS_RANKING)) != 0) return DRGNN_E_ARG;
    if ((direction != 1 && direction != -1) || n_labels < 0 || n_labels > MT_KMAX) return DRGNN_E_ARG;
    if ((what & DRGNN_METRICS_RANKING) && (!order || !hits)) return DRGNN_E_ARG;
    if (workspace_bytes < drgnn_metrics_workspace_bytes(n)) return DRGNN_E_CAPACITY;
    if (n_labels > 0 && (label_lo < -(1 << 20) || label_lo > (1 << 20))) return DRGNN_E_ARG;
    int64_t off[9];
    mt_layout(n, off);
    char* ws = (char*)workspace;
    MetricsArgs a;
    a.pred = pred; a.y = y; a.n = n; a.thr = threshold; a.dir = direction; a.lo = label_lo; a.K = n_labels;
    a.G = (int)((n + 8 * MT_NT - 1) / (8 * MT_NT));
    if (a.G > MT_RED_WGS) a.G = MT_RED_WGS;
    a.n_tiles = (int)mt_tiles(n);
    a.keys[0] = (unsigned long long*)(ws + off[0]); a.keys[1] = (unsigned long long*)(ws + off[1]);
    a.vals[0] = order; a.vals[1] = (int32_t*)(ws + off[2]);
    a.hist = (int32_t*)(ws + off[3]);
    a.fpart = (double*)(ws + off[4]); a.ipart = (long long*)(ws + off[5]);
    a.tsum = (long long*)(ws + off[6]); a.ssum = (long long*)(ws + off[7]);
    a.counts = (long long*)counts; a.scores = scores; a.hits = (long long*)hits;
    MetricsArgs r = a;                  // the |r| sort: keys only
    r.vals[0] = r.vals[1] = nullptr;
    DRGNN_EMU_ONLY(std::unique_ptr<MtRedShared> rs(new MtRedShared); std::unique_ptr<MtScanShared> ss(new MtScanShared);
                   std::unique_ptr<MtHitShared> hs(new MtHitShared);)
    const Grid parts = grid1(a.G, MT_NT), tiles = grid1(a.n_tiles, MT_NT), one = grid1(1, MT_NT);
    int rc;
    if (what & (DRGNN_METRICS_COUNTS | DRGNN_METRICS_REGRESSION)) {
        DRGNN_LAUNCH(k_mt_reduce, parts, stream, mt_reduce_block(a, (int)bx, 0, *rs), a, 0);
        DRGNN_LAUNCH(k_mt_combine, one, stream, mt_combine_block(a, 0), a, 0);
    }
    if (what & DRGNN_METRICS_REGRESSION) {
        DRGNN_LAUNCH(k_mt_reduce, parts, stream, mt_reduce_block(a, (int)bx, 1, *rs), a, 1);
        DRGNN_LAUNCH(k_mt_combine, one, stream, mt_combine_block(a, 1), a, 1);
        DRGNN_LAUNCH(k_mt_keys, tiles, stream, mt_keys_block(r, (int)bx, 1), r, 1);
        if ((rc = mt_sort(r, stream))) return rc;
        DRGNN_LAUNCH(k_mt_median, grid1(1, 64), stream, mt_median(r), r);
    }
    if (what & DRGNN_METRICS_RANKING) {
        DRGNN_LAUNCH(k_mt_keys, tiles, stream, mt_keys_block(a, (int)bx, 0), a, 0);
        if ((rc = mt_sort(a, stream))) return rc;
        DRGNN_LAUNCH(k_mt_hit, tiles, stream, mt_hit_block(a, (int)bx, 0, *hs), a, 0);
        DRGNN_LAUNCH(k_mt_hit_scan, grid1(1, MT_SNT), stream, mt_hit_scan_block(a, *ss), a);
        DRGNN_LAUNCH(k_mt_hit, tiles, stream, mt_hit_block(a, (int)bx, 1, *hs), a, 1);
    }
    return 0;
}

}  // extern "C"
