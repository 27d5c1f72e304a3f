// drgnn_capi_layers.hip -- the entry points of layers.py, community_pooling.py and clustering.py: the stand-alone conv layers,
// the pooling functions, graclus, Markov clustering and Louvain, with the __global__ wrappers they launch.  One of the
// drgnn_capi*.hip units (drgnn_capi.hip says how they are built and what an entry point looks like).
#include "drgnn_capi_common.h"
#include "drgnn_layers.h"
#include "drgnn_mcl.h"
#include "drgnn_louvain.h"

#ifndef DRGNN_EMU
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_conv_gemm(ConvLayerArgs a) { conv_gemm_block(a, blockIdx.x); }
__global__ void __launch_bounds__(256) k_conv_aggregate(ConvLayerArgs a) {
    conv_aggregate_item(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
__global__ void __launch_bounds__(256) k_conv_bwd_du(ConvLayerArgs a) {
    conv_bwd_du_item(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_conv_bwd_dw(ConvLayerArgs a) { conv_bwd_dw_block(a, blockIdx.x); }
__global__ void __launch_bounds__(256) k_conv_reduce(ConvReduceArgs a) {
    conv_reduce_item(a, blockIdx.x * blockDim.x + threadIdx.x);
}
__global__ void __launch_bounds__(256) k_conv_bwd_dx(ConvLayerArgs a) {
    conv_bwd_dx_item(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_segpool_fwd(SegPoolArgs a) { segpool_fwd_block(a, blockIdx.x); }
__global__ void __launch_bounds__(256) k_segmax_bwd(SegPoolArgs a, int64_t n_items, int64_t n_nodes) {
    segmax_bwd_item(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_items, n_nodes);
}
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_edge_export(EdgeExportArgs a) { edge_export_block(a, blockIdx.x); }
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_cluster_max(ClusterOffsetArgs a) {
    __shared__ long long mm[2];
    cluster_max_block(a, blockIdx.x, mm);
}
__global__ void k_cluster_scan(ClusterOffsetArgs a) { cluster_scan_single(a); }
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_cluster_add(ClusterOffsetArgs a) { cluster_add_block(a, blockIdx.x); }
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_mcl(MclArgs a) {
    __shared__ double red[DRGNN_NTHREADS];
    __shared__ int flag[2];
    mcl_graph(a, blockIdx.x, flag, red);
}
__global__ void __launch_bounds__(LV_W) k_louvain(LouvainArgs a) {
    extern __shared__ __attribute__((aligned(16))) int smem_lv[];
    louvain_graph(a, blockIdx.x, smem_lv);
}
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_graclus(GraclusArgs a) {
    extern __shared__ __attribute__((aligned(16))) int smem_g[];
    graclus_block(a, blockIdx.x, smem_g);
}
#endif  // !DRGNN_EMU

extern "C" {

// ---- stand-alone layers / pooling functions ---------------------------------------------------
static int conv_layer_fill(ConvLayerArgs& a, int32_t kind, const float* x, int64_t n_nodes, int32_t F,
                           int32_t H, const drgnn_conv_params* p, const int32_t* ws_i32,
                           const float* ws_f32, int64_t n_edges) {
    if (kind < DRGNN_GINET || kind > DRGNN_FOUT || !x || !p || !p->w_nbr || !ws_i32) return DRGNN_E_ARG;
    if (kind != DRGNN_GINET && (!p->w_self || !p->bias)) return DRGNN_E_ARG;
    if (kind == DRGNN_SGAT && !ws_f32) return DRGNN_E_ARG;
    if (F < 1 || H < 1 || H > DRGNN_LAYER_MAXH || n_nodes >= INT32_MAX) return DRGNN_E_WIDTH;
    TopoLayout lay;
    topo_layout(n_nodes, n_edges, 1, &lay);
    TopoView tv = topo_view(const_cast<int32_t*>(ws_i32), const_cast<float*>(ws_f32), lay);
    a.kind = kind; a.x = x; a.F = F; a.H = H; a.p = *p; a.N = (int)n_nodes;
    a.rowptr = tv.p[DRGNN_TI_ROWPTR0]; a.col = tv.p[DRGNN_TI_COL0]; a.w = tv.w0;
    a.colptr = tv.p[DRGNN_TI_COLPTR0]; a.ridx = tv.p[DRGNN_TI_ROWIDX0]; a.tslot = tv.p[DRGNN_TI_TSLOT0];
    a.u = nullptr; a.out = nullptr; a.grad_out = nullptr; a.partials = nullptr; a.grad_x = nullptr;
    return 0;
}

int64_t drgnn_conv_layer_slabs(int64_t n_nodes) { return (n_nodes + DRGNN_LAYER_ROWS - 1) / DRGNN_LAYER_ROWS; }
int64_t drgnn_conv_layer_partial_elems(int32_t kind, int32_t F, int32_t H) { return conv_partial_floats(kind, F, H); }

int drgnn_conv_layer_forward(int32_t kind, const float* x, int64_t n_nodes, int32_t F, int32_t H,
                             const drgnn_conv_params* p, const int32_t* ws_i32, const float* ws_f32,
                             int64_t n_edges, float* u, float* out, void* stream) {
    ConvLayerArgs a;
    int rc = conv_layer_fill(a, kind, x, n_nodes, F, H, p, ws_i32, ws_f32, n_edges);
    if (rc) return rc;
    if (!u || !out) return DRGNN_E_ARG;
    a.u = u; a.out = out;
    const int64_t slabs = drgnn_conv_layer_slabs(n_nodes);
    DRGNN_LAUNCH(k_conv_gemm, grid1(slabs), stream, conv_gemm_block(a, (int)bx), a);
    DRGNN_LAUNCH(k_conv_aggregate, grid_items(n_nodes * H), stream, conv_aggregate_item(a, bx), a);
    return 0;
}

int drgnn_conv_layer_backward(int32_t kind, const float* x, int64_t n_nodes, int32_t F, int32_t H,
                              const drgnn_conv_params* p, const int32_t* ws_i32, const float* ws_f32,
                              int64_t n_edges, const float* grad_out, float* du, float* partials,
                              const drgnn_conv_grads* g, float* grad_x, void* stream) {
    ConvLayerArgs a;
    int rc = conv_layer_fill(a, kind, x, n_nodes, F, H, p, ws_i32, ws_f32, n_edges);
    if (rc) return rc;
    if (!grad_out || !du || !partials || !g) return DRGNN_E_ARG;
    a.u = du; a.grad_out = grad_out; a.partials = partials; a.grad_x = grad_x;
    const int64_t slabs = drgnn_conv_layer_slabs(n_nodes);
    DRGNN_LAUNCH(k_conv_bwd_du, grid_items(n_nodes * H), stream, conv_bwd_du_item(a, bx), a);
    DRGNN_LAUNCH(k_conv_bwd_dw, grid1(slabs), stream, conv_bwd_dw_block(a, (int)bx), a);
    ConvReduceArgs r;
    r.partials = partials; r.n_wg = (int)slabs; r.kind = kind; r.F = F; r.H = H; r.lay = *p; r.g = *g;
    DRGNN_LAUNCH(k_conv_reduce, grid_items(conv_partial_floats(kind, F, H)), stream, conv_reduce_item(r, (int)bx), r);
    if (grad_x) DRGNN_LAUNCH(k_conv_bwd_dx, grid_items(n_nodes * F), stream, conv_bwd_dx_item(a, bx), a);
    return 0;
}

int drgnn_segpool_forward(const int32_t* ws_i32, int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                          const float* x, int32_t H, int32_t op, float* out, int64_t* arg, void* stream) {
    if (!ws_i32 || !x || !out || H < 1 || (op != 0 && op != 1)) return DRGNN_E_ARG;
    TopoLayout lay;
    topo_layout(n_nodes, n_edges, n_graphs, &lay);
    SegPoolArgs a;
    a.tv = topo_view(const_cast<int32_t*>(ws_i32), nullptr, lay);
    a.x = x; a.H = H; a.n_graphs = (int)n_graphs; a.op = op; a.out = out; a.arg = arg;
    a.grad_out = nullptr; a.grad_x = nullptr; a.arg_in = nullptr;
    DRGNN_LAUNCH(k_segpool_fwd, grid1(n_graphs), stream, segpool_fwd_block(a, (int)bx), a);
    return 0;
}

int drgnn_segmax_backward(const float* grad_out, const int64_t* arg, int64_t n_clusters, int32_t H,
                          int64_t n_nodes, float* grad_x, void* stream) {
    if (!grad_out || !arg || !grad_x) return DRGNN_E_ARG;
    SegPoolArgs a;
    a.H = H; a.grad_out = grad_out; a.arg_in = arg; a.grad_x = grad_x;
    a.x = nullptr; a.out = nullptr; a.arg = nullptr; a.n_graphs = 0; a.op = 0;
    const int64_t n_items = n_clusters * H;
    DRGNN_LAUNCH(k_segmax_bwd, grid_items(n_items), stream, segmax_bwd_item(a, bx, n_items, n_nodes), a, n_items, n_nodes);
    return 0;
}

int drgnn_pooled_edges_export(const int32_t* ws_i32, const float* ws_f32, int64_t n_nodes, int64_t n_edges,
                              int64_t n_graphs, int64_t e1_total, int64_t* edge_index, float* edge_attr,
                              void* stream) {
    if (!ws_i32 || (e1_total > 0 && !edge_index)) return DRGNN_E_ARG;
    TopoLayout lay;
    topo_layout(n_nodes, n_edges, n_graphs, &lay);
    EdgeExportArgs a;
    a.tv = topo_view(const_cast<int32_t*>(ws_i32), const_cast<float*>(ws_f32), lay);
    a.n_graphs = (int)n_graphs; a.edge_index = edge_index; a.edge_attr = edge_attr; a.e1_total = e1_total;
    DRGNN_LAUNCH(k_edge_export, grid1(n_graphs), stream, edge_export_block(a, (int)bx), a);
    return 0;
}

int drgnn_cluster_offset(int64_t* cluster, const int32_t* node_ptr, int64_t n_graphs, int64_t* scratch,
                         void* stream) {
    if (!cluster || !node_ptr || !scratch || n_graphs < 0) return DRGNN_E_ARG;
    if (n_graphs == 0) return 0;
    ClusterOffsetArgs a;
    a.cluster = cluster; a.nptr = node_ptr; a.n_graphs = (int)n_graphs; a.maxes = (long long*)scratch;
    DRGNN_EMU_ONLY(long long mm[2];)
    DRGNN_LAUNCH(k_cluster_max, grid1(n_graphs), stream, cluster_max_block(a, (int)bx, mm), a);
    DRGNN_LAUNCH(k_cluster_scan, grid1(1, 64), stream, cluster_scan_single(a), a);
    DRGNN_LAUNCH(k_cluster_add, grid1(n_graphs), stream, cluster_add_block(a, (int)bx), a);
    return 0;
}

// ---- graclus ----------------------------------------------------------------------------------------
int drgnn_graclus(const int32_t* ws_i32, int64_t n_nodes, int64_t n_edges, int64_t n_graphs, int32_t max_nodes,
                  int32_t max_edges, const float* weight, const int64_t* perm, int64_t* cluster, void* stream) {
    if (!ws_i32 || n_nodes < 0 || n_edges < 0 || n_graphs < 0 || max_nodes < 0 || max_edges < 0) return DRGNN_E_ARG;
    if (n_nodes > 0 && !cluster) return DRGNN_E_ARG;
    if (n_graphs == 0) return 0;
    TopoLayout lay;
    topo_layout(n_nodes, n_edges, n_graphs, &lay);
    GraclusArgs a;
    a.tv = topo_view(const_cast<int32_t*>(ws_i32), nullptr, lay);
    a.n_graphs = (int)n_graphs; a.weight = weight; a.perm = perm; a.cluster = cluster;
    a.capN = max_nodes > 0 ? max_nodes : 1; a.capE = max_edges > 0 ? max_edges : 1;
    const int64_t words = (int64_t)(a.capN + 1) + 2 * (int64_t)a.capE + a.capN;
    if (words * 4 > DRGNN_LDS_LIMIT) return DRGNN_E_CAPACITY;
    DRGNN_EMU_ONLY(std::vector<int> buf((size_t)words + 16);)
    DRGNN_LAUNCH(k_graclus, grid1(n_graphs, DRGNN_NTHREADS, words * 4), stream, graclus_block(a, (int)bx, buf.data()), a);
    return 0;
}

// ---- offline clustering ---------------------------------------------------------------------------
int drgnn_mcl(const int64_t* edge_index, int64_t n_edges, const int32_t* node_ptr, const int32_t* edge_ptr,
              const int64_t* mat_ptr, int64_t n_graphs, double* mat_scratch, int32_t* int_scratch,
              int64_t* labels, int32_t* info, void* stream) {
    if (!node_ptr || !edge_ptr || !mat_ptr || !mat_scratch || !int_scratch || !labels || !info || n_graphs < 0)
        return DRGNN_E_ARG;
    if (n_edges > 0 && !edge_index) return DRGNN_E_ARG;
    if (n_graphs == 0) return 0;
    MclArgs a;
    a.edge_index = edge_index; a.n_edges = n_edges; a.node_ptr = node_ptr; a.edge_ptr = edge_ptr;
    a.mat_ptr = mat_ptr; a.n_graphs = (int)n_graphs; a.mat = mat_scratch; a.iscr = int_scratch;
    a.labels = labels; a.info = info; a.iterations = 100; a.prune_threshold = 1e-3;
    DRGNN_EMU_ONLY(std::vector<double> red(DRGNN_NTHREADS); int flag[2];)
    DRGNN_LAUNCH(k_mcl, grid1(n_graphs), stream, mcl_graph(a, (int)bx, flag, red.data()), a);
    return 0;
}

int drgnn_louvain(const int64_t* edge_index, int64_t n_edges, const int32_t* node_ptr, const int32_t* edge_ptr,
                  int64_t n_graphs, int32_t max_nodes, int32_t max_edges, int64_t* labels, int32_t* info,
                  double* modularity, void* stream) {
    if (!node_ptr || !edge_ptr || !info || !modularity || n_graphs < 0 || n_edges < 0 || max_nodes < 0 ||
        max_edges < 0)
        return DRGNN_E_ARG;
    if (n_edges > 0 && !edge_index) return DRGNN_E_ARG;
    if (max_nodes > 0 && !labels) return DRGNN_E_ARG;
    if (n_graphs == 0) return 0;
    const int64_t words = louvain_lds_words(max_nodes, max_edges);
    if (words * 4 > DRGNN_LDS_LIMIT) return DRGNN_E_CAPACITY;
    LouvainArgs a;
    a.edge_index = edge_index; a.n_edges = n_edges; a.node_ptr = node_ptr; a.edge_ptr = edge_ptr;
    a.n_graphs = (int)n_graphs; a.capN = max_nodes; a.capE = max_edges;
    a.labels = labels; a.info = info; a.modularity = modularity;
    DRGNN_EMU_ONLY(std::vector<int> buf((size_t)words + 16);)
    DRGNN_LAUNCH(k_louvain, grid1(n_graphs, LV_W, words * 4), stream, louvain_graph(a, (int)bx, buf.data()), a);
    return 0;
}

}  // extern "C"
