// drgnn_capi.hip -- the training path of the extern "C" surface declared in include/drgnn.h: layout queries, topology builder,
// launch pair, fused step, head, Adam, p2p, the update launches, collation and the epoch loop, with its kernels
// (drgnn_kernels.h).  The feature entry points live next to it, one unit per subsystem, named after the Python modules that
// call them: drgnn_capi_layers.hip, _iface.hip, _residues.hip, _poses.hip, _metrics.hip.  What several units use is in
// drgnn_capi_common.h.
//
// Built twice from these sources, every drgnn_capi*.hip:
//   hipcc --offload-arch=gfx950 -> csrc/libdrgnn.so        (the product: an object per unit, Makefile)
//   g++ -x c++ -DDRGNN_EMU      -> tests/emu/build/libdrgnn_emu.so (CPU test-suite only:
//        every "launch" becomes a loop over workgroups on host pointers; ONE unit: tests/emu/build_emu.sh compiles this
//        file, which includes the feature units at its end)
//
// The entry points write their launch sequence ONCE for both builds, with DRGNN_LAUNCH / DRGNN_EMU_ONLY / drgnn_clear of
// drgnn_launch.h: the checks, phases, guards and early returns the CPU suite runs are the ones the GPU runs.  That holds for
// the feature entry points (the drgnn_capi_<subsystem>.hip units) and for the launches of the training path: the topology
// builder (topo_launch) and its prologue, the launch pair (net_launch, its co-built builder included), the head, the flat Adam,
// the all-reduce, collation and the epoch loop's clear.  A new feature entry point touches two places, both its subsystem's
// own: its block function in drgnn_<subsystem>.h, and its __global__ wrapper, checks and launches in
// drgnn_capi_<subsystem>.hip; a new UNIT also gets its include line at the end of this file.  A DRGNN_EMU conditional says on
// its line why the builds differ in what they DO: the fused step (emu_step stands in for the aggregation-first kernels, so its
// pick, checks, plans and launch differ), the device queries, drgnn_topology_status, the update / gradient / reduce launches
// and adam_opt_impl (item-wise sums against the kernels' blocks), the drgnn_p2p_* allocation functions and the profiling hook.
#define DRGNN_KERNELS_MAIN
#include "drgnn_kernels.h"

#include "drgnn_capi_common.h"


// =====================================================================================
// host side
// =====================================================================================
extern "C" {

int drgnn_abi_version(void) { return DRGNN_ABI_VERSION; }

#if defined(DRGNN_PHASE_TIMING) && !defined(DRGNN_EMU)
// profiling build only: where phase_mark() writes (device buffer of >= 4002 uint64)
int drgnn_debug_set_phase_buffer(void* dev_buf) {
    unsigned long long* p = (unsigned long long*)dev_buf;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_phase_buf), &p, sizeof(p));
}
#endif

int drgnn_topology_layout(int64_t n_nodes, int64_t n_edges, int64_t n_graphs, int64_t* off_i32,
                          int64_t* off_f32) {
    if (n_nodes < 0 || n_edges < 0 || n_graphs < 0 || !off_i32 || !off_f32) return DRGNN_E_ARG;
    TopoLayout L;
    topo_layout(n_nodes, n_edges, n_graphs, &L);
    for (int k = 0; k <= DRGNN_TI_COUNT; ++k) off_i32[k] = L.i32[k];
    for (int k = 0; k <= DRGNN_TF_COUNT; ++k) off_f32[k] = L.f32[k];
    return 0;
}

int64_t drgnn_topology_scratch_elems(int64_t n_nodes, int64_t n_edges, int64_t n_graphs) {
    return topo_gscratch_base(n_nodes, n_edges, n_graphs) + TOPO_GSCRATCH_CONST;
}

// tile_f > 0: + the x tile of the aggregation tiles (DRGNN_TOPO_TILES)
static int64_t topo_lds_bytes(int capN, int capE, int tile_f = 0) {
    const int64_t capT = (capN > capE ? capN : capE) + 1;
    // (the x tile's rows are padded to pad4(F) + 4 floats)
    return 4 * (topo_scratch_ints(capN, capE, capT, (int64_t)capN + capE + 2) + (tile_f > 0 ? (int64_t)capN * (((tile_f + 3) & ~3) + 4) : 0));
}
static bool topo_tiles_shape_ok(int capN, int capE, int F) {
    const int TF = (F + 3) & ~3;
    if (capN <= 0 || F <= 0 || F > 256 || (int64_t)capN * TF > 16 * DRGNN_BCAP) return false;      // (x tile: 4 float4 per lane)
    return topo_lds_bytes(capN, capE > 0 ? capE : 1, F) <= DRGNN_LDS_LIMIT;
}

int64_t drgnn_topology_lds_bytes(int32_t max_nodes, int32_t max_edges) {
    if (max_nodes <= 0) return 0;
    return topo_lds_bytes(max_nodes, max_edges > 0 ? max_edges : 1);
}

int64_t drgnn_topology_tiles_elems(int64_t n_nodes, int32_t n_feat) {
    if (n_nodes < 0 || n_feat <= 0) return 0;
    const int64_t TF = ((int64_t)n_feat + 3) & ~(int64_t)3;      // S [n][TF] | D [n] | C [n] | (F % 4 != 0) X [n][TF]
    return (n_feat & 3) ? drgnn_tiles_x_off(n_nodes, TF) + n_nodes * TF : n_nodes * (TF + 2);
}
int32_t drgnn_topology_tiles_ok(int32_t max_nodes, int32_t max_edges, int32_t n_feat) {
    return topo_tiles_shape_ok(max_nodes, max_edges, n_feat) ? 1 : 0;
}

}  // extern "C"

#ifndef DRGNN_TOPO_SPLIT_MAX_GRAPHS
#define DRGNN_TOPO_SPLIT_MAX_GRAPHS 160
#endif
// fills a TopoLaunch from the public arguments; *lds_out = LDS bytes (0: global scratch path)
static int topo_prepare(TopoLaunch& L, int64_t* lds_out, const int64_t* edge_index, const float* edge_attr,
                        const int64_t* batch, const int64_t* cluster0, const int64_t* cluster1,
                        const int32_t* node_ptr, const int32_t* edge_ptr, const int32_t* c1_ptr,
                        int64_t n_nodes, int64_t n_edges, int64_t len_cluster1, int64_t n_graphs,
                        int32_t max_nodes, int32_t max_edges, int32_t* ws_i32, float* ws_f32,
                        int32_t* scratch_i32, int32_t flags = DRGNN_TOPO_HIER, const float* x_in = nullptr,
                        float* tiles = nullptr, int32_t tile_f = 0) {
    if (n_nodes < 0 || n_edges < 0 || n_graphs < 0 || !ws_i32) return DRGNN_E_ARG;
    if (!batch && !(node_ptr && edge_ptr)) return DRGNN_E_ARG;      // the offsets are derived from `batch`
    if (!cluster0 && cluster1) return DRGNN_E_ARG;
    if (n_edges > 0 && !edge_index) return DRGNN_E_ARG;
    if (edge_attr && !ws_f32) return DRGNN_E_ARG;
    if (n_nodes + n_graphs >= INT32_MAX || n_edges >= INT32_MAX) return DRGNN_E_CAPACITY;
    TopoLayout lay;
    topo_layout(n_nodes, n_edges, n_graphs, &lay);
    L.tv = topo_view(ws_i32, ws_f32, lay);
    L.args.edge_index = edge_index;
    L.args.edge_attr = edge_attr;
    L.args.cluster0 = cluster0;
    L.args.cluster1 = cluster1;
    L.args.c1_ptr = c1_ptr;
    L.args.n_edges = n_edges;
    L.args.len_cluster1 = len_cluster1;
    L.args.n_graphs = (int)n_graphs;
    L.args.set_ids = nullptr; L.args.set_node_ptr = L.args.set_edge_ptr = L.args.set_c1_ptr = nullptr;
    L.args.set_x = nullptr; L.args.set_y = nullptr; L.args.x_out = nullptr; L.args.y_out = nullptr;
    L.args.n_set = 0; L.args.n_feat = 0; L.args.y_bytes = 0;
    L.args.flags = flags;
    L.args.x_in = nullptr; L.args.tiles = nullptr; L.args.tile_nodes = n_nodes; L.args.tile_f = 0;
    if (flags & DRGNN_TOPO_TILES) {
        // the aggregation tiles need the hierarchical order's companions, an output buffer and float4-loadable features
        // (x_in null: resident-set mode, the caller fills in the set's x and checks it)
        if (!(flags & DRGNN_TOPO_HIER) || !tiles || (x_in && !(tile_f & 3) && (((uintptr_t)x_in) & 15)) || (((uintptr_t)tiles) & 15)) return DRGNN_E_ARG;
        if (!topo_tiles_shape_ok(max_nodes, max_edges, tile_f)) return DRGNN_E_CAPACITY;
        L.args.x_in = x_in; L.args.tiles = tiles; L.args.tile_f = tile_f;
    }
    L.gscratch = scratch_i32;
    L.level1_only = 0;
    L.roles = 1;
    L.pf_ids = nullptr; L.pf_n = 0; L.pf_graphs = 0;
    L.user_nptr = (node_ptr && edge_ptr) ? node_ptr : nullptr;
    L.user_eptr = (node_ptr && edge_ptr) ? edge_ptr : nullptr;
    int64_t lds = 0;
    L.capN = 0; L.capE = 0;
    if (max_nodes > 0) {
        lds = topo_lds_bytes(max_nodes, max_edges > 0 ? max_edges : 1, L.args.tile_f);
        if (lds <= DRGNN_LDS_LIMIT) { L.capN = max_nodes; L.capE = max_edges > 0 ? max_edges : 1; }
        else lds = 0;
    }
    if (L.args.tile_f > 0 && L.capN == 0) return DRGNN_E_CAPACITY;      // (tiles are formed by the LDS builder only)
    // two independent workgroups per graph (edge structures / member lists) when nothing forces the
    // single-chain order: LDS path, clusters present, depth-1 ids located by the caller
    // ... and when the extra workgroups find idle CUs: two workgroups per graph shorten the builder's critical path
    // (what counts while a mini-batch leaves CUs idle) but repeat the cluster ranking; beyond ~one workgroup per CU the
    // total work decides and one workgroup per graph does less of it
    if (L.capN > 0 && cluster0 != nullptr && L.user_nptr != nullptr && !(cluster1 != nullptr && c1_ptr == nullptr) &&
        n_graphs <= DRGNN_TOPO_SPLIT_MAX_GRAPHS)
        L.roles = 2;
    *lds_out = lds;
    return 0;
}

// a request in either mode -> launch description
static int topo_prepare_req(TopoLaunch& T, int64_t* tlds, const drgnn_topology_request* r) {
    const drgnn_graph_set* gs = r->set;
    if (!gs)
        return topo_prepare(T, tlds, r->edge_index, r->edge_attr, r->batch, r->cluster0, r->cluster1, r->node_ptr,
                            r->edge_ptr, r->c1_ptr, r->n_nodes, r->n_edges, r->len_cluster1, r->n_graphs, r->max_nodes,
                            r->max_edges, r->ws_i32, r->ws_f32, r->scratch_i32, r->flags, r->x, r->tiles, r->n_feat);
    if (!r->ids || !r->node_ptr || !r->edge_ptr || !gs->node_ptr || !gs->edge_ptr || !gs->cluster0) return DRGNN_E_ARG;
    if (gs->cluster1 && (!gs->c1_ptr || !r->c1_ptr)) return DRGNN_E_ARG;
    if (r->x_out && (!gs->x || gs->n_feat <= 0)) return DRGNN_E_ARG;
    if (r->y_out && (!gs->y || (gs->y_bytes != 4 && gs->y_bytes != 8))) return DRGNN_E_ARG;
    const float* attr = (r->ws_f32 && gs->edge_attr) ? gs->edge_attr : nullptr;
    if ((r->flags & DRGNN_TOPO_TILES) && (!gs->x || gs->n_feat <= 0 || (!(gs->n_feat & 3) && (((uintptr_t)gs->x) & 15)))) return DRGNN_E_ARG;
    const int rc = topo_prepare(T, tlds, gs->edge_index, attr, nullptr, gs->cluster0, gs->cluster1, r->node_ptr,
                                r->edge_ptr, r->c1_ptr, r->n_nodes, r->n_edges, r->len_cluster1, r->n_graphs,
                                r->max_nodes, r->max_edges, r->ws_i32, r->ws_f32, r->scratch_i32, r->flags, nullptr, r->tiles,
                                gs->n_feat);
    if (rc) return rc;
    TopoArgs& a = T.args;
    a.n_edges = gs->n_edges;                  // row stride of the SET's edge_index
    a.set_ids = r->ids; a.set_node_ptr = gs->node_ptr; a.set_edge_ptr = gs->edge_ptr; a.set_c1_ptr = gs->c1_ptr;
    a.set_x = gs->x; a.set_y = gs->y; a.x_out = r->x_out; a.y_out = r->y_out;
    a.n_set = gs->n_graphs; a.n_feat = gs->n_feat; a.y_bytes = gs->y_bytes;
    return 0;
}

// One launch of a prepared builder: out of `lds` bytes of LDS at L.roles workgroups per graph, or out of the global scratch.
static int topo_launch(const TopoLaunch& L, int64_t lds, void* stream) {
    DRGNN_EMU_ONLY(std::vector<int> buf((size_t)(lds / 4) + 16);)
    if (L.capN > 0)
        DRGNN_LAUNCH(k_topo<true>, grid1((int64_t)L.args.n_graphs * L.roles, DRGNN_NTHREADS, lds), stream,
                     topo_block<true>(L, (int)bx, buf.data()), L);
    else
        DRGNN_LAUNCH(k_topo<false>, grid1(L.args.n_graphs), stream, topo_block<false>(L, (int)bx, buf.data()), L);
    return 0;
}

static int topology_build_impl(const int64_t* edge_index, const float* edge_attr, const int64_t* batch,
                         const int64_t* cluster0, const int64_t* cluster1, const int32_t* node_ptr,
                         const int32_t* edge_ptr, const int32_t* c1_ptr, int64_t n_nodes,
                         int64_t n_edges, int64_t len_cluster1, int64_t n_graphs, int32_t max_nodes,
                         int32_t max_edges, int32_t* ws_i32, float* ws_f32, int32_t* scratch_i32,
                         int32_t flags, void* stream, const float* x_in = nullptr, float* tiles = nullptr,
                         int32_t tile_f = 0) {
    TopoLaunch L;
    int64_t lds = 0;
    int rc0 = topo_prepare(L, &lds, edge_index, edge_attr, batch, cluster0, cluster1, node_ptr, edge_ptr, c1_ptr,
                           n_nodes, n_edges, len_cluster1, n_graphs, max_nodes, max_edges, ws_i32, ws_f32,
                           scratch_i32, flags, x_in, tiles, tile_f);
    if (rc0) return rc0;
    if (L.capN == 0 && !scratch_i32) return DRGNN_E_CAPACITY;
    if (n_graphs == 0) return 0;
    PtrArgs pa;
    pa.batch = batch; pa.edge_row = edge_index; pa.n_nodes = n_nodes; pa.n_edges = n_edges;
    pa.n_graphs = (int)n_graphs; pa.nptr = L.tv.p[DRGNN_TI_NPTR]; pa.eptr = L.tv.p[DRGNN_TI_EPTR];
    pa.err = L.tv.p[DRGNN_TI_ERR];
    if (!(node_ptr && edge_ptr)) {
        // the offsets prologue.  k_topo_begin has no tables to copy here: what is left of it is the clear of the four status
        // words, which the emulation spells out (the kernel has no item function to name)
        const int n = (int)n_graphs + 1;
        const int64_t span = n_nodes > n_edges ? n_nodes : n_edges;
        DRGNN_LAUNCH(k_topo_begin, grid_items(n), stream, if (bx == 0) memset(pa.err, 0, 4 * sizeof(int32_t)),
                     (const int32_t*)nullptr, (const int32_t*)nullptr, pa.nptr, pa.eptr, pa.err, n);
        DRGNN_LAUNCH(k_ptrs, grid_items(span > 0 ? span : 1), stream, ptr_item(pa, bx), pa);
    }
    // a second pass for the depth-1 clusters when their offsets were not supplied (they follow from the first pass)
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) { if (!(cluster1 && !c1_ptr)) break; L.level1_only = 1; L.roles = 1; }
        if ((rc0 = topo_launch(L, lds, stream))) return rc0;
    }
    return 0;
}

extern "C" {

int drgnn_topology_build(const int64_t* edge_index, const float* edge_attr, const int64_t* batch,
                         const int64_t* cluster0, const int64_t* cluster1, const int32_t* node_ptr,
                         const int32_t* edge_ptr, const int32_t* c1_ptr, int64_t n_nodes,
                         int64_t n_edges, int64_t len_cluster1, int64_t n_graphs, int32_t max_nodes,
                         int32_t max_edges, int32_t* ws_i32, float* ws_f32, int32_t* scratch_i32,
                         void* stream_) {
    return topology_build_impl(edge_index, edge_attr, batch, cluster0, cluster1, node_ptr, edge_ptr, c1_ptr, n_nodes, n_edges,
                               len_cluster1, n_graphs, max_nodes, max_edges, ws_i32, ws_f32, scratch_i32, DRGNN_TOPO_HIER,
                               stream_);
}

int drgnn_topology_build_request(const drgnn_topology_request* r, void* stream_) {
    if (!r) return DRGNN_E_ARG;
    if (!r->set)
        return topology_build_impl(r->edge_index, r->edge_attr, r->batch, r->cluster0, r->cluster1, r->node_ptr,
                                   r->edge_ptr, r->c1_ptr, r->n_nodes, r->n_edges, r->len_cluster1, r->n_graphs,
                                   r->max_nodes, r->max_edges, r->ws_i32, r->ws_f32, r->scratch_i32, r->flags, stream_,
                                   r->x, r->tiles, r->n_feat);
    TopoLaunch L;
    int64_t lds = 0;
    const int rc = topo_prepare_req(L, &lds, r);
    if (rc) return rc;
    if (L.capN == 0 && !r->scratch_i32) return DRGNN_E_CAPACITY;
    return topo_launch(L, lds, stream_);      // (a request without graphs: an empty grid)
}

int drgnn_topology_tiles(const int32_t* ws_i32, const float* ws_f32, int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                         const float* x, int32_t n_feat, int32_t use_weights, float* tiles, void* stream) {
    if (!ws_i32 || !x || !tiles || n_nodes < 0 || n_edges < 0 || n_graphs < 0 || n_feat <= 0) return DRGNN_E_ARG;
    if (use_weights && !ws_f32) return DRGNN_E_ARG;
    if (n_graphs == 0) return 0;
    TopoLayout lay;
    topo_layout(n_nodes, n_edges, n_graphs, &lay);
    TilesArgs a;
    a.tv = topo_view(const_cast<int32_t*>(ws_i32), const_cast<float*>(ws_f32), lay);
    a.x = x; a.tiles = tiles; a.n_nodes = n_nodes; a.n_feat = n_feat; a.use_weights = use_weights ? 1 : 0;
    DRGNN_LAUNCH(k_tiles, grid1(n_graphs), stream, tiles_block(a, (int)bx), a);
    return 0;
}

int drgnn_batch_offsets(const drgnn_graph_set* set, const int32_t* ids, int64_t n_ids, int32_t batch_size,
                        int32_t* ptrs, void* stream) {
    if (!set || !ids || !ptrs || n_ids < 0 || batch_size < 1 || !set->node_ptr || !set->edge_ptr) return DRGNN_E_ARG;
    if (batch_size > 4096) return DRGNN_E_CAPACITY;
    if (n_ids == 0) return 0;
    OffsetsArgs a;
    a.set = *set; a.ids = ids; a.n_ids = n_ids; a.batch_size = batch_size; a.ptrs = ptrs;
    const int64_t nb = (n_ids + batch_size - 1) / batch_size;
    // (batch_size <= 4096: at most 53 276 bytes of dynamic LDS, never beyond 64 KiB)
    const int64_t words = (int64_t)DRGNN_NTHREADS + 4 + 3 * ((int64_t)batch_size + 1);
    DRGNN_EMU_ONLY(std::vector<int> buf((size_t)words);)
    DRGNN_LAUNCH(k_batch_offsets, grid1(nb, DRGNN_NTHREADS, words * 4), stream,
                 batch_offsets_block(a, (int)bx, buf.data() + DRGNN_NTHREADS + 4, buf.data()), a);
    return 0;
}

int drgnn_topology_finalize(int32_t* ws_i32, int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                            void* stream) {
    if (!ws_i32 || n_graphs < 0) return DRGNN_E_ARG;
    TopoLayout lay;
    topo_layout(n_nodes, n_edges, n_graphs, &lay);
    ScanArgs a;
    a.tv = topo_view(ws_i32, nullptr, lay);
    a.n_graphs = (int)n_graphs;
    DRGNN_EMU_ONLY(int part[DRGNN_NTHREADS + 4];)
    DRGNN_LAUNCH(k_finalize, grid1(1), stream, finalize_block(a, part), a);
    return 0;
}

int drgnn_topology_status(const int32_t* ws_i32, int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                          int32_t* status4, void* stream_) {
    if (!ws_i32 || !status4) return DRGNN_E_ARG;
    TopoLayout lay;
    topo_layout(n_nodes, n_edges, n_graphs, &lay);
    const int32_t* err = ws_i32 + lay.i32[DRGNN_TI_ERR];
    const int32_t* gst = ws_i32 + lay.i32[DRGNN_TI_GSTAT];
    std::vector<int32_t> host((size_t)(2 * n_graphs) + 4);
#ifdef DRGNN_EMU      // no launch: the device copies the words to the host and waits, the emulation reads them where they are
    for (int k = 0; k < 4; ++k) host[k] = err[k];
    for (int64_t g = 0; g < 2 * n_graphs; ++g) host[4 + g] = gst[g];
    (void)stream_;
#else
    HIP_TRY(hipMemcpyAsync(host.data(), err, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream_));
    if (n_graphs > 0)
        HIP_TRY(hipMemcpyAsync(host.data() + 4, gst, 2 * n_graphs * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream_));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
#endif
    status4[0] = host[0]; status4[1] = -1; status4[2] = 0; status4[3] = 0;
    for (int64_t g = 0; g < n_graphs; ++g) {
        host[4 + g] |= host[4 + n_graphs + g];       // edge-structure and member-list workgroups
        if (host[4 + g]) {
            status4[0] |= host[4 + g];
            if (status4[1] < 0) status4[1] = (int32_t)g;
            status4[2] += 1;
        }
    }
    return 0;
}

// ---- fused net ----------------------------------------------------------------------
// the LDS capacities a launch's bounds ask for: room for one edge at least; max_c0 counts only where it bounds anything
struct StepCaps { int N, E, C; };
static StepCaps step_caps(int32_t max_nodes, int32_t max_edges, int32_t max_c0) {
    return StepCaps{max_nodes, max_edges > 0 ? max_edges : 1, (max_c0 > 0 && max_c0 < max_nodes) ? max_c0 : max_nodes};
}

int64_t drgnn_net_lds_bytes(int32_t kind, int32_t n_feat, int32_t max_nodes, int32_t max_edges,
                            int32_t max_c0, int32_t backward) {
    if (max_nodes <= 0) return 0;
    const StepCaps c = step_caps(max_nodes, max_edges, max_c0);
    return 4 * net_scratch_words(kind, n_feat, c.N, c.E, c.C, backward);
}

int64_t drgnn_net_partial_elems(int32_t kind, int32_t n_feat) { (void)kind; return net_partial_floats(n_feat); }

int64_t drgnn_net_scratch_elems(int32_t kind, int32_t n_feat, int64_t n_nodes, int64_t n_edges,
                                int64_t n_graphs) {
    const int nb = (kind == DRGNN_GINET) ? 2 : 1;
    const int64_t f = net_gscratch_base(kind, n_feat, n_nodes, n_edges, n_graphs, 0);
    const int64_t b = net_gscratch_base(kind, n_feat, n_nodes, n_edges, n_graphs, 1);
    return nb * (f > b ? f : b) + 64;
}

}  // extern "C"

static int net_check(const drgnn_net_desc* net) {
    if (!net) return DRGNN_E_ARG;
    if (net->kind < DRGNN_GINET || net->kind > DRGNN_FOUT) return DRGNN_E_ARG;
    if (net->n_branch < 1 || net->n_branch > DRGNN_MAX_BRANCH) return DRGNN_E_ARG;
    if (net->n_feat < 1) return DRGNN_E_WIDTH;
    for (int b = 0; b < net->n_branch; ++b) {
        if (!net->conv1[b].w_nbr || !net->conv2[b].w_nbr) return DRGNN_E_ARG;
        if (net->kind != DRGNN_GINET &&
            (!net->conv1[b].w_self || !net->conv2[b].w_self || !net->conv1[b].bias || !net->conv2[b].bias))
            return DRGNN_E_ARG;
    }
    return 0;
}

// the one dispatch over a net's kind: launch(kind as a compile-time constant)
template <class Launch>
static int net_by_kind(int kind, Launch launch) {
    switch (kind) {
    case DRGNN_GINET: return launch(std::integral_constant<int, DRGNN_GINET>());
    case DRGNN_SGAT: return launch(std::integral_constant<int, DRGNN_SGAT>());
    default: return launch(std::integral_constant<int, DRGNN_FOUT>());
    }
}

// *co_built (when given): the topology of `co` has been built by this launch as well
template <bool BWD>
static int net_launch(NetLaunch& L, int32_t max_nodes, int32_t max_edges, int32_t max_c0, float* scratch,
                      void* stream, const TopoLaunch* co = nullptr, int64_t co_lds = 0, bool* co_built = nullptr) {
    const int kind = L.a.net.kind;
    const int64_t lds = drgnn_net_lds_bytes(kind, L.a.net.n_feat, max_nodes, max_edges, max_c0, BWD ? 1 : 0);
    L.capN = 0; L.capE = 0; L.capC = 0; L.gscratch = scratch;
    int64_t use_lds = 0;
    L.a.hf.stage = 0;
    if (lds > 0 && lds <= DRGNN_LDS_LIMIT) {
        const StepCaps c = step_caps(max_nodes, max_edges, max_c0);
        L.capN = c.N; L.capE = c.E; L.capC = c.C;
        use_lds = lds;
        if (BWD && L.a.hf.enabled) {    // room to keep the head's weights in LDS as well?
            const int64_t extra = drgnn_net_head_stage_bytes(L.a.hf.R, L.a.hf.H, L.a.hf.O);
            if (use_lds + extra <= DRGNN_LDS_LIMIT) { use_lds += extra; L.a.hf.stage = 1; }
        }
    } else if (!scratch) {
        return DRGNN_E_CAPACITY;
    }
    const int blocks = L.a.n_graphs * L.a.net.n_branch;
    // co-launched topology build of the next mini-batch: only when both jobs run out of LDS and the
    // builder needs no helper passes (offsets supplied, depth-1 ids located)
    const bool co_ok = co != nullptr && use_lds > 0 && co->capN > 0 && co->user_nptr != nullptr &&
                       !(co->args.cluster1 != nullptr && co->args.c1_ptr == nullptr) && co->args.n_graphs > 0 &&
                       blocks > 0;
    const int64_t all_lds = (co_ok && co_lds > use_lds) ? co_lds : use_lds;
    DRGNN_EMU_ONLY(std::vector<float> buf((size_t)(all_lds / 4) + 16);)
    if (co_ok) {      // the builder's workgroups behind the net's, in the same grid
        CoLaunch C;
        C.net = L; C.topo = *co; C.n_net = blocks;
        const int rc = net_by_kind(kind, [&](auto K) {
            constexpr int KIND = decltype(K)::value;
            DRGNN_LAUNCH((k_net_co_topo<KIND, BWD>), grid1(blocks + (int64_t)co->args.n_graphs * co->roles, DRGNN_NTHREADS, all_lds),
                         stream, (bx < blocks ? net_block<KIND, BWD, true>(C.net, (int)bx, buf.data())
                                              : topo_block<true>(C.topo, (int)bx - blocks, (int*)buf.data())), C);
            return 0;
        });
        if (co_built) *co_built = rc == 0;
        return rc;
    }
    // (a launch without graphs: an empty grid)
    return net_by_kind(kind, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        if (use_lds)
            DRGNN_LAUNCH((k_net<KIND, BWD, true>), grid1(blocks, DRGNN_NTHREADS, use_lds), stream,
                         (net_block<KIND, BWD, true>(L, (int)bx, buf.data())), L);
        else
            DRGNN_LAUNCH((k_net<KIND, BWD, false>), grid1(blocks), stream,
                         (net_block<KIND, BWD, false>(L, (int)bx, buf.data())), L);
        return 0;
    });
}

// what a forward and a backward launch share; the rest as for a launch that writes no readout, reads no gradient and has no head
static void net_fill(NetLaunch& L, const drgnn_net_desc* net, const float* x, const int32_t* ws_i32, const float* ws_f32,
                     int64_t n_nodes, int64_t n_edges, int64_t n_graphs, float* xp, int32_t* arg0, int32_t* arg1, int32_t* step_inc) {
    TopoLayout lay;
    topo_layout(n_nodes, n_edges, n_graphs, &lay);
    L.a.net = *net;
    L.a.x = x;
    L.a.tv = topo_view(const_cast<int32_t*>(ws_i32), const_cast<float*>(ws_f32), lay);
    L.a.n_nodes = n_nodes;
    L.a.n_graphs = (int)n_graphs;
    L.a.xp = xp; L.a.arg0 = arg0; L.a.arg1 = arg1; L.a.readout = nullptr;
    L.a.grad_readout = nullptr; L.a.partials = nullptr; L.a.grad_x = nullptr; L.a.n_partial = 0;
    L.a.step_inc = step_inc;
    L.a.hf.enabled = 0;
    L.n_edges = n_edges;
}

extern "C" {

int drgnn_net_forward(const drgnn_net_desc* net, const float* x, const int32_t* ws_i32,
                      const float* ws_f32, int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                      int32_t max_nodes, int32_t max_edges, int32_t max_c0, float* xp, int32_t* arg0,
                      int32_t* arg1, float* readout, float* scratch_f32, int32_t* step_inc, void* stream_) {
    int rc = net_check(net);
    if (rc) return rc;
    if (!x || !ws_i32 || !xp || !arg0 || !arg1 || !readout) return DRGNN_E_ARG;
    if (net->kind == DRGNN_SGAT && !ws_f32) return DRGNN_E_ARG;
    NetLaunch L;
    net_fill(L, net, x, ws_i32, ws_f32, n_nodes, n_edges, n_graphs, xp, arg0, arg1, step_inc);
    L.a.readout = readout;
    return net_launch<false>(L, max_nodes, max_edges, max_c0, scratch_f32, stream_);
}

static int net_backward_impl(const drgnn_net_desc* net, const float* x, const float* grad_readout,
                             const HeadFused* hf, const int32_t* ws_i32, const float* ws_f32,
                             int64_t n_nodes, int64_t n_edges, int64_t n_graphs, int32_t max_nodes,
                             int32_t max_edges, int32_t max_c0, const float* xp, const int32_t* arg0,
                             const int32_t* arg1, float* grad_x, float* partials, float* scratch_f32,
                             int32_t* step_inc, void* stream_, const drgnn_topology_request* next = nullptr) {
    int rc = net_check(net);
    if (rc) return rc;
    if (!x || (!grad_readout && !hf) || !ws_i32 || !xp || !arg0 || !arg1 || !partials) return DRGNN_E_ARG;
    NetLaunch L;
    net_fill(L, net, x, ws_i32, ws_f32, n_nodes, n_edges, n_graphs, const_cast<float*>(xp), const_cast<int32_t*>(arg0),
             const_cast<int32_t*>(arg1), step_inc);
    L.a.grad_readout = grad_readout; L.a.partials = partials; L.a.grad_x = grad_x;
    L.a.n_partial = (int)net_partial_floats(net->n_feat);
    if (hf) L.a.hf = *hf;
    if (!next) return net_launch<true>(L, max_nodes, max_edges, max_c0, scratch_f32, stream_);
    TopoLaunch T;
    int64_t tlds = 0;
    rc = topo_prepare_req(T, &tlds, next);
    if (rc) return rc;
    bool co_built = false;
    rc = net_launch<true>(L, max_nodes, max_edges, max_c0, scratch_f32, stream_, &T, tlds, &co_built);
    if (rc || co_built) return rc;
    // could not share the launch: build the next topology with its own launches
    return drgnn_topology_build_request(next, stream_);
}

}  // extern "C"

#ifdef DRGNN_EMU      // (emu_step: what the emulation runs in place of the aggregation-first kernels)
// The host emulation's fused step.  The aggregation-first kernels are SIMT code (MFMA fragments, DPP, lane reads) the
// emulation cannot execute; it steps the launch with the launch pair's per-graph routines instead -- net_forward_graph for
// both branches, then net_backward_graph with head_graph inside (inference: head_graph alone) -- and writes what the fused
// step writes: pred, readout [B, R], one compact head slab per graph (head_graph's slab without its H x R dW_fc1 block), one
// conv slab per (graph, branch) and Adam's step index step2[1].  Slot g reads graph gather_ids[g] of the workspace in cached
// mode; xp / argmax, the full head slabs and the targets by slot live in host buffers.
template <int KIND>
static void emu_step(const StepArgs& a, bool train, int capN, int capE, int capC) {
    const HeadFused& hf = a.hf;
    const int B = a.n_graphs, nb = a.net.n_branch, R = hf.R, H = hf.H, O = hf.O, F = a.net.n_feat;
    const int64_t P = head_partial_floats(R, H, O), PC = head_compact_floats(R, H, O);
    std::vector<float> xp((size_t)nb * a.n_nodes * DRGNN_H1), full((size_t)B * P), y_reg(B, 0.0f);
    std::vector<int32_t> arg0(xp.size()), arg1((size_t)nb * a.n_nodes * DRGNN_H2);
    std::vector<int64_t> y_cls(B, 0);
    const int64_t w0 = net_scratch_words(KIND, F, capN, capE, capC, 0), w1 = net_scratch_words(KIND, F, capN, capE, capC, 1);
    std::vector<float> scratch((size_t)(w0 > w1 ? w0 : w1) + 16), gp(1024 + H + R + 2 * DRGNN_MAX_OUT), dr(DRGNN_H2);
    auto graph_of = [&](int g) { return a.gather_ids ? a.gather_ids[g] : g; };
    for (int g = 0; g < B && train; ++g) {      // (head_graph reads the target of slot g; inference: zero targets, loss unused)
        if (hf.y_reg) y_reg[g] = hf.y_reg[graph_of(g)];
        if (hf.y_cls) y_cls[g] = hf.y_cls[graph_of(g)];
    }
    NetArgs n;
    n.net = a.net; n.x = a.x; n.tv = a.tv; n.n_nodes = a.n_nodes; n.n_graphs = a.ws_graphs;
    n.xp = xp.data(); n.arg0 = arg0.data(); n.arg1 = arg1.data(); n.readout = const_cast<float*>(hf.readout);
    n.grad_readout = nullptr; n.partials = a.partials; n.grad_x = nullptr; n.n_partial = a.n_partial; n.step_inc = nullptr;
    n.hf = hf;
    n.hf.y_reg = y_reg.data(); n.hf.y_cls = y_cls.data(); n.hf.partials = full.data(); n.hf.stage = 0;
    for (int g = 0; g < B; ++g) {
        const int gi = graph_of(g);
        const GraphDims d = net_dims(a.tv, gi);
        if (d.N > capN || d.E > capE || d.C > capC) {      // the caller's bounds were wrong: poisoned outputs, as on the device
            for (int c = 0; c < R; ++c) n.readout[(long)g * R + c] = DRGNN_NAN;
            for (int64_t i = 0; i < PC && train; ++i) hf.partials[g * PC + i] = DRGNN_NAN;
            for (int o = 0; o < O; ++o) hf.pred[(long)g * O + o] = DRGNN_NAN;
            continue;
        }
        for (int br = 0; br < nb; ++br) net_forward_graph<KIND>(n, g, gi, br, scratch.data(), capN, capE, capC);
        if (!train) {
            head_graph(n.hf, g, 0, gp.data(), dr.data(), hf.w1, R, hf.b1, hf.w2, hf.b2, hf.readout + (long)g * R);
            continue;
        }
        for (int br = 0; br < nb; ++br) net_backward_graph<KIND>(n, g, gi, br, scratch.data(), capN, capE, capC);
        memcpy(hf.partials + g * PC, full.data() + g * P + (int64_t)H * R, (size_t)PC * 4);
    }
    if (train) a.step2[1] = a.step2[0] + 1;
}
#endif

// The head of a fused launch from its descriptor.  upstream: a TASK_GRAD target is the upstream gradient, read where a regression
// target is (the fused step; the launch pair has no such task); step_bias, train: drgnn_net.h, HeadFused.
static void head_fused_fill(HeadFused& hf, const drgnn_head_desc* hd, int64_t n_graphs, const void* target, bool upstream, int step_bias,
                            int train, const float* readout, const int32_t* step, float* pred, float* partials) {
    hf.enabled = 1; hf.B = (int)n_graphs; hf.R = hd->R; hf.H = hd->H; hf.O = hd->O; hf.task = hd->task;
    hf.p_drop = hd->train ? hd->p_drop : 0.0f; hf.seed = hd->seed; hf.step_bias = step_bias; hf.train = train; hf.sigmoid = hd->transform_sigmoid;
    hf.drop_mask = hd->train ? hd->drop_mask : nullptr;
    hf.w1 = hd->w1; hf.b1 = hd->b1; hf.w2 = hd->w2; hf.b2 = hd->b2; hf.class_w = hd->class_w;
    hf.y_reg = (upstream ? hd->task != DRGNN_TASK_CLASS : hd->task == DRGNN_TASK_REG) ? (const float*)target : nullptr;
    hf.y_cls = (hd->task == DRGNN_TASK_CLASS) ? (const int64_t*)target : nullptr;
    hf.readout = readout; hf.step = step; hf.pred = pred; hf.partials = partials; hf.stage = 0;
}

extern "C" {

int drgnn_net_backward(const drgnn_net_desc* net, const float* x, const float* grad_readout,
                       const int32_t* ws_i32, const float* ws_f32, int64_t n_nodes, int64_t n_edges,
                       int64_t n_graphs, int32_t max_nodes, int32_t max_edges, int32_t max_c0,
                       const float* xp, const int32_t* arg0, const int32_t* arg1, float* grad_x,
                       float* partials, float* scratch_f32, int32_t* step_inc, void* stream_) {
    return net_backward_impl(net, x, grad_readout, nullptr, ws_i32, ws_f32, n_nodes, n_edges, n_graphs,
                             max_nodes, max_edges, max_c0, xp, arg0, arg1, grad_x, partials, scratch_f32,
                             step_inc, stream_);
}

int drgnn_net_backward_fused_head(const drgnn_net_desc* net, const drgnn_head_desc* hd, const float* x,
                                  const float* readout, const void* target, const int32_t* step,
                                  const int32_t* ws_i32, const float* ws_f32, int64_t n_nodes,
                                  int64_t n_edges, int64_t n_graphs, int32_t max_nodes, int32_t max_edges,
                                  int32_t max_c0, const float* xp, const int32_t* arg0, const int32_t* arg1,
                                  float* pred, float* head_partials, float* grad_x, float* partials,
                                  float* scratch_f32, const drgnn_topology_request* next_topology,
                                  void* stream_) {
    if (!hd || !hd->w1 || !hd->b1 || !hd->w2 || !hd->b2 || !readout || !target || !pred || !head_partials)
        return DRGNN_E_ARG;
    if (!net || hd->R != DRGNN_H2 * net->n_branch || hd->H < 1 || hd->H > 512 || hd->O < 1 || hd->O > DRGNN_MAX_OUT)
        return DRGNN_E_WIDTH;
    HeadFused hf;
    head_fused_fill(hf, hd, n_graphs, target, false, -1, 1, readout, step, pred, head_partials);
    return net_backward_impl(net, x, nullptr, &hf, ws_i32, ws_f32, n_nodes, n_edges, n_graphs, max_nodes,
                             max_edges, max_c0, xp, arg0, arg1, grad_x, partials, scratch_f32, nullptr, stream_,
                             next_topology);
}

// ---- fused training step ---------------------------------------------------------------------
static int64_t step_lds_bytes(int kind, int F, int capN, int capE, int capC, int R, int H, int O) {
    return 4 * step_scratch_words(kind, F, capN, capE, capC, R, H, O);
}

int64_t drgnn_net_step_lds_bytes(int32_t kind, int32_t n_feat, int32_t max_nodes, int32_t max_edges,
                                 int32_t max_c0, int32_t R, int32_t H, int32_t O) {
    if (max_nodes <= 0 || max_nodes > 32767 || max_edges > 65535 || n_feat > 256) return 0;   // else: the launch pair
    const StepCaps c = step_caps(max_nodes, max_edges, max_c0);
    return step_lds_bytes(kind, n_feat, c.N, c.E, c.C, R, H, O);
}

int64_t drgnn_head_compact_elems(int32_t R, int32_t H, int32_t O) { return head_compact_floats(R, H, O); }

// ---- launch plan of the fused step (include/drgnn.h: drgnn_step_plan) ---------------------------------------------------
// CUs this process may count on for co-residency of a launch's workgroups: the device's CU count, per device id (ADVICE r03:
// a process may drive devices of different sizes).  DRGNN_RESIDENT_CUS=<n> overrides it (a CU mask -- HSA_CU_MASK /
// ROC_GLOBAL_CU_MASK -- or a share of the GPU leaves fewer CUs than the attribute says); DRGNN_SHARED_GPU=1 means "assume
// nothing": every layout that waits for a partner workgroup is off (one workgroup per graph).
static int device_cu_count() {
#ifdef DRGNN_EMU      // (no device to ask)
    return 256;
#else
    static int cus[64];
    static int env_cus = -2;
    if (env_cus == -2) {
        const char* sh = getenv("DRGNN_SHARED_GPU");
        const char* lim = getenv("DRGNN_RESIDENT_CUS");
        env_cus = (sh && sh[0] == '1') ? 0 : (lim && atoi(lim) > 0) ? atoi(lim) : -1;
    }
    if (env_cus >= 0) return env_cus;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 1;      // unknown device: never assume co-residency
    if (cus[dev] == 0) {
        int n = 0;
        cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 1;
    }
    return cus[dev];
#endif
}
#ifndef DRGNN_EMU      // (the emulation has no device)
static int step_current_device() { int dev = 0; return hipGetDevice(&dev) == hipSuccess ? dev : 0; }
#endif

// the overrides of a plan (all 0 = automatic; no_paired is ignored).  DRGNN_STEP_PLAN=<one|two|noclass|product|nosplit>[,...]
// (read once) gives the defaults of a process for launches whose plan overrides nothing: same-box A/B runs of whole programs
struct StepOverrides { int force_wgs, no_class, no_aggregate, no_split; };
static StepOverrides step_env_overrides() {
    static int parsed = 0;
    static StepOverrides env = {0, 0, 0, 0};
    if (!parsed) {
        StepOverrides o = {0, 0, 0, 0};
        const char* v = getenv("DRGNN_STEP_PLAN");
        if (v) {
            if (strstr(v, "one")) o.force_wgs = 1;
            if (strstr(v, "two")) o.force_wgs = 2;
            if (strstr(v, "noclass")) o.no_class = 1;
            if (strstr(v, "product")) o.no_aggregate = 1;
            if (strstr(v, "nosplit")) o.no_split = 1;
        }
        env = o;
        parsed = 1;
    }
    return env;
}
// DRGNN_NO_PREFETCH (A/B runs): cached-topology launches without the next mini-batch's prefetch workgroups; read once
static bool step_no_prefetch() {
    static int v = -1;
    if (v < 0) v = getenv("DRGNN_NO_PREFETCH") != nullptr ? 1 : 0;
    return v != 0;
}
static StepOverrides step_overrides_of(const drgnn_step_plan* p) {
    if (p && (p->force_wgs || p->no_class || p->no_aggregate || p->no_split))
        return StepOverrides{p->force_wgs, p->no_class, p->no_aggregate, p->no_split};
    return step_env_overrides();
}

// padded feature width of the width-specialised kernels a launch of these bounds may take (16 / 32 / 48 / 64), 0 = generic.
// x == nullptr: alignment not judged here
static int step_variant(int kind, const float* x, int F, int capN, int capE, int capC, int H, int O) {
    if (!step_burst_guaranteed(kind, x, F, capN, capE, capC, H, O)) return 0;
    const int f16 = step_pad16(F);
    return (f16 == 16 || f16 == 32 || f16 == 48 || f16 == 64) ? f16 : 0;
}

// ... of the AGGREGATION-FIRST kernels: they read padded tile rows, so any feature count up to 64 has a width class; what
// remains of step_burst_guaranteed are the head width and the burst capacities
// from_memory: the form that reads the S rows of the tiles from memory (GINet, drgnn_step3.h SG): no register burst of the tile
static int step_af_width(int kind, int F, int capN, int capE, int capC, int H, int O, bool from_memory = false) {
    if (H != ((kind == DRGNN_GINET) ? 128 : 64) || F < 1 || F > 64) return 0;
    const int TF = (F + 3) & ~3;
    const bool ok = (F * DRGNN_H1 <= DRGNN_BCAP) && (from_memory || (long)capN * TF <= 16L * DRGNN_BCAP) && (capN + 1 <= DRGNN_BCAP) &&
                    (capE <= 2 * DRGNN_BCAP) && (capC * DRGNN_H1 <= 4 * DRGNN_BCAP) && O * H <= 2 * DRGNN_BCAP &&
                    H * 8 <= STEP_WB_J * DRGNN_BCAP;
    return ok ? step_pad16(F) : 0;
}

// what a launch is, as far as its layout goes
struct StepAsk {
    int kind, F, capN, capE, capC, R, H, O;
    int64_t B;
    int64_t co;             // graphs of the topology the launch co-builds (0: none, or not co-launchable)
    int co_roles;           // workgroups per graph that builder may take: 2 or 1
    bool train;
    bool x_ok;              // x is 16-byte aligned (or not known to be otherwise)
    int topo_flags;         // HIER / TILES (tiles usable) / LEAN of the workspace the launch reads
    int commit_wgs;         // single-branch nets: workgroups per graph the caller sized its buffers for (0: free choice)
    StepOverrides ov;
};
// SK_EMU: the host emulation's stand-in for the fused kernels (train_step_impl); the others: drgnn_step_af.h
enum { SK_EMU, SK_AF2, SK_AF3, SK_AF3B };
struct StepPick {
    int rc;                 // 0, or the error a launch of this shape returns (family NONE)
    int family, kernel, wgs, slabs, width, cls, lean_ok, builder_roles;
    int xg;                 // sGAT / FoutNet: 1 = the x-from-memory form (the S and the x tile together do not fit the LDS), 2 = S too
    int sg;                 // GINet, one workgroup per graph: the S-from-memory form (the S tile does not fit the LDS)
    int64_t lds, xchg_words;
    int capN, capE, capC;   // the LDS capacities the kernel is launched with (the class's when cls)
};
static const int64_t STEP_LDS_NEVER = (int64_t)1 << 50;

static StepPick step_pick(const StepAsk& q) {
    StepPick k;
    memset(&k, 0, sizeof(k));
    k.capN = q.capN; k.capE = q.capE; k.capC = q.capC;
    k.builder_roles = q.co > 0 ? q.co_roles : 0;
    k.slabs = (q.kind == DRGNN_GINET) ? 2 : 1;
    const int cus = device_cu_count();
    const int64_t co = q.co > 0 ? q.co : 0;
    auto two_ok = [&](int64_t extra) {
        if (q.ov.force_wgs == 1) return false;
        if (q.ov.force_wgs == 2) return true;
        return 2 * q.B + extra <= cus;
    };
    const int emu_width = q.x_ok ? step_variant(q.kind, nullptr, q.F, q.capN, q.capE, q.capC, q.H, q.O) : 0;
    // the aggregation-first family: a workspace with the hierarchical order and usable tiles, a width class, the reference head
#ifdef DRGNN_EMU      // (the emulation has no aggregation-first kernel: no shape qualifies)
    const bool af_shape = false;
    const int af_w = 0;
#else
    // (the single-branch nets read x rows next to the tiles: the input's when F % 4 == 0 -- 16-byte aligned then --, else the
    // tiles' padded copy; GINet reads the tiles only)
    int af_w = step_af_width(q.kind, q.F, q.capN, q.capE, q.capC, q.H, q.O);
    const bool af_ws = !q.ov.no_aggregate && (q.topo_flags & DRGNN_TOPO_HIER) && (q.topo_flags & DRGNN_TOPO_TILES);
    const bool af_shape = af_ws && af_w != 0 && (q.kind == DRGNN_GINET || (q.F & 3) != 0 || q.x_ok);
    // (the forms that leave the tiles' S rows in memory -- GINet's one-workgroup kernel, the 48- / 64-wide single-branch kernels:
    // graphs the staged forms have no LDS -- or no register burst -- for)
    const int sg_w = af_ws ? step_af_width(q.kind, q.F, q.capN, q.capE, q.capC, q.H, q.O, true) : 0;
#endif
    // A launch the aggregation-first kernels do not cover -- a head that is not the reference's, more than 64 features, a
    // workspace without the hierarchical order or usable tiles, the no_aggregate override -- is family NONE on the device: the
    // launch pair (drgnn_net_forward + drgnn_net_backward_fused_head) steps it.  The host emulation has none of those kernels:
    // it reports family PRODUCT for its stand-in (SK_EMU), bounded by the LDS of the retired product-first kernel.
#ifdef DRGNN_EMU      // (the LDS bound of the emulation's stand-in; the device never picks SK_EMU)
    const int64_t lemu = step_lds_bytes(q.kind, q.F, q.capN, q.capE, q.capC, q.R, q.H, q.O);
#else
    const int64_t lemu = STEP_LDS_NEVER;
#endif
    if (q.kind == DRGNN_GINET) {
        const bool narrow = q.H < DRGNN_H2;      // (the exchange words of a graph are 2 x 32 of its 2 x H: a narrower head runs one workgroup per graph)
        const int64_t l2af = af_shape ? 4 * step3_scratch_words(q.F, q.capN, q.capE, q.capC, q.H, q.O) : STEP_LDS_NEVER;
        int64_t l1af = af_shape ? 4 * step3b_scratch_words(q.F, q.capN, q.capE, q.capC, q.H, q.O) : STEP_LDS_NEVER;
#ifndef DRGNN_EMU      // (a from-memory form of the aggregation-first kernels)
        if (l1af > DRGNN_LDS_LIMIT && sg_w != 0) {
            const int64_t l1sg = 4 * step3b_scratch_words(q.F, q.capN, q.capE, q.capC, q.H, q.O, 1);
            if (l1sg <= DRGNN_LDS_LIMIT) { l1af = l1sg; k.sg = 1; af_w = sg_w; }
        }
#endif
        const bool af_two = l2af <= DRGNN_LDS_LIMIT, af_one = l1af <= DRGNN_LDS_LIMIT, emu_ok = lemu <= DRGNN_LDS_LIMIT;
        const bool can_two = !narrow && (af_two || emu_ok);
        const bool can_one = af_one || emu_ok;
        // two workgroups per graph only while every workgroup of the launch is resident -- with the builder at two
        // workgroups per graph if that fits, else at one; else one workgroup per graph; else two with the builder on its own
        int wgs = 0;
        if (can_two && two_ok(co * k.builder_roles)) wgs = 2;
        else if (can_two && k.builder_roles == 2 && two_ok(co)) { wgs = 2; k.builder_roles = 1; }
        else if (can_one) wgs = 1;
        else if (can_two && two_ok(0)) { wgs = 2; k.builder_roles = 0; }
        else { k.rc = DRGNN_E_CAPACITY; return k; }
        k.wgs = wgs;
        if (wgs == 2) { k.kernel = af_two ? SK_AF3 : SK_EMU; k.lds = af_two ? l2af : lemu; }
        else { k.kernel = af_one ? SK_AF3B : SK_EMU; k.lds = af_one ? l1af : lemu; }
        if (wgs == 2) k.sg = 0;      // (the S-from-memory form is the one-workgroup kernel's)
        k.xchg_words = 2 * (int64_t)(q.H > DRGNN_H2 ? q.H : DRGNN_H2);
    } else {
        int64_t laf = af_shape ? 4 * step2_scratch_words(q.kind, q.F, q.capN, q.capE, q.capC, q.H, q.O) : STEP_LDS_NEVER;
        if (af_shape && laf > DRGNN_LDS_LIMIT) {
            // graphs whose S and x tiles do not fit together (49 - 64 features at 200 nodes, 260+ nodes at the narrower widths):
            // the x rows stay in memory (drgnn_step2.h, XG)
            const int64_t lxg = 4 * step2_scratch_words(q.kind, q.F, q.capN, q.capE, q.capC, q.H, q.O, 1);
            if (lxg <= DRGNN_LDS_LIMIT) { laf = lxg; k.xg = 1; }
        }
#ifndef DRGNN_EMU      // (a from-memory form of the aggregation-first kernels)
        if (laf > DRGNN_LDS_LIMIT && sg_w >= 32 && ((q.F & 3) != 0 || q.x_ok)) {
            // ... and where the S tile alone is too much (the 32-, 48- and 64-wide kernels beyond 250 - 360 nodes): the S rows too
            const int64_t lxg = 4 * step2_scratch_words(q.kind, q.F, q.capN, q.capE, q.capC, q.H, q.O, 2);
            if (lxg <= DRGNN_LDS_LIMIT) { laf = lxg; k.xg = 2; af_w = sg_w; }
        }
#endif
        const bool af_ok = laf <= DRGNN_LDS_LIMIT;
        // the node-split layout: training launches of the aggregation-first kernels under GINet's residency rule
        int wgs = 1;
        // (training launches only.  Round 6 instantiated the split layout for inference launches too and measured it on the same
        // box, predict_epoch at batch 64: sGAT 14.8 us per mini-batch against 13.35 with one workgroup per graph (cached topology),
        // FoutNet 14.6 against 13.1 -- a forward alone is too short for its two hand-offs, profiles/r06_split_inference_ab.txt)
        const bool may_split = q.train && af_ok && !q.ov.no_split;
        if (q.commit_wgs == 2) {
            // the caller sized its buffers for two workgroups per graph: no silent fallback to another layout
            if (!may_split) { k.rc = DRGNN_E_CAPACITY; return k; }
            if (two_ok(co * k.builder_roles)) wgs = 2;
            else if (k.builder_roles == 2 && two_ok(co)) { wgs = 2; k.builder_roles = 1; }
            else if (two_ok(0)) { wgs = 2; k.builder_roles = 0; }
            else { k.rc = DRGNN_E_CAPACITY; return k; }
        } else if (q.commit_wgs == 0 && may_split) {
            // (a launch without a builder counts one idle CU per graph all the same: with every CU holding a half graph the
            // hand-offs cost more than the halved phases give and k_update sums twice the slabs -- cached topology at batch
            // 128, us per step, split / whole: sGAT 20.7 / 19.2, FoutNet 20.5 / 19.5; profiles/r05_batch_sweep.txt)
            if (co == 0) { if (two_ok(q.B)) wgs = 2; }
            else if (two_ok(co * k.builder_roles)) wgs = 2;
            else if (k.builder_roles == 2 && two_ok(co)) { wgs = 2; k.builder_roles = 1; }
        }
        k.wgs = wgs;
        if (af_ok) { k.kernel = SK_AF2; k.lds = laf; }
        else if (lemu <= DRGNN_LDS_LIMIT) { k.kernel = SK_EMU; k.lds = lemu; }
        else { k.rc = DRGNN_E_CAPACITY; return k; }
        k.slabs = wgs;
        k.xchg_words = (wgs == 2) ? step2_xchg_words(q.capC > 0 ? q.capC : 1) : 0;
    }
    // one round of workgroups instead of two: the builder at ONE workgroup per graph when that makes the launch resident
    // (measured, tools/r03_split_sweep.sh: sGAT at batch 128, 128 step + 256 builder workgroups = two rounds, 37.2 us per
    // step; 128 + 128 = one round, 29.0 us)
    if (k.builder_roles == 2 && k.wgs == 1 && q.B + 2 * co > cus && q.B + co <= cus) k.builder_roles = 1;
    k.lean_ok = (k.kernel != SK_EMU) ? 1 : 0;
    k.width = k.lean_ok ? af_w : emu_width;
    k.family = k.lean_ok ? DRGNN_STEP_FAMILY_AGGREGATE : DRGNN_STEP_FAMILY_PRODUCT;
    // Capacity class (drgnn_step.h: STEP_CLS_*): a batch whose maxima lie inside the class is stepped by the 32- or 48-wide
    // kernels whose LDS layout is a compile-time constant (the training and the inference instances; 48 features: the feature
    // count of the reference's shipped regression models)
#ifndef DRGNN_EMU      // (the capacity classes are instances of the aggregation-first kernels)
    if (!q.ov.no_class && !k.sg && !k.xg && (k.width == 32 || k.width == 48) && q.capN <= STEP_CLS_N && q.capE <= STEP_CLS_E &&
        q.capC <= STEP_CLS_C && step_af_width(q.kind, q.F, STEP_CLS_N, STEP_CLS_E, STEP_CLS_C, q.H, q.O) == k.width) {
        // (the 32-wide class instance of the one-workgroup kernel keeps Z1 / XP / dS per branch: STEP3B_DUAL)
        const int64_t lc = k.kernel == SK_AF3B ? 4 * (step3b_scratch_words(q.F, STEP_CLS_N, STEP_CLS_E, STEP_CLS_C, q.H, q.O) +
                                                      (STEP3B_DUAL(k.width, 1, q.train) ? step3b_dual_extra_words(STEP_CLS_N, STEP_CLS_C) : 0))
                         : k.kernel == SK_AF3 ? 4 * step3_scratch_words(q.F, STEP_CLS_N, STEP_CLS_E, STEP_CLS_C, q.H, q.O)
                                              : 4 * step2_scratch_words(q.kind, q.F, STEP_CLS_N, STEP_CLS_E, STEP_CLS_C, q.H, q.O);
        if (lc <= DRGNN_LDS_LIMIT) {
            k.cls = 1;
            k.capN = STEP_CLS_N; k.capE = STEP_CLS_E; k.capC = STEP_CLS_C;
            k.lds = lc;
        }
    }
#endif
    return k;
}

// sGAT / FoutNet: the from-memory level of the pick (1: x rows, 2: S rows too); GINet: 1 = its S-from-memory form
static int step_mem_level(int kind, const StepPick& k) { return kind == DRGNN_GINET ? (k.sg ? 1 : 0) : k.xg; }

// The shape of a launch and the overrides of its plan; the rest as for a launch that co-builds nothing, reads an aligned x and
// is free in its layout -- the callers fill in what they know better.
static StepAsk step_ask(int kind, int F, const StepCaps& c, int R, int H, int O, int64_t B, bool train, const drgnn_step_plan* plan) {
    StepAsk q;
    q.kind = kind; q.F = F; q.capN = c.N; q.capE = c.E; q.capC = c.C; q.R = R; q.H = H; q.O = O; q.B = B;
    q.co = 0; q.co_roles = 1; q.train = train; q.x_ok = true; q.topo_flags = 0; q.commit_wgs = 0;
    q.ov = step_overrides_of(plan);
    return q;
}

static bool step_bounds_ok(int32_t max_nodes, int32_t max_edges, int32_t n_feat) {
    return max_nodes > 0 && max_nodes <= 32767 && max_edges <= 65535 && n_feat <= 256;
}

int32_t drgnn_net_step_plan(drgnn_step_plan* p) {
    if (!p) return 0;
    p->family = DRGNN_STEP_FAMILY_NONE; p->wgs_per_graph = 0; p->slabs_per_graph = 0; p->width = 0; p->cls = 0; p->lean_ok = 0;
    p->builder_wgs_per_graph = 0; p->lds_bytes = 0; p->xchg_words = 0; p->from_memory = 0; p->reserved = 0;
    if (!step_bounds_ok(p->max_nodes, p->max_edges, p->n_feat) || p->n_graphs < 0 || p->H < 1 || p->H > 512 || p->O < 1 ||
        p->O > DRGNN_MAX_OUT || p->kind < 0 || p->kind > DRGNN_FOUT)
        return 0;
    StepAsk q = step_ask(p->kind, p->n_feat, step_caps(p->max_nodes, p->max_edges, p->max_c0), p->R, p->H, p->O, p->n_graphs,
                         p->train != 0, p);
    q.co = p->co_built_graphs > 0 ? p->co_built_graphs : 0;
    q.co_roles = (q.co > 0 && q.co <= DRGNN_TOPO_SPLIT_MAX_GRAPHS) ? 2 : 1;
    q.topo_flags = p->topo_flags;
    const StepPick k = step_pick(q);
    if (k.rc) return 0;
    p->family = k.family; p->wgs_per_graph = k.wgs; p->slabs_per_graph = k.slabs; p->width = k.width; p->cls = k.cls;
    p->lean_ok = k.lean_ok; p->builder_wgs_per_graph = k.builder_roles; p->lds_bytes = k.lds; p->xchg_words = k.xchg_words;
    p->from_memory = step_mem_level(p->kind, k) ? 1 : 0;
    return k.wgs;
}

int64_t drgnn_net_step_xchg_elems(int32_t kind, int32_t max_nodes, int32_t max_c0, int32_t H) {
    if (kind == DRGNN_GINET) return 2 * (int64_t)(H > DRGNN_H2 ? H : DRGNN_H2);
    const int capC = step_caps(max_nodes, 0, max_c0).C;
    return step2_xchg_words(capC > 0 ? capC : 1);
}

int32_t drgnn_net_step_variant(int32_t kind, const float* x, int32_t n_feat, int32_t max_nodes, int32_t max_edges,
                               int32_t max_c0, int32_t H, int32_t O) {
    const StepCaps c = step_caps(max_nodes, max_edges, max_c0);
    return step_variant(kind, x, n_feat, c.N, c.E, c.C, H, O);
}

#ifndef DRGNN_EMU      // (a runtime launch of the aggregation-first kernels)
// One launch of a step kernel instance (+ the co-launched builder's workgroups) with the argument array its caller built.  These
// kernels use up to the whole 160 KiB of LDS: the attribute is raised once per kernel instance and device (the call costs host
// time on every launch otherwise).
static int step_launch(const void* kern, void** args, int64_t lds_bytes, unsigned grid, hipStream_t stream) {
    if (lds_bytes > 64 * 1024) {
        struct Seen { const void* fn; int dev; };
        static Seen seen[256];
        static int n_seen = 0;
        const int dev = step_current_device();
        bool known = false;
        const int n = __atomic_load_n(&n_seen, __ATOMIC_ACQUIRE);
        for (int i = 0; i < n && !known; ++i) known = seen[i].fn == kern && seen[i].dev == dev;
        if (!known) {
            if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DRGNN_LDS_LIMIT) != hipSuccess) {
                (void)hipGetLastError();      // (profiling builds carry a static LDS word: ask for what this launch needs)
                HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
            } else {
                // (a cache, not state: a lost race only repeats the idempotent call above)
                const int slot = __atomic_fetch_add(&n_seen, 0, __ATOMIC_RELAXED);
                if (slot < 256) { seen[slot].fn = kern; seen[slot].dev = dev; __atomic_store_n(&n_seen, slot + 1, __ATOMIC_RELEASE); }
            }
        }
    }
    HIP_TRY(hipLaunchKernel(kern, dim3(grid), dim3(DRGNN_NTHREADS), args, (size_t)lds_bytes, stream));
    return 0;
}
#endif

// The operands of one fused step launch, as its entry point (drgnn_net_train_step, drgnn_net_train_step_cached,
// drgnn_ens_predict_cached, drgnn_cohort_train_step_cached) got them.
struct StepOperands {
    const drgnn_net_desc* net;
    const drgnn_head_desc* hd;
    const float* x;
    const void* target;
    int32_t* step2;
    const int32_t* ws_i32;
    const float* ws_f32;
    // n_graphs graphs of the launch; (n_nodes, n_edges, ws_graphs): the shape the workspace was laid out for (the mini-batch
    // itself, or a whole cached set whose graphs gather_ids[0..n_graphs) are stepped)
    int64_t n_nodes, n_edges, n_graphs, ws_graphs;
    const int32_t* gather_ids;
    int32_t max_nodes, max_edges, max_c0;
    float *pred, *readout, *head_partials, *partials;
    uint64_t* xchg;
    const drgnn_topology_request* next;
    const drgnn_step_hints* hints;
    void* stream;
    const drgnn_ens_member* ens;      // an ensemble launch: its member table and K
    int ens_K;
    const CohortStep* coh;            // a cohort launch
};
// ... of a launch on a cached set's workspace (the callers have checked cache, cache->x and cache->ws_i32)
static StepOperands step_operands_cached(const drgnn_net_desc* net, const drgnn_head_desc* hd, const drgnn_topology_cache* cache,
                                         const int32_t* ids, int64_t n_graphs, int32_t max_nodes, int32_t max_edges, int32_t max_c0,
                                         const drgnn_step_hints* hints, void* stream) {
    StepOperands s = {};
    s.net = net; s.hd = hd; s.x = cache->x; s.target = cache->y; s.ws_i32 = cache->ws_i32; s.ws_f32 = cache->ws_f32;
    s.n_nodes = cache->n_nodes; s.n_edges = cache->n_edges; s.n_graphs = n_graphs; s.ws_graphs = cache->n_graphs;
    s.gather_ids = ids; s.max_nodes = max_nodes; s.max_edges = max_edges; s.max_c0 = max_c0; s.hints = hints; s.stream = stream;
    return s;
}

static int step_check(const StepOperands& s) {
    const drgnn_net_desc* net = s.net;
    const drgnn_head_desc* hd = s.hd;
    const int rc = net_check(net);
    if (rc) return rc;
#ifdef DRGNN_EMU      // (what a member axis asks for: the emulation has neither launch)
    if (s.ens || s.coh) return DRGNN_E_CAPACITY;      // (the host emulation has no ensemble / cohort launch: their plans answer NONE)
#else
    // a cohort launch (drgnn_cohort_train_step_cached): the members' parameters, outputs, slabs and step words come from the
    // member table; what the checks below ask of a single model's are member 0's stand-ins
    if (s.coh && (s.coh->K < 1 || !s.coh->members || !s.coh->ids || !s.coh->counts || !hd || hd->train != 1 ||
                  hd->task == DRGNN_TASK_GRAD || hd->drop_mask || !(s.hints && s.hints->plan) || !s.target || s.ens))
        return DRGNN_E_ARG;
#endif
    if (s.ens && (s.ens_K < 1 || !s.gather_ids || hd->train || !(s.hints && s.hints->plan))) return DRGNN_E_ARG;
    if (!hd || !s.x || !s.ws_i32) return DRGNN_E_ARG;
    if (!s.coh && (!hd->w1 || !hd->b1 || !hd->w2 || !hd->b2 || !s.step2 || !s.pred || !s.readout)) return DRGNN_E_ARG;
    // hd->train: 1 = the whole step; 0 = inference; 2 = the forward of a training step (predictions only, dropout on)
    if (hd->train < 0 || hd->train > 2) return DRGNN_E_ARG;
    if (hd->train == 1 && !s.coh && (!s.target || !s.head_partials || !s.partials)) return DRGNN_E_ARG;      // inference needs neither
    if (hd->task != DRGNN_TASK_REG && hd->task != DRGNN_TASK_CLASS && hd->task != DRGNN_TASK_GRAD) return DRGNN_E_ARG;
    if (hd->task == DRGNN_TASK_GRAD && s.gather_ids) return DRGNN_E_ARG;      // (the upstream gradient is indexed by slot)
    if (net->n_branch > 1 && !s.xchg && !s.ens && !s.coh) return DRGNN_E_ARG;      // (the ensemble / cohort forms exchange nothing)
    if (net->kind == DRGNN_SGAT && !s.ws_f32) return DRGNN_E_ARG;
    if (hd->R != DRGNN_H2 * net->n_branch || hd->H < 1 || hd->H > 512 || hd->O < 1 || hd->O > DRGNN_MAX_OUT)
        return DRGNN_E_WIDTH;
    if (!step_bounds_ok(s.max_nodes, s.max_edges, net->n_feat)) return DRGNN_E_CAPACITY;
    return 0;
}

// the co-launched builder of the next mini-batch's topology
struct StepBuilder {
    TopoLaunch T;
    int64_t lds;
    bool ok;      // the request can share the step's launch
};
static int step_builder(const StepOperands& s, StepBuilder& b) {
    b.lds = 0; b.ok = false;
    if (!s.next) return 0;
    const int rc = topo_prepare_req(b.T, &b.lds, s.next);
    if (rc) return rc;
    const TopoLaunch& T = b.T;
    b.ok = T.capN > 0 && T.user_nptr != nullptr && !(T.args.cluster1 != nullptr && T.args.c1_ptr == nullptr) &&
           T.args.n_graphs > 0 && s.n_graphs > 0;
    // the builder inside a GINet / FoutNet step launch is compiled without the edge-weight path: a request that wants
    // weights (another kind's topology) gets a launch of its own
    if (s.net->kind != DRGNN_SGAT && T.args.edge_attr != nullptr && T.tv.w0 != nullptr) b.ok = false;
    return 0;
}

// the layout: one decision procedure (step_pick) for this launch and for drgnn_net_step_plan, and what the launch's plan and
// hints commit it to
static int step_layout(const StepOperands& s, StepBuilder& b, StepAsk& q, StepPick& k) {
    const drgnn_head_desc* hd = s.hd;
    const drgnn_step_hints* hints = s.hints;
    const drgnn_step_plan* plan = hints ? hints->plan : nullptr;
    const int kind = s.net->kind;
    q = step_ask(kind, s.net->n_feat, step_caps(s.max_nodes, s.max_edges, s.max_c0), hd->R, hd->H, hd->O, s.n_graphs, hd->train == 1, plan);
    q.co = b.ok ? (int64_t)b.T.args.n_graphs : 0;
    q.co_roles = b.ok ? b.T.roles : 1;
    q.x_ok = (((uintptr_t)s.x) & 15) == 0;
    q.topo_flags = hints ? hints->topo_flags : 0;
    // (the caller vouches for the tiles' flavour: weighted sums for sGAT, plain sums for FoutNet / GINet)
    if (!(hints && hints->tiles && ((((uintptr_t)hints->tiles) & 15) == 0))) q.topo_flags &= ~DRGNN_TOPO_TILES;
    q.commit_wgs = (kind == DRGNN_GINET) ? 0 : (plan && plan->wgs_per_graph == 2) ? 2 : 1;
    if (s.ens || s.coh) { q.ov.force_wgs = 1; q.commit_wgs = (kind == DRGNN_GINET) ? 0 : 1; }      // (the ensemble / cohort forms: one workgroup per graph)
    if (q.commit_wgs == 2 && !s.xchg) return DRGNN_E_CAPACITY;
    k = step_pick(q);
    if (k.rc) return k.rc;
    // a workspace built with DRGNN_TOPO_LEAN holds only what the aggregation-first kernels read
    if (hints && (hints->topo_flags & DRGNN_TOPO_LEAN) && !k.lean_ok) return DRGNN_E_ARG;
    // the autograd boundary (an upstream gradient instead of a target, a forward with the dropout mask of the step) is the
    // aggregation-first kernels' alone
    if ((hd->task == DRGNN_TASK_GRAD || hd->train == 2) && !k.lean_ok) return DRGNN_E_ARG;
    // a plan handed along with its `out` members filled (drgnn_net_step_plan) is a commitment: the launch takes the kernel
    // family, width class and slab layout the caller planned (and sized its buffers / made its assertions from) or fails --
    // never a silent third layout (a plan of another mode -- training against inference -- is only a carrier of overrides)
    if (plan && plan->family != DRGNN_STEP_FAMILY_NONE && (plan->train != 0) == q.train &&
        (plan->family != k.family || plan->width != k.width || plan->cls != k.cls || plan->slabs_per_graph != k.slabs))
        return DRGNN_E_CAPACITY;
    if (b.ok && k.builder_roles == 0) b.ok = false;      // the builder gets a launch of its own
    if ((s.ens || s.coh) && (k.wgs != 1 || (k.kernel != SK_AF3B && k.kernel != SK_AF2))) return DRGNN_E_CAPACITY;
    if (b.ok) b.T.roles = k.builder_roles;
    return 0;
}

// The table of the launch's graphs the host knows (drgnn_kernels.h: StepDims); count = 0 where it does not.
static int step_host_dims(const StepOperands& s, const StepAsk& q, StepDims& D) {
    const drgnn_step_hints* hints = s.hints;
    const int64_t n_graphs = s.n_graphs;
    D.count = 0;
    // host-known graph numbers of a cached-topology launch are range-checked whatever the batch size: the kernel reads the
    // set's tables at gather_ids[g] as is
    if (s.gather_ids && hints && hints->host_ids)
        for (int64_t g = 0; g < n_graphs; ++g)
            if (hints->host_ids[g] < 0 || hints->host_ids[g] >= s.ws_graphs) return DRGNN_E_ARG;
    if (!(hints && n_graphs > 0 && n_graphs <= DRGNN_STEP_DIMS_MAX)) return 0;
    bool ok = true;
    if (!s.gather_ids && hints->host_node_ptr && hints->host_edge_ptr) {
        for (int g = 0; g < (int)n_graphs; ++g) {
            D.n0[g] = hints->host_node_ptr[g]; D.n[g] = hints->host_node_ptr[g + 1] - hints->host_node_ptr[g];
            D.e0[g] = hints->host_edge_ptr[g]; D.e[g] = hints->host_edge_ptr[g + 1] - hints->host_edge_ptr[g];
            D.gi[g] = g;
            ok = ok && D.n[g] >= 0 && D.e[g] >= 0 && D.n[g] <= q.capN && D.e[g] <= q.capE;
        }
        if (ok && (hints->host_node_ptr[n_graphs] != s.n_nodes || hints->host_edge_ptr[n_graphs] != s.n_edges)) ok = false;
    } else if (s.gather_ids && hints->host_ids && hints->set_node_ptr && hints->set_edge_ptr) {
        for (int g = 0; g < (int)n_graphs; ++g) {
            const int64_t id = hints->host_ids[g];
            if (id < 0 || id >= s.ws_graphs) { ok = false; break; }
            D.n0[g] = (int32_t)hints->set_node_ptr[id]; D.n[g] = (int32_t)(hints->set_node_ptr[id + 1] - hints->set_node_ptr[id]);
            D.e0[g] = (int32_t)hints->set_edge_ptr[id]; D.e[g] = (int32_t)(hints->set_edge_ptr[id + 1] - hints->set_edge_ptr[id]);
            D.gi[g] = (int32_t)id;
            ok = ok && D.n[g] <= q.capN && D.e[g] <= q.capE;
        }
    } else {
        ok = false;
    }
    if (ok) D.count = (int)n_graphs;       // (a table that contradicts the capacities is ignored: the device path decides)
    return 0;
}

static void step_args(const StepOperands& s, const StepAsk& q, StepArgs& a) {
    TopoLayout lay;
    topo_layout(s.n_nodes, s.n_edges, s.ws_graphs, &lay);
    a.gather_ids = s.gather_ids; a.ws_graphs = (int)s.ws_graphs;
    a.tiles = (q.topo_flags & DRGNN_TOPO_TILES) ? s.hints->tiles : nullptr; a.tile_nodes = s.n_nodes;
    a.net = *s.net; a.x = s.x;
    a.tv = topo_view(const_cast<int32_t*>(s.ws_i32), const_cast<float*>(s.ws_f32), lay);
    a.n_nodes = s.n_nodes; a.n_graphs = (int)s.n_graphs;
    a.partials = s.partials; a.n_partial = (int)net_partial_floats(q.F);
    a.xchg = (unsigned long long*)s.xchg; a.step2 = s.step2;
    a.xchg_stride = (int)step2_xchg_words(q.capC > 0 ? q.capC : 1);
    head_fused_fill(a.hf, s.hd, s.n_graphs, s.target, true, 0, q.train ? 1 : 0, s.readout, s.step2, s.pred, s.head_partials);
}

#ifndef DRGNN_EMU      // (the launch of the aggregation-first kernels: emu_step stands in for it)
// What shares the grid with the step's workgroups: the builder's, or the next mini-batch's prefetchers.  Returns their number;
// *lds: the launch's dynamic LDS.
static int step_co_setup(const StepOperands& s, const StepBuilder& b, const StepPick& k, int blocks, StepCoLaunch& C, int64_t* lds) {
    const drgnn_step_hints* hints = s.hints;
    const StepArgs& a = C.step.a;
    *lds = k.lds;
    C.topo.pf_ids = nullptr; C.topo.pf_n = 0; C.topo.pf_graphs = 0;
    if (b.ok) {
        C.topo = b.T;
        if (b.lds > *lds) *lds = b.lds;
        return b.T.args.n_graphs * b.T.roles;
    }
    // (an ensemble / cohort kernel runs its own workgroups only)
    if (s.ens || s.coh || !s.gather_ids || !(hints && hints->next_ids && hints->n_next > 0) || (blocks % 8) != 0 ||
        blocks + hints->n_next > device_cu_count() || step_no_prefetch() || a.tiles == nullptr)
        return 0;
    // cached topology, CUs to spare: one extra workgroup per graph of the NEXT mini-batch warms the L2 of the XCD that
    // will step it (prefetch_block; beyond the resident size the workgroups would only queue behind the step's)
    const int kind = a.net.kind, F = a.net.n_feat, TF = (F + 3) & ~3;
    TopoLaunch& Q = C.topo;
    memset(&Q, 0, sizeof(Q));
    Q.tv = a.tv;
    Q.pf_ids = hints->next_ids; Q.pf_n = (int)hints->n_next; Q.pf_graphs = a.ws_graphs;
    Q.pf_tiles = a.tiles; Q.pf_f = TF; Q.pf_tile_nodes = s.n_nodes;
    Q.pf_x = (kind == DRGNN_GINET) ? nullptr : (F & 3) ? a.tiles + drgnn_tiles_x_off(s.n_nodes, TF) : s.x;
    Q.pf_coef = (kind != DRGNN_GINET) ? 1 : 0;
    Q.pf_y = s.hd->train == 1 ? s.target : nullptr; Q.pf_y_bytes = (s.hd->task == DRGNN_TASK_REG) ? 4 : 8;
    return Q.pf_n;
}

// the kernel instance of the pick (drgnn_step_af.h) and its launch, each form with its own argument array
static int step_run(const StepOperands& s, const StepPick& k, const StepCoLaunch& C, int64_t lds, unsigned grid) {
    if (k.kernel == SK_EMU) return DRGNN_E_CAPACITY;      // (the host emulation's; step_pick never picks it here)
    AfKey key;
    key.kind = s.net->kind; key.width = k.width; key.wgs = k.wgs; key.level = step_mem_level(key.kind, k); key.cls = k.cls;
    key.gather = s.gather_ids != nullptr; key.train = s.hd->train == 1;
    key.axis = s.ens ? AF_AXIS_ENS : s.coh ? AF_AXIS_COHORT : AF_AXIS_NONE;
    const void* kern = af_kernel(key);
    if (!kern) return key.axis == AF_AXIS_NONE ? DRGNN_E_ARG : DRGNN_E_CAPACITY;
    void* c = const_cast<StepCoLaunch*>(&C);
    if (s.ens) {
        const drgnn_ens_member* members = s.ens;
        int K = s.ens_K;
        void* args[] = {c, &members, &K};
        return step_launch(kern, args, lds, grid, (hipStream_t)s.stream);
    }
    if (s.coh) {
        void* args[] = {c, const_cast<CohortStep*>(s.coh)};
        return step_launch(kern, args, lds, grid, (hipStream_t)s.stream);
    }
    void* args[] = {c};
    return step_launch(kern, args, lds, grid, (hipStream_t)s.stream);
}
#endif

static int train_step_impl(const StepOperands& s) {
    int rc = step_check(s);
    if (rc) return rc;
    StepBuilder b;
    if ((rc = step_builder(s, b))) return rc;
    StepAsk q;
    StepPick k;
    if ((rc = step_layout(s, b, q, k))) return rc;
#ifdef DRGNN_EMU      // (the emulation's stand-in steps the graphs itself: no co-launch record)
    StepLaunch L;
#else
    StepCoLaunch C;
    StepLaunch& L = C.step;
#endif
    L.capN = k.capN; L.capE = k.capE; L.capC = k.capC;
    L.words = k.lds / 4;
    if ((rc = step_host_dims(s, q, L.dims))) return rc;
    step_args(s, q, L.a);
    // grid of the step part: graphs in groups of 8 x 2 when a graph has two workgroups (step2_block, step3_block)
    // (ensemble / cohort: graphs in groups of 8 x K, see ens_slot)
    const int64_t n_graphs = s.n_graphs;
    const int multi_K = s.ens ? s.ens_K : s.coh ? s.coh->K : 0;
    const int blocks = multi_K ? (int)((n_graphs + 7) / 8) * 8 * multi_K : (k.wgs == 2) ? (int)((n_graphs + 7) / 8) * 16 : (int)n_graphs;
    if (blocks > 0) {
#ifdef DRGNN_EMU      // emu_step (above) in place of the aggregation-first kernels, then the co-built topology as a launch of its own
        if (q.kind == DRGNN_GINET) emu_step<DRGNN_GINET>(L.a, q.train, k.capN, k.capE, k.capC);
        else if (q.kind == DRGNN_SGAT) emu_step<DRGNN_SGAT>(L.a, q.train, k.capN, k.capE, k.capC);
        else emu_step<DRGNN_FOUT>(L.a, q.train, k.capN, k.capE, k.capC);
        if (b.ok && (rc = topo_launch(b.T, b.lds, s.stream))) return rc;
#else
        C.n_net = blocks;
        int64_t lds = 0;
        const int extra = step_co_setup(s, b, k, blocks, C, &lds);
        if ((rc = step_run(s, k, C, lds, (unsigned)(blocks + extra)))) return rc;
#endif
    }
    if (s.next && (!b.ok || blocks == 0))
        return drgnn_topology_build_request(s.next, s.stream);
    return 0;
}

int drgnn_net_train_step(const drgnn_net_desc* net, const drgnn_head_desc* hd, const float* x,
                         const void* target, int32_t* step2, const int32_t* ws_i32, const float* ws_f32,
                         int64_t n_nodes, int64_t n_edges, int64_t n_graphs, int32_t max_nodes,
                         int32_t max_edges, int32_t max_c0, float* pred, float* readout,
                         float* head_partials, float* partials, uint64_t* xchg,
                         const drgnn_topology_request* next, const drgnn_step_hints* hints, void* stream_) {
    StepOperands s = {};
    s.net = net; s.hd = hd; s.x = x; s.target = target; s.step2 = step2; s.ws_i32 = ws_i32; s.ws_f32 = ws_f32;
    s.n_nodes = n_nodes; s.n_edges = n_edges; s.n_graphs = n_graphs; s.ws_graphs = n_graphs;
    s.max_nodes = max_nodes; s.max_edges = max_edges; s.max_c0 = max_c0;
    s.pred = pred; s.readout = readout; s.head_partials = head_partials; s.partials = partials; s.xchg = xchg;
    s.next = next; s.hints = hints; s.stream = stream_;
    return train_step_impl(s);
}

int drgnn_net_train_step_cached(const drgnn_net_desc* net, const drgnn_head_desc* hd,
                                const drgnn_topology_cache* cache, const int32_t* ids, int64_t n_graphs,
                                int32_t max_nodes, int32_t max_edges, int32_t max_c0, int32_t* step2, float* pred,
                                float* readout, float* head_partials, float* partials, uint64_t* xchg,
                                const drgnn_step_hints* hints, void* stream_) {
    if (!cache || !ids || !cache->ws_i32 || !cache->x || n_graphs < 0 || n_graphs > cache->n_graphs) return DRGNN_E_ARG;
    if (hd && hd->train == 1) {
        if (!cache->y || cache->y_bytes != (hd->task == DRGNN_TASK_REG ? 4 : 8)) return DRGNN_E_ARG;
    }
    StepOperands s = step_operands_cached(net, hd, cache, ids, n_graphs, max_nodes, max_edges, max_c0, hints, stream_);
    s.step2 = step2; s.pred = pred; s.readout = readout; s.head_partials = head_partials; s.partials = partials; s.xchg = xchg;
    return train_step_impl(s);
}

// the plan of a launch with a member axis (K models / members): the one-workgroup-per-graph forms, where no workgroup of the
// launch waits for another
static int32_t member_step_plan(drgnn_step_plan* p, int32_t K, int32_t max_K, int32_t train) {
    if (!p) return 0;
    p->train = train;
    p->force_wgs = 1;
    p->co_built_graphs = 0;
    const int32_t wgs = drgnn_net_step_plan(p);
#ifdef DRGNN_EMU      // (the emulation has no launch with a member axis)
    (void)K; (void)max_K; (void)wgs;
    p->family = DRGNN_STEP_FAMILY_NONE;
    return 0;
#else
    if (K < 1 || K > max_K || wgs != 1 || p->family != DRGNN_STEP_FAMILY_AGGREGATE || p->lds_bytes <= 0 ||
        p->lds_bytes > DRGNN_LDS_LIMIT || (int64_t)K * ((p->n_graphs + 7) / 8) * 8 > (int64_t)INT32_MAX) {
        p->family = DRGNN_STEP_FAMILY_NONE;
        return 0;
    }
    return 1;
#endif
}

int32_t drgnn_ens_step_plan(drgnn_step_plan* p, int32_t K) { return member_step_plan(p, K, INT32_MAX, 0); }

int drgnn_ens_predict_cached(const drgnn_net_desc* net, const drgnn_head_desc* hd, const drgnn_ens_member* members,
                             int32_t K, const drgnn_topology_cache* cache, const int32_t* ids, int64_t n_graphs,
                             int32_t max_nodes, int32_t max_edges, int32_t max_c0, int32_t* step2, float* pred,
                             float* readout, const drgnn_step_hints* hints, void* stream_) {
    if (!members || K < 1 || !hd || hd->train || !pred || !readout) return DRGNN_E_ARG;
    if (!cache || !ids || !cache->ws_i32 || !cache->x || n_graphs < 0 || n_graphs > cache->n_graphs) return DRGNN_E_ARG;
    StepOperands s = step_operands_cached(net, hd, cache, ids, n_graphs, max_nodes, max_edges, max_c0, hints, stream_);
    s.step2 = step2; s.pred = pred; s.readout = readout; s.ens = members; s.ens_K = K;
    return train_step_impl(s);
}

int32_t drgnn_cohort_step_plan(drgnn_step_plan* p, int32_t K) { return member_step_plan(p, K, 65535, 1); }

int drgnn_cohort_train_step_cached(const drgnn_net_desc* net, const drgnn_head_desc* hd, const drgnn_cohort_member* members,
                                   int32_t K, const drgnn_topology_cache* cache, const int32_t* ids, const int32_t* counts,
                                   int64_t ids_stride, int64_t n_graphs, int32_t max_nodes, int32_t max_edges, int32_t max_c0,
                                   const drgnn_step_hints* hints, void* stream_) {
    if (!members || K < 1 || K > 65535 || !hd || hd->train != 1 || !ids || !counts || ids_stride < n_graphs) return DRGNN_E_ARG;
    if (!cache || !cache->ws_i32 || !cache->x || n_graphs < 0 || n_graphs > cache->n_graphs) return DRGNN_E_ARG;
    if (!cache->y || cache->y_bytes != (hd->task == DRGNN_TASK_REG ? 4 : 8)) return DRGNN_E_ARG;
#ifdef DRGNN_EMU      // (no cohort launch in the emulation)
    (void)net; (void)max_nodes; (void)max_edges; (void)max_c0; (void)hints; (void)stream_;
    return DRGNN_E_CAPACITY;      // (the host emulation has no cohort launch: drgnn_cohort_step_plan answers NONE)
#else
    CohortStep coh;
    coh.members = members; coh.ids = ids; coh.counts = counts; coh.K = K; coh.stride = ids_stride;
    StepOperands s = step_operands_cached(net, hd, cache, ids, n_graphs, max_nodes, max_edges, max_c0, hints, stream_);
    s.coh = &coh;
    return train_step_impl(s);
#endif
}

// ---- dense head + loss + optimiser ----------------------------------------------------------
int64_t drgnn_head_partial_elems(int32_t R, int32_t H, int32_t O) { return head_partial_floats(R, H, O); }
int64_t drgnn_head_num_slabs(int64_t n_graphs) { const int t = head_tile(n_graphs); return (n_graphs + t - 1) / t; }

// hidden units k_head stages at a time for T graphs per workgroup: all H, or for inference the largest multiple of 16 that
// fits LDS (the passes of head_block); 0: none does
static int head_chunk(const drgnn_head_desc* hd, int T) {
    if (4 * head_lds_words(hd->R, hd->H, hd->O, T) <= DRGNN_LDS_LIMIT) return hd->H;
    if (hd->train) return 0;
    for (int hc = (hd->H - 1) / 16 * 16; hc >= 16; hc -= 16)
        if (4 * head_lds_words(hd->R, hc, hd->O, T) <= DRGNN_LDS_LIMIT) return hc;
    return 0;
}

int32_t drgnn_head_pass_units(int32_t R, int32_t H, int32_t O, int64_t n_graphs) {
    drgnn_head_desc hd = {};
    hd.R = R; hd.H = H; hd.O = O; hd.train = 0;
    if (R < 1 || H < 1 || O < 1 || O > DRGNN_MAX_OUT) return 0;
    return head_chunk(&hd, head_tile(n_graphs));
}
int64_t drgnn_net_head_stage_bytes(int32_t R, int32_t H, int32_t O) { return 4 * head_stage_words(R, H, O); }

static int head_check(const drgnn_head_desc* hd) {
    if (!hd || !hd->w1 || !hd->b1 || !hd->w2 || !hd->b2) return DRGNN_E_ARG;
    if (hd->R < 1 || hd->H < 1 || hd->O < 1 || hd->O > DRGNN_MAX_OUT) return DRGNN_E_WIDTH;
    // (a training head is staged whole, whatever the batch size; an inference launch takes a wider one in passes)
    if (head_chunk(hd, DRGNN_HEAD_TILE_LARGE) == 0) return DRGNN_E_WIDTH;
    if (hd->task != DRGNN_TASK_REG && hd->task != DRGNN_TASK_CLASS) return DRGNN_E_ARG;
    if (!(hd->p_drop >= 0.0f && hd->p_drop < 1.0f)) return DRGNN_E_ARG;
    return 0;
}

int drgnn_head_step(const drgnn_head_desc* hd, const float* readout, const void* target,
                    int64_t n_graphs, const int32_t* step, float* pred, float* grad_readout,
                    float* partials, void* stream) {
    int rc = head_check(hd);
    if (rc) return rc;
    if (!readout || !pred || n_graphs < 0) return DRGNN_E_ARG;
    if (hd->train && (!target || !grad_readout || !partials)) return DRGNN_E_ARG;
    if (n_graphs == 0) return 0;
    HeadArgs a;
    a.readout = readout;
    a.y_reg = (hd->task == DRGNN_TASK_REG) ? (const float*)target : nullptr;
    a.y_cls = (hd->task == DRGNN_TASK_CLASS) ? (const int64_t*)target : nullptr;
    a.class_w = hd->class_w;
    a.w1 = hd->w1; a.b1 = hd->b1; a.w2 = hd->w2; a.b2 = hd->b2;
    a.step = step; a.pred = pred; a.grad_readout = hd->train ? grad_readout : nullptr;
    a.partials = partials;
    a.B = (int)n_graphs; a.R = hd->R; a.H = hd->H; a.O = hd->O;
    a.task = hd->task; a.train = hd->train; a.p_drop = hd->p_drop; a.seed = hd->seed; a.sigmoid = hd->transform_sigmoid;
    a.T = head_tile(n_graphs);
    a.HC = head_chunk(hd, a.T);
    const int blocks = (int)((n_graphs + a.T - 1) / a.T);
    const int64_t lds = 4 * head_lds_words(hd->R, a.HC, hd->O, a.T);
    DRGNN_EMU_ONLY(std::vector<float> buf((size_t)(lds / 4) + 16);)
    DRGNN_LAUNCH(k_head, grid1(blocks, DRGNN_NTHREADS, lds), stream, head_block(a, (int)bx, buf.data()), a);
    return 0;
}

int drgnn_head_reduce(const float* partials, int64_t n_graphs, int32_t R, int32_t H, int32_t O,
                      float* grad_block, float* loss, int32_t* step, void* stream) {
    if (!partials || !grad_block) return DRGNN_E_ARG;
    HeadReduceArgs a;
    a.partials = partials;
    a.n_wg = (int)((n_graphs + head_tile(n_graphs) - 1) / head_tile(n_graphs));
    a.P = (int)head_partial_floats(R, H, O);
    a.grad = grad_block; a.loss = loss; a.step = step;
    DRGNN_LAUNCH(k_head_reduce, grid_items(a.P - 1), stream, head_reduce_item(a, (int)bx), a);
    return 0;
}

int drgnn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                    const int32_t* step, int64_t n, double lr, double beta1, double beta2, double eps,
                    double weight_decay, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step || n < 0) return DRGNN_E_ARG;
    if (n == 0) return 0;
    AdamArgs a;
    a.param = param; a.grad = grad; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq; a.step = step; a.n = n;
    adam_set_hyper(a, lr, beta1, beta2, eps, weight_decay);
    DRGNN_LAUNCH(k_adam, grid_items(n), stream, adam_item(a, bx), a);
    return 0;
}

}  // extern "C"

// ---- the options of drgnn_optim ------------------------------------------------------------------------------------
static int optim_check(const drgnn_optim* o) {
    if (!o) return DRGNN_E_ARG;
    if (o->lr_n < 0 || (o->lr_n > 0 && !o->lr_table)) return DRGNN_E_ARG;
    if (o->n_dead < 0 || o->n_dead > DRGNN_ZERO_RANGES) return DRGNN_E_ARG;
    for (int r = 0; r < o->n_dead; ++r) if (o->dead_off[r] < 0 || o->dead_len[r] < 0) return DRGNN_E_ARG;
    if (o->clip && (!o->norm_words || o->norm_cap < 1)) return DRGNN_E_ARG;
    return 0;
}
// coupled L2 is the flat kernel's alone (drgnn_adam_step): the update launches then only leave the gradient
static bool optim_coupled(const drgnn_optim* o) { return !o->decoupled && o->weight_decay != 0.0; }
static void optim_adam_args(AdamArgs& a, const drgnn_optim* o) {
    adam_set_hyper(a, o->lr, o->beta1, o->beta2, o->eps, optim_coupled(o) ? o->weight_decay : 0.0);
}
// the Adam launch of the flat route; n_words > 0: norm_words[0, n_words) already hold the per-block sums of this gradient
static int adam_opt_impl(AdamArgs a, float* grad, const drgnn_optim* o, int n_words, void* stream_) {
    if (a.n == 0) return 0;
    const int64_t flat_words = (a.n + 255) / 256;
    if (o->clip && n_words == 0 && flat_words > o->norm_cap) return DRGNN_E_CAPACITY;
#ifdef DRGNN_EMU      // (another algorithm: the emulation forms Adam's scalars and the norm once and loops over the items)
    AdamOptScalars sc;
    adam_bias_scalars<true>(a, sc.step_size, sc.sqrt_bc2, o, &sc.decay);
    sc.clip = 1.0f;
    if (o->clip) {
        if (n_words == 0) {
            for (int64_t w = 0; w < flat_words; ++w) o->norm_words[w] = adam_norm_word(*o, grad, a.n, w * 256);
            n_words = (int)flat_words;
        }
        double norm;
        sc.clip = adam_clip_scale(*o, n_words, &norm);
        if (o->norm_out) o->norm_out[0] = (float)norm;
    }
    for (int64_t i = 0; i < a.n; ++i) adam_opt_item(a, *o, grad, i, sc);
    (void)stream_;
#else
    if (o->clip && n_words == 0) {
        hipLaunchKernelGGL(k_grad_norm_words, dim3((unsigned)flat_words), dim3(256), 0, (hipStream_t)stream_, grad, a.n, *o);
        HIP_TRY(hipGetLastError());
        n_words = (int)flat_words;
    }
    hipLaunchKernelGGL(k_adam_opt, dim3((unsigned)flat_words), dim3(256), 0, (hipStream_t)stream_, a, *o, grad, n_words);
    HIP_TRY(hipGetLastError());
#endif
    return 0;
}

extern "C" {

int64_t drgnn_optim_norm_words(int64_t n_param) {
    // update blocks: 64 gradient elements each, a branch's and the head's last block partly filled, slots of the conv partials
    // that are no parameter (at most as many again); flat route: one word per 256 elements
    return n_param < 0 ? (int64_t)DRGNN_E_ARG : n_param / 16 + 64;
}

int drgnn_adam_step_opt(float* param, float* grad, float* exp_avg, float* exp_avg_sq, const int32_t* step, int64_t n,
                        const drgnn_optim* optim, void* stream_) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step || n < 0) return DRGNN_E_ARG;
    const int rc = optim_check(optim);
    if (rc) return rc;
    AdamArgs a;
    a.param = param; a.grad = grad; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq; a.step = step; a.n = n;
    optim_adam_args(a, optim);
    return adam_opt_impl(a, grad, optim, 0, stream_);
}

}  // extern "C"

extern "C" {

int64_t drgnn_p2p_bytes(int64_t n_floats) { return n_floats < 0 ? (int64_t)DRGNN_E_ARG : p2p_bytes(n_floats); }

int drgnn_p2p_alloc(int64_t bytes, void** dev_ptr, void* handle) {
    if (bytes <= 0 || !dev_ptr) return DRGNN_E_ARG;
#ifdef DRGNN_EMU      // (device memory and its IPC handle; the emulation: host memory, the pointer as the handle)
    *dev_ptr = calloc(1, (size_t)bytes);
    if (handle) { memset(handle, 0, 64); memcpy(handle, dev_ptr, sizeof(void*)); }     // same-process "handle"
    return *dev_ptr ? 0 : DRGNN_E_CAPACITY;
#else
    // fine-grained: coherent across devices WITHIN a kernel (coarse-grained memory is only coherent at launch boundaries)
    HIP_TRY(hipExtMallocWithFlags(dev_ptr, (size_t)bytes, hipDeviceMallocFinegrained));
    HIP_TRY(hipMemset(*dev_ptr, 0, (size_t)bytes));
    HIP_TRY(hipDeviceSynchronize());
    if (handle) {
        static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
        HIP_TRY(hipIpcGetMemHandle((hipIpcMemHandle_t*)handle, *dev_ptr));
    }
    return 0;
#endif
}

int drgnn_p2p_open(const void* handle, void** dev_ptr) {
    if (!handle || !dev_ptr) return DRGNN_E_ARG;
#ifdef DRGNN_EMU      // (as drgnn_p2p_alloc)
    memcpy(dev_ptr, handle, sizeof(void*));
    return 0;
#else
    const hipIpcMemHandle_t h = *(const hipIpcMemHandle_t*)handle;
    HIP_TRY(hipIpcOpenMemHandle(dev_ptr, h, hipIpcMemLazyEnablePeerAccess));
    return 0;
#endif
}

int drgnn_p2p_close(void* dev_ptr) {
#ifdef DRGNN_EMU      // (as drgnn_p2p_alloc)
    (void)dev_ptr;
    return 0;
#else
    if (!dev_ptr) return DRGNN_E_ARG;
    HIP_TRY(hipIpcCloseMemHandle(dev_ptr));
    return 0;
#endif
}

int drgnn_p2p_free(void* dev_ptr) {
#ifdef DRGNN_EMU      // (as drgnn_p2p_alloc)
    free(dev_ptr);
    return 0;
#else
    if (!dev_ptr) return DRGNN_E_ARG;
    HIP_TRY(hipFree(dev_ptr));
    return 0;
#endif
}

int drgnn_allreduce_oneshot(float* grad, int64_t n, void* const* peer_bufs, int32_t world, int32_t rank, float weight,
                            uint32_t* seq, int32_t* status, int32_t part, void* stream) {
    if (!grad || n < 0 || !peer_bufs || world < 1 || world > DRGNN_P2P_MAX || rank < 0 || rank >= world || !seq || !status ||
        part < 0 || part > 2)
        return DRGNN_E_ARG;
    if (n == 0) return 0;
    P2PArgs a;
    a.grad = grad; a.n = n; a.world = world; a.rank = rank; a.weight = weight; a.seq = seq; a.status = status; a.part = part;
    for (int r = 0; r < DRGNN_P2P_MAX; ++r) a.peer[r] = (r < world) ? (float*)peer_bufs[r] : nullptr;
    for (int r = 0; r < world; ++r) if (!a.peer[r]) return DRGNN_E_ARG;
    DRGNN_LAUNCH(k_allreduce_oneshot, grid1(DRGNN_P2P_WGS, DRGNN_P2P_THREADS), stream, p2p_block(a, (int)bx), a);
    return 0;
}

}  // extern "C"

// ---- the update launches: the slabs' fixed-order sums, dW_fc1, Adam, the step word ---------------------------------------------
// Where a call's sums go.  compact: the head slabs are the fused step's, [head_slabs][head_compact_floats] + readout
// [head_slabs][R], and dW_fc1 is formed here; otherwise the launch pair's [head_slabs][head_partial_floats] with dW_fc1 inside.
struct UpdateDst { const drgnn_net_desc* net; drgnn_conv_grads* g_conv1; drgnn_conv_grads* g_conv2; int32_t R, H, O; bool compact; };
// What they read.  slabs_per_graph: conv slabs per graph, 0 = n_branch; 2: the split layout of a single-branch net (drgnn_step2.h)
struct UpdateSlabs {
    const float* conv_partials; int64_t n_graphs; const float* head_partials; int64_t head_slabs; const float* readout;
    int32_t slabs_per_graph;
};
struct UpdateFlat { float* param; float* grad; float* exp_avg; float* exp_avg_sq; int64_t n_param, head_offset; };
// One update call (zero-initialised by update_call).  A cohort call (its slabs are the fused step's: compact) takes the slabs, flat
// buffers, step words and Adam's scalars of every member from the member table: `slabs` and the buffers of `flat` stay empty.
struct UpdateCall {
    UpdateDst dst; UpdateSlabs slabs; UpdateFlat flat;      // (flat.head_offset: of the head's gradient block in the flat gradient)
    const int32_t* step;               // legacy layout: the step word Adam reads
    int32_t* step2;                    // compact layout: the 2-word counter of drgnn_net_train_step, Adam reads [1], [0] is committed
    float* loss; float* loss2;         // the batch loss and its optional second destination (cohort: loss2 = losses [K])
    double lr, beta1, beta2, eps;      // Adam's scalars, or the record(s) of an _opt form: optim, a cohort's optims
    const drgnn_optim* optim; bool options;      // (options: an _opt form, the record(s) must be given)
    bool cohort; const drgnn_cohort_member* members; const drgnn_optim* optims; const int32_t* counts; int32_t K, any_clip;
    int32_t apply_adam; void* stream;
};
static UpdateCall update_call(const UpdateDst& dst, const UpdateSlabs& slabs, const UpdateFlat& flat, float* loss, int32_t apply_adam,
                              void* stream) {
    UpdateCall c = {};
    c.dst = dst; c.slabs = slabs; c.flat = flat; c.loss = loss; c.apply_adam = apply_adam; c.stream = stream;
    return c;
}
// (a single-branch net's two half-graph slabs are two more "graphs" to the fixed-order sum)
static bool slabs_split(const drgnn_net_desc* net, int32_t slabs_per_graph) { return net->n_branch == 1 && slabs_per_graph == 2; }
static int slabs_check(const drgnn_net_desc* net, int32_t slabs_per_graph) {
    return (slabs_per_graph == 0 || slabs_per_graph == net->n_branch || slabs_split(net, slabs_per_graph)) ? 0 : DRGNN_E_ARG;
}
static int head_width_check(const UpdateDst& d) {
    return (d.R != DRGNN_H2 * d.net->n_branch || d.H < 1 || d.H > 512 || d.O < 1 || d.O > DRGNN_MAX_OUT) ? DRGNN_E_WIDTH : 0;
}
// every refusal of the update launches (but the capacity of the norm words: update_run, where the blocks are counted)
static int update_check(const UpdateCall& c) {
    const UpdateDst& d = c.dst;
    if (c.cohort) {
        if (!c.members || c.K < 1 || c.K > 65535 || !c.counts || (c.options && !c.optims)) return DRGNN_E_ARG;
        if (c.flat.n_param < 1 || c.flat.head_offset < 0 || c.flat.head_offset >= c.flat.n_param) return DRGNN_E_ARG;
        if (!d.net) return DRGNN_E_WIDTH;      // (not E_ARG: what a cohort call without a net has always answered)
        if (int rc = head_width_check(d)) return rc;
    }
    if (int rc = net_check(d.net)) return rc;
    if (!d.g_conv1 || !d.g_conv2 || slabs_check(d.net, c.slabs.slabs_per_graph)) return DRGNN_E_ARG;
    if (c.cohort) return 0;
    if (c.options) { if (int rc = optim_check(c.optim)) return rc; }
    if (!c.slabs.conv_partials || !c.slabs.head_partials || !c.flat.grad) return DRGNN_E_ARG;
    if (d.compact && (!c.slabs.readout || !c.step2)) return DRGNN_E_ARG;
    if (c.apply_adam && (!c.flat.param || !c.flat.exp_avg || !c.flat.exp_avg_sq || (!d.compact && !c.step))) return DRGNN_E_ARG;
    return 0;
}
// the conv sums: `rows` slabs [n_branch][net_partial_floats] into the model's own gradient tensors
static void reduce_fill(ReduceArgs& r, const drgnn_net_desc* net, const float* partials, int64_t rows, const drgnn_conv_grads* g1,
                        const drgnn_conv_grads* g2) {
    r = ReduceArgs{};             // (no grad_x; no destinations beyond the net's branches)
    r.partials = partials; r.n_graphs = (int)rows; r.n_branch = net->n_branch;
    r.n_feat = net->n_feat; r.n_partial = (int)net_partial_floats(net->n_feat); r.kind = net->kind;
    for (int b = 0; b < DRGNN_MAX_BRANCH; ++b) { r.lay1[b] = net->conv1[b]; r.lay2[b] = net->conv2[b]; }
    for (int b = 0; b < net->n_branch; ++b) { r.g1[b] = g1[b]; r.g2[b] = g2[b]; }
}
// the sums of an UpdateArgs: the conv sums, the head's sources, dW_fc1's operands, the conv block counts.  Returns the head items of
// the launch: a slab's floats (+ dW_fc1) without its last `n_tail` slots.
static int update_sums_fill(UpdateArgs& u, const UpdateDst& d, const UpdateSlabs& s, int n_tail) {
    reduce_fill(u.r, d.net, s.conv_partials, slabs_split(d.net, s.slabs_per_graph) ? 2 * s.n_graphs : s.n_graphs, d.g_conv1, d.g_conv2);
    u.h.partials = s.head_partials; u.h.n_wg = (int)s.head_slabs;
    u.h.P = (int)(d.compact ? head_compact_floats(d.R, d.H, d.O) : head_partial_floats(d.R, d.H, d.O));
    u.readout = s.readout; u.hR = d.R; u.hH = d.H;
    u.blocks_per_branch = (u.r.n_partial + 63) / 64;
    u.conv_blocks = d.net->n_branch * u.blocks_per_branch;
    return (d.compact ? d.H * d.R : 0) + u.h.P - n_tail;
}

static int update_run(const UpdateCall& c) {
    if (int rc = update_check(c)) return rc;
    UpdateArgs u = {};
    const int head_items = update_sums_fill(u, c.dst, c.slabs, 1);       // the gradient block + the loss (1: not the weight slot)
    const int n_blocks = u.conv_blocks + (head_items + 63) / 64;
    if (!c.cohort) { u.h.grad = c.flat.grad + c.flat.head_offset; u.ad.step = c.dst.compact ? c.step2 + 1 : c.step; }
    u.h.loss = c.loss; u.loss2 = (c.loss || c.cohort) ? c.loss2 : nullptr; u.step2 = c.dst.compact ? c.step2 : nullptr;
    u.ad.param = c.flat.param; u.ad.grad = c.flat.grad; u.ad.exp_avg = c.flat.exp_avg; u.ad.exp_avg_sq = c.flat.exp_avg_sq;
    u.ad.n = c.flat.n_param;
    // the options: AdamW / the learning-rate table inside this launch; a clipping step (and coupled L2) as the sums launch,
    // Adam off, + the flat Adam launch.  Without Adam (data parallel) the launch is the plain one.
    const drgnn_optim* opt = c.apply_adam ? c.optim : nullptr;
    const bool opt_flat = opt && (opt->clip || optim_coupled(opt));
    if (c.optim) optim_adam_args(u.ad, c.optim);
    else adam_set_hyper(u.ad, c.lr, c.beta1, c.beta2, c.eps, 0.0);
    u.apply_adam = (c.apply_adam && !opt_flat) ? 1 : 0;
#ifdef DRGNN_EMU      // (another algorithm: item by item, sums in slab order, against the kernels' 64-element blocks of four quarter sums)
    if (c.cohort) return DRGNN_E_CAPACITY;
    if (opt) u.apply_adam = 0;           // (host loop: the sums here, then the flat loop with the options)
    const ReduceArgs& r = u.r;
    for (int64_t i = 0; i < (int64_t)r.n_branch * r.n_partial; ++i) {
        const int br = (int)(i / r.n_partial), p = (int)(i % r.n_partial);
        if (!reduce_live(r, p)) continue;
        float* d = reduce_dst(r, br, p);
        if (d) update_store(u, d, reduce_sum(r, br, p, 0, 1));
    }
    for (int i = 0; i < head_items; ++i) update_head_store(u, i, update_head_sum(u, i, 0, 1));
    if (u.step2) u.step2[0] = u.step2[1];
    if (opt) return adam_opt_impl(u.ad, c.flat.grad, opt, 0, c.stream);
#else
    const dim3 grid((unsigned)n_blocks, c.cohort ? (unsigned)c.K : 1u), threads(DRGNN_UPDATE_THREADS);
    hipStream_t stream = (hipStream_t)c.stream;
    if (opt) {
        const bool words = opt->clip && !optim_coupled(opt);     // (coupled L2: the flat route's own words)
        if (words && n_blocks > opt->norm_cap) return DRGNN_E_CAPACITY;
        hipLaunchKernelGGL(k_update_opt, grid, threads, 0, stream, u, *opt, words ? opt->norm_words : (double*)nullptr);
        HIP_TRY(hipGetLastError());
        return opt_flat ? adam_opt_impl(u.ad, c.flat.grad, opt, words ? n_blocks : 0, c.stream) : 0;
    }
    if (c.optims) {
        // (the records live in device memory: their norm_cap is the caller's promise, drgnn_optim_norm_words, checked here
        // against this launch's blocks and guarded in the kernel)
        if (c.any_clip && n_blocks > drgnn_optim_norm_words(c.flat.n_param)) return DRGNN_E_CAPACITY;
        hipLaunchKernelGGL(k_update_cohort_opt, grid, threads, 0, stream, u, c.members, c.optims, c.counts, c.flat.head_offset);
        HIP_TRY(hipGetLastError());
        if (!c.any_clip || !c.apply_adam) return 0;
        hipLaunchKernelGGL(k_adam_cohort_opt, dim3((unsigned)((c.flat.n_param + 255) / 256), (unsigned)c.K), dim3(256), 0, stream,
                           c.members, c.optims, c.counts, c.flat.n_param, n_blocks);
    } else if (c.cohort) {
        hipLaunchKernelGGL(k_update_cohort, grid, threads, 0, stream, u, c.members, c.counts, c.flat.head_offset);
    } else {
        hipLaunchKernelGGL(k_update, grid, threads, 0, stream, u);
    }
    HIP_TRY(hipGetLastError());
#endif
    return 0;
}

extern "C" {

int drgnn_net_reduce_grads(const drgnn_net_desc* net, const float* partials, int64_t n_nodes, int64_t n_graphs,
                           drgnn_conv_grads* g_conv1, drgnn_conv_grads* g_conv2, float* grad_x, void* stream_) {
    if (int rc = net_check(net)) return rc;
    if (!partials || !g_conv1 || !g_conv2) return DRGNN_E_ARG;
    ReduceArgs r;
    reduce_fill(r, net, partials, n_graphs, g_conv1, g_conv2);
    r.grad_x = grad_x; r.n_nodes = n_nodes;
    int64_t items = (int64_t)net->n_branch * r.n_partial;
    if (grad_x && net->n_branch > 1 && n_nodes * net->n_feat > items) items = n_nodes * net->n_feat;
#ifdef DRGNN_EMU      // (another algorithm: item by item against k_reduce's blocks of four quarter sums)
    for (int64_t i = 0; i < (int64_t)net->n_branch * r.n_partial; ++i) {
        const int br = (int)(i / r.n_partial), p = (int)(i % r.n_partial);
        if (reduce_live(r, p)) reduce_write(r, br, p, reduce_sum(r, br, p, 0, 1));
    }
    for (int64_t i = 0; grad_x && i < n_nodes * net->n_feat; ++i) reduce_grad_x(r, i);
    (void)stream_; (void)items;
#else
    const int reduce_blocks = net->n_branch * ((r.n_partial + 63) / 64);      // (blocks do not straddle branches)
    hipLaunchKernelGGL(k_reduce, dim3((unsigned)reduce_blocks), dim3(256), 0, (hipStream_t)stream_, r, items);
    HIP_TRY(hipGetLastError());
#endif
    return 0;
}

int drgnn_train_update(const drgnn_net_desc* net, const float* conv_partials, int64_t n_graphs, drgnn_conv_grads* g_conv1,
                       drgnn_conv_grads* g_conv2, const float* head_partials, int64_t head_slabs, int32_t R, int32_t H, int32_t O,
                       int64_t head_offset, float* flat_param, float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_param,
                       const int32_t* step, float* loss, double lr, double beta1, double beta2, double eps, int32_t apply_adam,
                       void* stream_) {
    UpdateCall c = update_call({net, g_conv1, g_conv2, R, H, O, false}, {conv_partials, n_graphs, head_partials, head_slabs, nullptr, 0},
                               {flat_param, flat_grad, exp_avg, exp_avg_sq, n_param, head_offset}, loss, apply_adam, stream_);
    c.step = step; c.lr = lr; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps;
    return update_run(c);
}

int drgnn_step_update(const drgnn_net_desc* net, const float* conv_partials, int64_t n_graphs, drgnn_conv_grads* g_conv1,
                      drgnn_conv_grads* g_conv2, const float* head_partials, const float* readout, int32_t R, int32_t H, int32_t O,
                      int64_t head_offset, float* flat_param, float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_param,
                      int32_t* step2, float* loss, double lr, double beta1, double beta2, double eps, int32_t apply_adam,
                      int32_t slabs_per_graph, void* stream_) {
    UpdateCall c = update_call({net, g_conv1, g_conv2, R, H, O, true},
                               {conv_partials, n_graphs, head_partials, n_graphs, readout, slabs_per_graph},
                               {flat_param, flat_grad, exp_avg, exp_avg_sq, n_param, head_offset}, loss, apply_adam, stream_);
    c.step2 = step2; c.lr = lr; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps;
    return update_run(c);
}

int drgnn_train_update_opt(const drgnn_net_desc* net, const float* conv_partials, int64_t n_graphs, drgnn_conv_grads* g_conv1,
                           drgnn_conv_grads* g_conv2, const float* head_partials, int64_t head_slabs, int32_t R, int32_t H, int32_t O,
                           int64_t head_offset, float* flat_param, float* flat_grad, float* exp_avg, float* exp_avg_sq,
                           int64_t n_param, const int32_t* step, float* loss, const drgnn_optim* optim, int32_t apply_adam,
                           void* stream_) {
    UpdateCall c = update_call({net, g_conv1, g_conv2, R, H, O, false}, {conv_partials, n_graphs, head_partials, head_slabs, nullptr, 0},
                               {flat_param, flat_grad, exp_avg, exp_avg_sq, n_param, head_offset}, loss, apply_adam, stream_);
    c.step = step; c.optim = optim; c.options = true;
    return update_run(c);
}

int drgnn_step_update_opt(const drgnn_net_desc* net, const float* conv_partials, int64_t n_graphs, drgnn_conv_grads* g_conv1,
                          drgnn_conv_grads* g_conv2, const float* head_partials, const float* readout, int32_t R, int32_t H,
                          int32_t O, int64_t head_offset, float* flat_param, float* flat_grad, float* exp_avg, float* exp_avg_sq,
                          int64_t n_param, int32_t* step2, float* loss, const drgnn_optim* optim, int32_t apply_adam,
                          int32_t slabs_per_graph, void* stream_) {
    UpdateCall c = update_call({net, g_conv1, g_conv2, R, H, O, true},
                               {conv_partials, n_graphs, head_partials, n_graphs, readout, slabs_per_graph},
                               {flat_param, flat_grad, exp_avg, exp_avg_sq, n_param, head_offset}, loss, apply_adam, stream_);
    c.step2 = step2; c.optim = optim; c.options = true;
    return update_run(c);
}

static UpdateCall cohort_call(const UpdateDst& dst, const UpdateFlat& flat, const drgnn_cohort_member* members, int32_t K,
                              const int32_t* counts, float* losses, int32_t apply_adam, void* stream) {
    UpdateCall c = update_call(dst, UpdateSlabs{}, flat, nullptr, apply_adam, stream);
    c.cohort = true; c.members = members; c.K = K; c.counts = counts; c.loss2 = losses;
    return c;
}
int drgnn_cohort_update(const drgnn_net_desc* net, const drgnn_cohort_member* members, int32_t K, const int32_t* counts,
                        drgnn_conv_grads* g_conv1, drgnn_conv_grads* g_conv2, int32_t R, int32_t H, int32_t O,
                        int64_t head_offset, int64_t n_param, float* losses, int32_t apply_adam, void* stream_) {
    return update_run(cohort_call({net, g_conv1, g_conv2, R, H, O, true}, {nullptr, nullptr, nullptr, nullptr, n_param, head_offset},
                                  members, K, counts, losses, apply_adam, stream_));
}

int drgnn_cohort_update_opt(const drgnn_net_desc* net, const drgnn_cohort_member* members, const drgnn_optim* optims, int32_t K,
                            const int32_t* counts, drgnn_conv_grads* g_conv1, drgnn_conv_grads* g_conv2, int32_t R, int32_t H,
                            int32_t O, int64_t head_offset, int64_t n_param, float* losses, int32_t apply_adam, int32_t any_clip,
                            void* stream_) {
    UpdateCall c = cohort_call({net, g_conv1, g_conv2, R, H, O, true}, {nullptr, nullptr, nullptr, nullptr, n_param, head_offset},
                               members, K, counts, losses, apply_adam, stream_);
    c.optims = optims; c.options = true; c.any_clip = any_clip;
    return update_run(c);
}

int drgnn_step_gradients(const drgnn_net_desc* net, const float* conv_partials, int64_t n_graphs, drgnn_conv_grads* g_conv1,
                         drgnn_conv_grads* g_conv2, const float* head_partials, const float* readout, int32_t R, int32_t H, int32_t O,
                         float* head_grad, const float* graph_weight, float* const* zero_ptr, const int64_t* zero_len, int32_t n_zero,
                         int32_t* step2, int32_t slabs_per_graph, void* stream_) {
    const UpdateDst dst = {net, g_conv1, g_conv2, R, H, O, true};
    int rc;
    if ((rc = net_check(net))) return rc;
    if (!conv_partials || !g_conv1 || !g_conv2 || !head_partials || !readout || !head_grad || n_graphs < 0) return DRGNN_E_ARG;
    if (n_zero < 0 || n_zero > DRGNN_ZERO_RANGES || (n_zero > 0 && (!zero_ptr || !zero_len))) return DRGNN_E_ARG;
    if ((rc = slabs_check(net, slabs_per_graph)) || (rc = head_width_check(dst))) return rc;
    GradArgs ga = {};
    UpdateArgs& u = ga.u;
    // the gradient block (2: neither the loss nor the weight slot is a gradient)
    const int head_items = update_sums_fill(u, dst, {conv_partials, n_graphs, head_partials, n_graphs, readout, slabs_per_graph}, 2);
    const int head_blocks = (head_items + 63) / 64;
    u.h.grad = head_grad; u.step2 = step2;
    ga.graph_weight = graph_weight; ga.wshift = slabs_split(net, slabs_per_graph) ? 1 : 0; ga.n_zero = n_zero;
    for (int i = 0; i < n_zero; ++i) {
        if (!zero_ptr[i] || zero_len[i] < 0) return DRGNN_E_ARG;
        ga.zero_ptr[i] = zero_ptr[i]; ga.zero_len[i] = zero_len[i];
    }
#ifdef DRGNN_EMU      // (another algorithm: item by item against k_gradients' blocks of four quarter sums)
    const ReduceArgs& r = u.r;
    for (int64_t i = 0; i < (int64_t)net->n_branch * r.n_partial; ++i) {
        const int br = (int)(i / r.n_partial), p = (int)(i % r.n_partial);
        if (!reduce_live(r, p)) continue;
        float* d = reduce_dst(r, br, p);
        if (d) *d = graph_weight ? reduce_sum_w(r, br, p, 0, 1, graph_weight, ga.wshift) : reduce_sum(r, br, p, 0, 1);
    }
    for (int i = 0; i < head_items; ++i)
        head_grad[i] = graph_weight ? update_head_sum_w(u, i, 0, 1, graph_weight) : update_head_sum(u, i, 0, 1);
    for (int i = 0; i < n_zero; ++i) memset(ga.zero_ptr[i], 0, sizeof(float) * (size_t)ga.zero_len[i]);
    if (step2) step2[0] = step2[1];
    (void)stream_; (void)head_blocks;
#else
    hipLaunchKernelGGL(k_gradients, dim3((unsigned)(u.conv_blocks + head_blocks + 1)), dim3(256), 0, (hipStream_t)stream_, ga);
    HIP_TRY(hipGetLastError());
#endif
    return 0;
}

// ---- mini-batch assembly from the resident graph set -----------------------------------------------
int drgnn_collate(const drgnn_graph_set* set, const int32_t* ids, int64_t n_graphs, int64_t n_nodes,
                  int64_t n_edges, float* x, int64_t* edge_index, float* edge_attr, int64_t* batch,
                  int64_t* cluster0, int64_t* cluster1, void* y, int32_t* node_ptr, int32_t* edge_ptr,
                  int32_t* c1_ptr, void* stream) {
    if (!set || !ids || n_graphs < 0 || n_nodes < 0 || n_edges < 0 || !node_ptr || !edge_ptr) return DRGNN_E_ARG;
    if (!set->node_ptr || !set->edge_ptr || set->n_feat <= 0 || set->n_graphs < 0) return DRGNN_E_ARG;
    if (n_nodes > 0 && (!x || !batch || !set->x)) return DRGNN_E_ARG;
    if (n_edges > 0 && (!edge_index || !set->edge_index)) return DRGNN_E_ARG;
    if ((edge_attr && !set->edge_attr) || (cluster0 && !set->cluster0)) return DRGNN_E_ARG;
    if (cluster1 && (!set->cluster1 || !set->c1_ptr || !c1_ptr)) return DRGNN_E_ARG;
    if (y && (!set->y || (set->y_bytes != 4 && set->y_bytes != 8))) return DRGNN_E_ARG;
    if (n_nodes > 0x7fffffffLL || n_edges > 0x7fffffffLL) return DRGNN_E_CAPACITY;   // int32 offset tables
    if (n_graphs == 0) return 0;
    CollateArgs a;
    a.set = *set; a.ids = ids; a.n_graphs = (int)n_graphs; a.n_edges = n_edges;
    a.x = x; a.edge_index = edge_index; a.edge_attr = edge_attr; a.batch = batch;
    a.cluster0 = cluster0; a.cluster1 = cluster1; a.y = y;
    a.node_ptr = node_ptr; a.edge_ptr = edge_ptr; a.c1_ptr = set->c1_ptr ? c1_ptr : nullptr;
    DRGNN_EMU_ONLY(int sh[4];)
    DRGNN_LAUNCH(k_collate, grid1(n_graphs), stream, collate_block(a, (int)bx, sh), a);
    return 0;
}

// ---- one training epoch, driven from here ---------------------------------------------------------
namespace {
struct EpochBatch { int64_t first, B, N, E, C; int maxN, maxE, maxC; };
struct EpochSlot { float* x; void* y; int32_t* ws_i32; float* ws_f32; float* tiles; };
struct EpochCarve {
    EpochSlot slot[2];
    int32_t* ptrs;                 // [n_batches][3][batch_size + 1]
    float* readout; float* partials; float* head_partials; uint64_t* xchg; int64_t xchg_bytes;
    int64_t bytes;
};
int epoch_batch(const drgnn_epoch_plan* p, int64_t k, EpochBatch* b) {
    const int64_t G = p->set->n_graphs;
    b->first = k * p->batch_size;
    b->B = p->n_ids - b->first < p->batch_size ? p->n_ids - b->first : p->batch_size;
    b->N = b->E = b->C = 0; b->maxN = b->maxE = b->maxC = 0;
    for (int64_t q = 0; q < b->B; ++q) {
        const int64_t id = p->host_ids[b->first + q];
        if (id < 0 || id >= G) return DRGNN_E_ARG;
        const int64_t n = p->host_node_ptr[id + 1] - p->host_node_ptr[id];
        const int64_t e = p->host_edge_ptr[id + 1] - p->host_edge_ptr[id];
        const int64_t c = p->host_c1_ptr[id + 1] - p->host_c1_ptr[id];
        if (n < 0 || e < 0 || c < 0) return DRGNN_E_ARG;
        b->N += n; b->E += e; b->C += c;
        if (n > b->maxN) b->maxN = (int)n;
        if (e > b->maxE) b->maxE = (int)e;
        if (c > b->maxC) b->maxC = (int)c;
    }
    return 0;
}
int epoch_check(const drgnn_epoch_plan* p) {
    if (!p || !p->set || !p->host_node_ptr || !p->host_edge_ptr || !p->ids || !p->host_ids || p->n_ids < 0 ||
        p->batch_size < 1 || !p->net || !p->head || !p->step2)
        return DRGNN_E_ARG;
    if (!p->inference && (!p->g_conv1 || !p->g_conv2 || !p->flat_param || !p->flat_grad || !p->exp_avg || !p->exp_avg_sq))
        return DRGNN_E_ARG;
    const drgnn_graph_set* gs = p->set;
    if (p->cache) {      // cached topology: the set is only consulted for sizes (host tables)
        const drgnn_topology_cache* tc = p->cache;
        if (!tc->ws_i32 || !tc->x || tc->n_graphs != gs->n_graphs || !p->host_c1_ptr) return DRGNN_E_ARG;
        if (p->need_weights && !tc->ws_f32) return DRGNN_E_ARG;
        if (!p->inference && (!tc->y || tc->y_bytes != (p->head->task == DRGNN_TASK_REG ? 4 : 8))) return DRGNN_E_ARG;
        if (gs->n_feat != p->net->n_feat) return DRGNN_E_WIDTH;
        if (p->batch_size > 4096) return DRGNN_E_CAPACITY;
        return 0;
    }
    if (!gs->node_ptr || !gs->edge_ptr || !gs->x || !gs->cluster0 || !gs->cluster1 || !gs->c1_ptr || !p->host_c1_ptr)
        return DRGNN_E_ARG;
    if (!p->inference && !gs->y) return DRGNN_E_ARG;
    if (gs->n_edges > 0 && !gs->edge_index) return DRGNN_E_ARG;
    if (p->need_weights && !gs->edge_attr) return DRGNN_E_ARG;
    if (gs->n_feat != p->net->n_feat) return DRGNN_E_WIDTH;
    if (!p->inference && gs->y_bytes != (p->head->task == DRGNN_TASK_REG ? 4 : 8)) return DRGNN_E_ARG;
    if (p->batch_size > 4096) return DRGNN_E_CAPACITY;
    return 0;
}
// the plan of mini-batch b's step launch on a workspace with `topo_flags` (co = graphs of the topology co-built by the same
// launch); family NONE: a graph does not fit the fused kernels
drgnn_step_plan epoch_plan_of(const drgnn_epoch_plan* p, const EpochBatch& b, int64_t co, int32_t topo_flags) {
    const drgnn_head_desc* hd = p->head;
    drgnn_step_plan pl;
    memset(&pl, 0, sizeof(pl));
    pl.kind = p->net->kind; pl.n_feat = p->net->n_feat; pl.max_nodes = b.maxN; pl.max_edges = b.maxE; pl.max_c0 = b.maxC;
    pl.R = hd->R; pl.H = hd->H; pl.O = hd->O; pl.n_graphs = b.B; pl.co_built_graphs = co;
    pl.train = p->inference ? 0 : 1; pl.topo_flags = topo_flags;
    if (p->step_overrides) {
        const drgnn_step_plan* o = p->step_overrides;
        pl.force_wgs = o->force_wgs; pl.no_class = o->no_class; pl.no_aggregate = o->no_aggregate; pl.no_split = o->no_split;
    }
    drgnn_net_step_plan(&pl);
    return pl;
}
// what the workspace of mini-batch b holds when its step is launched: the cache's flags, or what the loop asks its own builder
// for -- the hierarchical order, the aggregation tiles and nothing else (DRGNN_TOPO_LEAN) when the step that consumes it is one
// of the aggregation-first kernels, else the plain build (+ the order for the single-branch nets)
int32_t epoch_topo_flags(const drgnn_epoch_plan* p, const EpochBatch& b, int64_t co, const float* slot_x) {
    if (p->cache) {
        int32_t f = p->cache->flags;
        if (!p->cache->tiles) f &= ~DRGNN_TOPO_TILES;
        return f;
    }
    const bool f4 = (p->net->n_feat & 3) == 0;      // (16-byte aligned rows are only needed where rows ARE multiples of 16 bytes)
    const bool tiles_ok = drgnn_topology_tiles_ok(b.maxN, b.maxE, p->net->n_feat) != 0 && p->set->x != nullptr &&
                          (!f4 || (((((uintptr_t)p->set->x) & 15) == 0) && ((((uintptr_t)slot_x) & 15) == 0)));
    const int32_t af = DRGNN_TOPO_HIER | DRGNN_TOPO_LEAN | DRGNN_TOPO_TILES;
    if (tiles_ok && epoch_plan_of(p, b, co, af).lean_ok) return af;
    return (p->net->kind != DRGNN_GINET && !p->inference) ? DRGNN_TOPO_HIER : 0;
}
int64_t epoch_next_b(const drgnn_epoch_plan* p, int64_t k) {      // graphs of mini-batch k + 1 (0: none)
    const int64_t first = (k + 1) * p->batch_size;
    if (first >= p->n_ids) return 0;
    return p->n_ids - first < p->batch_size ? p->n_ids - first : p->batch_size;
}
// sizes the two mini-batch slots and the step slabs for the largest mini-batch of the plan
int epoch_carve(const drgnn_epoch_plan* p, char* base, EpochCarve* c) {
    int rc = epoch_check(p);
    if (rc) return rc;
    const int64_t nb = (p->n_ids + p->batch_size - 1) / p->batch_size;
    int64_t capN = 1, capB = 1, ws_i = 4, ws_f = 4, xchg_words = 0;
    bool any_split = false;
    const drgnn_head_desc* hd = p->head;
    for (int64_t k = 0; k < nb; ++k) {
        EpochBatch b;
        if ((rc = epoch_batch(p, k, &b))) return rc;
        if (b.maxN <= 0) return DRGNN_E_CAPACITY;
        // (slot buffers are 256-byte aligned: the alignment of x does not depend on the slot)
        const int64_t co = p->cache ? 0 : epoch_next_b(p, k);
        const drgnn_step_plan pl = epoch_plan_of(p, b, co, epoch_topo_flags(p, b, co, nullptr));
        if (pl.slabs_per_graph == 2 && p->net->kind != DRGNN_GINET) any_split = true;
        if (pl.xchg_words * b.B > xchg_words) xchg_words = pl.xchg_words * b.B;
        if (pl.family == DRGNN_STEP_FAMILY_NONE ||
            pl.lds_bytes > DRGNN_LDS_LIMIT || b.maxN > 32767 || b.maxE > 65535 ||
            (!p->cache && drgnn_topology_lds_bytes(b.maxN, b.maxE > 0 ? b.maxE : 1) > DRGNN_LDS_LIMIT))
            return DRGNN_E_CAPACITY;
        TopoLayout lay;
        topo_layout(b.N, b.E, b.B, &lay);
        if (lay.i32[DRGNN_TI_COUNT] > ws_i) ws_i = lay.i32[DRGNN_TI_COUNT];
        if (lay.f32[DRGNN_TF_COUNT] > ws_f) ws_f = lay.f32[DRGNN_TF_COUNT];
        if (b.N > capN) capN = b.N;
        if (b.B > capB) capB = b.B;
    }
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char* q = base ? base + o : nullptr; o += (bytes + 255) & ~(int64_t)255; return (void*)q; };
    const int F = p->net->n_feat, nbr = p->net->n_branch;
    for (int s = 0; s < 2; ++s) {
        EpochSlot& t = c->slot[s];
        if (p->cache) { t.x = nullptr; t.y = nullptr; t.ws_i32 = nullptr; t.ws_f32 = nullptr; t.tiles = nullptr; continue; }   // nothing to build
        t.x = (float*)take(capN * F * 4);
        t.tiles = (float*)take(drgnn_topology_tiles_elems(capN, F) * 4);      // (aggregation tiles of the slot's mini-batch)
        t.y = take(capB * 8);
        t.ws_i32 = (int32_t*)take(ws_i * 4);
        t.ws_f32 = p->need_weights ? (float*)take(ws_f * 4) : nullptr;
    }
    c->ptrs = p->cache ? nullptr : (int32_t*)take((nb > 0 ? nb : 1) * 3 * ((int64_t)p->batch_size + 1) * 4);
    c->readout = (float*)take(capB * hd->R * 4);
    c->partials = (float*)take(capB * (any_split ? 2 : nbr) * drgnn_net_partial_elems(p->net->kind, F) * 4);
    c->head_partials = (float*)take(capB * drgnn_head_compact_elems(hd->R, hd->H, hd->O) * 4);
    c->xchg_bytes = capB * nbr * (int64_t)(hd->H > DRGNN_H2 ? hd->H : DRGNN_H2) * 8;
    if (xchg_words * 8 > c->xchg_bytes) c->xchg_bytes = xchg_words * 8;
    c->xchg = (uint64_t*)take(c->xchg_bytes);
    c->bytes = o;
    return 0;
}
}  // namespace

int64_t drgnn_train_epoch_scratch_bytes(const drgnn_epoch_plan* plan) {
    EpochCarve c;
    const int rc = epoch_carve(plan, nullptr, &c);
    return rc ? (int64_t)rc : c.bytes;
}

// reduction of the step's slabs + optimiser update of mini-batch k: one launch, or (data parallel) gradient launch ->
// the caller's exchange -> Adam launch
static int epoch_update(const drgnn_epoch_plan* p, const EpochCarve& c, int64_t B, int64_t k, float* losses, void* stream,
                        int slabs_per_graph, const drgnn_optim* o) {
    const drgnn_head_desc* hd = p->head;
    const int fused = p->exchange ? 0 : 1;
    // (the last mini-batch of the call also writes the caller's loss word, drgnn_epoch_plan.last_loss)
    const int64_t nb = (p->n_ids + p->batch_size - 1) / p->batch_size;
    UpdateCall u = update_call({p->net, p->g_conv1, p->g_conv2, hd->R, hd->H, hd->O, true},
                               {c.partials, B, c.head_partials, B, c.readout, slabs_per_graph},
                               {p->flat_param, p->flat_grad, p->exp_avg, p->exp_avg_sq, p->n_param, p->head_offset}, losses + k, fused,
                               stream);
    u.step2 = p->step2; u.loss2 = (k == nb - 1) ? p->last_loss : nullptr;
    u.lr = p->lr; u.beta1 = p->beta1; u.beta2 = p->beta2; u.eps = p->eps; u.optim = o; u.options = o != nullptr;
    int rc = update_run(u);
    if (rc || fused) return rc;
    if ((rc = p->exchange(p->exchange_user, k, B, stream))) return rc;
    if (o) return drgnn_adam_step_opt(p->flat_param, p->flat_grad, p->exp_avg, p->exp_avg_sq, p->step2, p->n_param, o, stream);
    return drgnn_adam_step(p->flat_param, p->flat_grad, p->exp_avg, p->exp_avg_sq, p->step2, p->n_param, p->lr, p->beta1,
                           p->beta2, p->eps, 0.0, stream);
}

static int train_epoch_impl(const drgnn_epoch_plan* p, const drgnn_optim* optim, void* scratch, int64_t scratch_bytes, float* pred,
                            float* losses, void* stream);
int drgnn_train_epoch(const drgnn_epoch_plan* p, void* scratch, int64_t scratch_bytes, float* pred, float* losses,
                      void* stream) {
    return train_epoch_impl(p, nullptr, scratch, scratch_bytes, pred, losses, stream);
}
int drgnn_train_epoch_opt(const drgnn_epoch_plan* p, const drgnn_optim* optim, void* scratch, int64_t scratch_bytes, float* pred,
                          float* losses, void* stream) {
    const int rc = optim_check(optim);
    return rc ? rc : train_epoch_impl(p, optim, scratch, scratch_bytes, pred, losses, stream);
}
static int train_epoch_impl(const drgnn_epoch_plan* p, const drgnn_optim* optim, void* scratch, int64_t scratch_bytes, float* pred,
                            float* losses, void* stream) {
    EpochCarve c;
    int rc = epoch_carve(p, (char*)scratch, &c);
    if (rc) return rc;
    if (p->n_ids == 0) return 0;
    const bool train = !p->inference;
    if (!scratch || !pred || (train && !losses) || ((uintptr_t)scratch & 15)) return DRGNN_E_ARG;
    if (scratch_bytes < c.bytes) return DRGNN_E_CAPACITY;
    const int64_t nb = (p->n_ids + p->batch_size - 1) / p->batch_size;
    const drgnn_head_desc* hd = p->head;
    drgnn_head_desc head = *hd;
    head.train = train ? 1 : 0;
    // the exchange words carry the step index as a tag: they only have to start from a value no step uses
    if ((rc = drgnn_clear(c.xchg, (size_t)c.xchg_bytes, stream))) return rc;
    if (p->cache) {
        // cached topology: a mini-batch is its list of graph numbers -- step launch (+ update launch), nothing else
        for (int64_t k = 0; k < nb; ++k) {
            EpochBatch b;
            if ((rc = epoch_batch(p, k, &b))) return rc;
            drgnn_topology_cache tc = *p->cache;
            if (!train) tc.y = nullptr;
            drgnn_step_hints hints = {};
            hints.set_node_ptr = p->host_node_ptr; hints.set_edge_ptr = p->host_edge_ptr; hints.host_ids = p->host_ids + b.first;
            const drgnn_step_plan pl = epoch_plan_of(p, b, 0, epoch_topo_flags(p, b, 0, nullptr));
            const bool split = pl.slabs_per_graph == 2 && p->net->kind != DRGNN_GINET;
            hints.topo_flags = pl.topo_flags; hints.plan = &pl;
            hints.tiles = p->cache->tiles;
            // the graphs of mini-batch k + 1: prefetched by spare workgroups of this launch
            if (k + 1 < nb) { hints.next_ids = p->ids + b.first + b.B; hints.n_next = epoch_next_b(p, k); }
            rc = drgnn_net_train_step_cached(p->net, &head, &tc, p->ids + b.first, b.B, b.maxN, b.maxE, b.maxC, p->step2,
                                             pred + b.first * hd->O, c.readout, train ? c.head_partials : nullptr,
                                             train ? c.partials : nullptr, c.xchg, &hints, stream);
            if (rc) return rc;
            if (!train) continue;
            if ((rc = epoch_update(p, c, b.B, k, losses, stream, split ? 2 : 0, optim))) return rc;
        }
        return 0;
    }
    if ((rc = drgnn_batch_offsets(p->set, p->ids, p->n_ids, p->batch_size, c.ptrs, stream))) return rc;
    const int64_t W = (int64_t)p->batch_size + 1;
    // mini-batch k's topology + node features + targets, straight from the resident set into slot k & 1
    auto request = [&](int64_t k, const EpochBatch& b) {
        const EpochSlot& u = c.slot[k & 1];
        drgnn_topology_request r = {};
        int32_t* pk = c.ptrs + k * 3 * W;
        r.node_ptr = pk; r.edge_ptr = pk + W; r.c1_ptr = pk + 2 * W;
        r.n_nodes = b.N; r.n_edges = b.E; r.len_cluster1 = b.C; r.n_graphs = b.B;
        r.max_nodes = b.maxN; r.max_edges = b.maxE;
        r.ws_i32 = u.ws_i32; r.ws_f32 = u.ws_f32; r.scratch_i32 = nullptr;
        r.set = p->set; r.ids = p->ids + b.first; r.x_out = u.x; r.y_out = train ? u.y : nullptr;
        // (what the step that consumes this workspace reads: epoch_topo_flags)
        r.flags = epoch_topo_flags(p, b, epoch_next_b(p, k), u.x);
        if (r.flags & DRGNN_TOPO_TILES) { r.tiles = u.tiles; r.n_feat = p->net->n_feat; }
        return r;
    };
    EpochBatch cur, nxt;
    std::vector<int32_t> hn, he;       // (slot offset tables of the current mini-batch, reused)
    if ((rc = epoch_batch(p, 0, &cur))) return rc;
    int32_t cur_flags = 0;
    {
        const drgnn_topology_request r0 = request(0, cur);
        cur_flags = r0.flags;
        if ((rc = drgnn_topology_build_request(&r0, stream))) return rc;
    }
    for (int64_t k = 0; k < nb; ++k) {
        const EpochSlot& t = c.slot[k & 1];
        drgnn_topology_request req;
        const bool more = k + 1 < nb;
        if (more) {
            if ((rc = epoch_batch(p, k + 1, &nxt))) return rc;
            req = request(k + 1, nxt);
        }
        // the slot offsets of this mini-batch are known here (host size tables): hand them to the launch
        drgnn_step_hints hints = {};
        const drgnn_step_plan pl = epoch_plan_of(p, cur, more ? nxt.B : 0, cur_flags);      // (cur_flags: what request() asked the builder for)
        const bool split = pl.slabs_per_graph == 2 && p->net->kind != DRGNN_GINET;
        hints.topo_flags = cur_flags;
        hints.tiles = (cur_flags & DRGNN_TOPO_TILES) ? t.tiles : nullptr;
        hints.plan = &pl;
        if (cur.B <= DRGNN_STEP_DIMS_MAX) {
            hn.resize((size_t)cur.B + 1); he.resize((size_t)cur.B + 1);
            hn[0] = 0; he[0] = 0;
            for (int64_t q = 0; q < cur.B; ++q) {
                const int64_t id = p->host_ids[cur.first + q];
                hn[q + 1] = hn[q] + (int32_t)(p->host_node_ptr[id + 1] - p->host_node_ptr[id]);
                he[q + 1] = he[q] + (int32_t)(p->host_edge_ptr[id + 1] - p->host_edge_ptr[id]);
            }
            hints.host_node_ptr = hn.data(); hints.host_edge_ptr = he.data();
        }
        rc = drgnn_net_train_step(p->net, &head, t.x, train ? t.y : nullptr, p->step2, t.ws_i32, t.ws_f32, cur.N, cur.E,
                                  cur.B, cur.maxN, cur.maxE, cur.maxC, pred + cur.first * hd->O, c.readout,
                                  train ? c.head_partials : nullptr, train ? c.partials : nullptr, c.xchg,
                                  more ? &req : nullptr, &hints, stream);
        if (rc) return rc;
        if (more) cur_flags = req.flags;
        if (!train) { if (more) cur = nxt; continue; }
        if ((rc = epoch_update(p, c, cur.B, k, losses, stream, split ? 2 : 0, optim))) return rc;
        if (more) cur = nxt;
    }
    return 0;
}

}  // extern "C"

#ifdef DRGNN_EMU      // (the emulation is built from this file alone, in one g++ call: the feature units are part of it)
#include "drgnn_capi_layers.hip"
#include "drgnn_capi_iface.hip"
#include "drgnn_capi_residues.hip"
#include "drgnn_capi_poses.hip"
#include "drgnn_capi_metrics.hip"
#endif
