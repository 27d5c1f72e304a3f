/*
 * drgnn.h -- C ABI of the MI355X-native Deeprank-GNN message-passing hot path.
 *
 * One shared object (deeprank-gnn_amd/csrc/libdrgnn.so, built by hipcc for gfx950).
 * Every entry point takes raw DEVICE pointers, explicit sizes and a hipStream_t (passed
 * as void*), never allocates, never synchronises, and is hipGraph-capturable.  Return
 * value: 0 on success, a positive hipError_t from the launch, or a negative DRGNN_E_*
 * for argument errors detected on the host.  Data-dependent errors detected on the
 * device (malformed edge lists, wrong cluster1 length ...) are recorded per graph in the
 * topology workspace (DRGNN_TI_GSTAT / DRGNN_TI_ERR) and poison that graph's outputs with
 * NaN; read them back with drgnn_topology_status().
 *
 * The reference has no C/FFI boundary (it is pure Python on torch_geometric /
 * torch_scatter / torch_sparse, which are un-vendored).  Each entry point cites the
 * reference function (file:line under the reference repository) whose arithmetic it
 * replaces; the Python class protocol above this ABI (GINet / sGAT / FoutNet,
 * community_pooling ...) lives in deeprank-gnn_amd/ and mirrors the reference names.
 *
 * Index tensors arrive as the reference stores them (int64 edge_index [2,E], cluster
 * ids, batch vector: DataSet.py:268-269,354-357); everything derived is int32.
 */
#ifndef DRGNN_H
#define DRGNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRGNN_ABI_VERSION 5

/* host-side argument errors */
#define DRGNN_E_ARG      (-1)   /* null pointer / negative size / bad mode            */
#define DRGNN_E_CAPACITY (-2)   /* workspace too small for the request                */
#define DRGNN_E_WIDTH    (-3)   /* feature width not supported by the fused kernels   */

/* device-side status bits (DRGNN_TI_ERR[0]) */
#define DRGNN_S_EDGE_RANGE    1  /* an edge endpoint lies outside its graph's node range */
#define DRGNN_S_UNSORTED      2  /* batch vector / edge list not grouped by graph        */
#define DRGNN_S_CLUSTER_RANGE 4  /* a graph's cluster ids span more than N_g+E_g+1 values*/
#define DRGNN_S_CLUSTER1_LEN  8  /* len(cluster1) != number of depth-0 clusters          */
/* fault bits of step2[2] (fused training step) */
#define DRGNN_FAULT_EXCHANGE  1  /* a GINet branch workgroup waited in vain for its partner's half of fc1 (value = NaN) */
#define DRGNN_FAULT_SPLIT     2  /* a half-graph workgroup of the node-split layout waited in vain for its partner's hand-off */

/* layer kinds (what "conv" means) */
#define DRGNN_GINET 0  /* z_i = sum_{e:row=i} W x_col            ginet.py:50-73 (alpha == 1)   */
#define DRGNN_SGAT  1  /* z_i = mean_e a_e [x_i||x_col] W + b     sGAT.py:62-93                 */
#define DRGNN_FOUT  2  /* z_i = x_i Wc + mean_e (x Wn)_col + b    foutnet.py:56-82 (NaN if deg 0)*/

/* ---- topology workspace ----------------------------------------------------------
 * Built once per mini-batch from the index tensors only (no learned quantity), shared
 * by both GINet branches and by forward and backward.  Layout: "padded per-graph
 * segments" -- graph g owns node slots [nptr[g], nptr[g+1]) and edge slots
 * [eptr[g], eptr[g+1]) of every array, pooled levels use a prefix of the same slots
 * (C0_g <= N_g, E1_g <= E_g), pointer-like arrays of length n+1 start at nptr[g]+g.
 * All node/cluster ids stored inside are LOCAL to their graph.
 */
enum drgnn_topo_i32 {
    DRGNN_TI_NPTR = 0,   /* [B+1]  node offsets per graph                                   */
    DRGNN_TI_EPTR,       /* [B+1]  edge offsets per graph                                   */
    DRGNN_TI_ROWPTR0,    /* [N+B]  CSR by row (edge_index[0]) of the input graph            */
    DRGNN_TI_COL0,       /* [E]    neighbour (edge_index[1]), rows ordered by edge id       */
    DRGNN_TI_EID0,       /* [E]    original edge id (local) of every CSR slot               */
    DRGNN_TI_COLPTR0,    /* [N+B]  CSC (transpose) of the input graph                        */
    DRGNN_TI_ROWIDX0,    /* [E]                                                              */
    DRGNN_TI_TSLOT0,     /* [E]    CSR slot of every CSC entry (to look up its weight)      */
    DRGNN_TI_CL0,        /* [N]    consecutive depth-0 cluster id of every node             */
    DRGNN_TI_NC0,        /* [B]    number of depth-0 clusters                                */
    DRGNN_TI_MPTR0,      /* [N+B]  member lists of depth-0 clusters                          */
    DRGNN_TI_MEM0,       /* [N]    members, ascending node id inside a cluster               */
    DRGNN_TI_ROWPTR1,    /* [N+B]  CSR of the pooled graph (pool_edge output, sorted)        */
    DRGNN_TI_COL1,       /* [E]                                                              */
    DRGNN_TI_NE1,        /* [B]    number of pooled edges                                    */
    DRGNN_TI_COLPTR1,    /* [N+B]  CSC of the pooled graph                                   */
    DRGNN_TI_ROWIDX1,    /* [E]                                                              */
    DRGNN_TI_TSLOT1,     /* [E]                                                              */
    DRGNN_TI_CL1,        /* [N]    consecutive depth-1 cluster id of every depth-0 cluster   */
    DRGNN_TI_NC1,        /* [B]                                                              */
    DRGNN_TI_MPTR1,      /* [N+B]                                                            */
    DRGNN_TI_MEM1,       /* [N]                                                              */
    DRGNN_TI_CPTR0,      /* [B+1]  exclusive scan of NC0  (filled by drgnn_topology_finalize)*/
    DRGNN_TI_E1PTR,      /* [B+1]  exclusive scan of NE1                                     */
    DRGNN_TI_CPTR1,      /* [B+1]  exclusive scan of NC1                                     */
    DRGNN_TI_ERR,        /* [4]    [0] batch-level status bits (offset derivation)           */
    DRGNN_TI_GSTAT,      /* [2B]   per-graph status bits (edge half, member half), rewritten by every build */
    /* Hierarchical node order (built with depth 1): nodes sorted by (depth-1 cluster of their depth-0 cluster, depth-0
     * cluster, node id), i.e. the members of a depth-0 cluster are consecutive positions and the depth-0 clusters of a
     * depth-1 cluster are consecutive runs, in the order of MEM1.  The node-split step kernels (csrc/drgnn_step2.h) keep
     * their rows in this order: cluster maxima run over contiguous rows and a prefix of the depth-1 clusters is a prefix
     * of the positions (what lets two workgroups share one graph with both poolings local). */
    DRGNN_TI_HORD,       /* [N]    local node id at hierarchical position p                                      */
    DRGNN_TI_HMP0,       /* [N+B]  first position of the q-th depth-0 cluster IN MEM1 ORDER, q = 0..C0            */
    DRGNN_TI_HSPLIT,     /* [4B]   per graph {k, MPTR1[k], HMP0[MPTR1[k]], C1}: k = the number of leading depth-1
                                   clusters whose node total is closest to N/2 (the two-workgroup split point)   */
    DRGNN_TI_IHORD,      /* [N]    hierarchical position of local node i (the inverse of HORD)                    */
    DRGNN_TI_COUNT
};
enum drgnn_topo_f32 {
    DRGNN_TF_W0 = 0,     /* [E] edge_attr in CSR0 slot order                                 */
    DRGNN_TF_W1,         /* [E] pooled edge_attr (duplicates summed) in CSR1 slot order      */
    DRGNN_TF_COUNT
};

/* Element offsets of every array inside the two workspaces, and their total sizes.
 * off_i32 has DRGNN_TI_COUNT+1 entries (last = total int32 elements), off_f32 has
 * DRGNN_TF_COUNT+1 entries. */
int drgnn_topology_layout(int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                          int64_t* off_i32, int64_t* off_f32);

/* Build the topology workspace.
 * Replaces, for the whole mini-batch and without host synchronisation:
 *   - the implicit COO use of edge_index in the conv layers (ginet.py:52, sGAT.py:64,
 *     foutnet.py:58,71-73)                                      -> CSR0 / CSC0
 *   - get_preloaded_cluster (community_pooling.py:25-30) + consecutive_cluster [3P]
 *                                                               -> CL0/CL1, member lists
 *   - pool_edge [3P] on the external edges (community_pooling.py:200-201): relabel, drop
 *     self loops, sort by (row,col), merge duplicates with edge_attr summed
 *                                                               -> CSR1 / CSC1 / W1
 * edge_index  int64 [2,E] (global node ids, edges grouped by graph)
 * edge_attr   float [E] or NULL (one edge feature, as the reference supports)
 * batch       int64 [N] ascending graph id per node
 * cluster0    int64 [N]  per-graph cluster ids (any integers; made consecutive here);
 *             NULL = graph-only build (CSR0/CSC0/W0), used by the stand-alone conv layers
 * cluster1    int64 [L1] per-graph ids of the depth-0 clusters; L1 must equal sum C0_g;
 *             may be NULL (then only depth 0 is built: CL1.. untouched)
 * node_ptr / edge_ptr / c1_ptr  int32 [B+1] or NULL: per-graph offsets if the caller
 *             knows them (our DataLoader does); otherwise derived on the device.
 * max_nodes / max_edges: upper bounds on any single graph's size (used to size LDS);
 *             pass 0 if unknown (kernels then use their global-memory scratch path,
 *             scratch_i32 must hold drgnn_topology_scratch_elems() ints).
 */
int64_t drgnn_topology_scratch_elems(int64_t n_nodes, int64_t n_edges, int64_t n_graphs);
/* LDS bytes the builder needs for the given per-graph bounds; it runs out of LDS when this
 * is <= 160 KiB and max_nodes > 0, else out of scratch_i32. */
int64_t drgnn_topology_lds_bytes(int32_t max_nodes, int32_t max_edges);
int drgnn_topology_build(const int64_t* edge_index, const float* edge_attr,
                         const int64_t* batch, const int64_t* cluster0, const int64_t* cluster1,
                         const int32_t* node_ptr, const int32_t* edge_ptr, const int32_t* c1_ptr,
                         int64_t n_nodes, int64_t n_edges, int64_t len_cluster1, int64_t n_graphs,
                         int32_t max_nodes, int32_t max_edges,
                         int32_t* ws_i32, float* ws_f32, int32_t* scratch_i32, void* stream);

/* Exclusive scans CPTR0 / E1PTR / CPTR1 (only needed to materialise compact pooled
 * tensors for the function-level API: community_pooling(), max_pool_x()). */
int drgnn_topology_finalize(int32_t* ws_i32, int64_t n_nodes, int64_t n_edges,
                            int64_t n_graphs, void* stream);

/* status4[0] = OR of all status bits, status4[1] = first offending graph (or -1); this one
 * DOES synchronise the stream. */
int drgnn_topology_status(const int32_t* ws_i32, int64_t n_nodes, int64_t n_edges,
                          int64_t n_graphs, int32_t* status4, void* stream);

/* ---- fused network body ------------------------------------------------------------
 * One convolution branch of GINet / sGAT / FoutNet:
 *   conv1 -> relu -> community_pooling(max) -> conv2 -> relu -> max_pool_x -> graph mean
 * (ginet.py:103-114,133; sGAT.py:119-133; foutnet.py:108-120), one workgroup per
 * (graph, branch), intermediates in LDS.  The FC head (fc1/relu/dropout/fc2) stays
 * outside.  H1 = 16, H2 = 32 as hard-coded in the reference (ginet.py:87-92).
 *
 * Weight operands are described as strided [K,H] matrices so that each model's own
 * parameter layout is used in place: element (k,h) = ptr[k*sk + h*sh].
 *   GINet   nbr = fc.weight [H,F]           (sk=1, sh=F)   self = NULL   bias = NULL
 *   sGAT    nbr = weight[F:2F,:], self = weight[0:F,:]     (sk=H, sh=1)  bias [H]
 *   FoutNet nbr = Wn, self = Wc  [F,H]                     (sk=H, sh=1)  bias [H]
 */
typedef struct drgnn_conv_params {
    const float* w_nbr;  int64_t nbr_sk, nbr_sh;
    const float* w_self; int64_t self_sk, self_sh;   /* NULL for GINet */
    const float* bias;                                /* NULL for GINet */
} drgnn_conv_params;

typedef struct drgnn_conv_grads {       /* same striding as the parameters; NULL = skip */
    float* w_nbr;
    float* w_self;
    float* bias;
} drgnn_conv_grads;

#define DRGNN_MAX_BRANCH 2

typedef struct drgnn_net_desc {
    int32_t kind;          /* DRGNN_GINET / DRGNN_SGAT / DRGNN_FOUT                    */
    int32_t n_branch;      /* 2 for GINet (conv*, conv*_ext), else 1                   */
    int32_t n_feat;        /* F: input node features                                    */
    int32_t reserved;
    drgnn_conv_params conv1[DRGNN_MAX_BRANCH];
    drgnn_conv_params conv2[DRGNN_MAX_BRANCH];
} drgnn_net_desc;

/* Saved-for-backward tensors, all in the padded per-graph layout, per branch b:
 *   xp   float [n_branch][N][16]   pooled node features (input of conv2)
 *   arg0 int32 [n_branch][N][16]   local node id that won the depth-0 max, -1 = no grad
 *   arg1 int32 [n_branch][N][32]   local depth-0 cluster that won the depth-1 max, -1 = no grad
 * readout float [B][32*n_branch]   per-graph mean of the depth-1 pooled features
 */
/* max_nodes / max_edges / max_c0: upper bounds on any single graph's node count, edge count
 * and number of depth-0 clusters (max_c0 = 0: unknown -> max_nodes).  They size the LDS
 * carve (forward and backward differ); when it exceeds 160 KiB (or max_nodes == 0) the
 * kernels run out of `scratch_f32` (global, drgnn_net_scratch_elems() floats) instead. */
int64_t drgnn_net_lds_bytes(int32_t kind, int32_t n_feat, int32_t max_nodes, int32_t max_edges,
                            int32_t max_c0, int32_t backward);

int drgnn_net_forward(const drgnn_net_desc* net, const float* x,
                      const int32_t* ws_i32, const float* ws_f32,
                      int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                      int32_t max_nodes, int32_t max_edges, int32_t max_c0,
                      float* xp, int32_t* arg0, int32_t* arg1, float* readout,
                      float* scratch_f32, int32_t* step_inc /* optional: ++*step_inc once */,
                      void* stream);

/* Backward of the above.  grad_readout float [B][32*n_branch].  Every workgroup writes its
 * graph's parameter-gradient contribution into `partials` (float [n_graphs*n_branch][P],
 * P = drgnn_net_partial_elems(); K x H row-major blocks
 * [dW1nbr F*16][dW1self F*16][db1 16][dW2nbr 16*32][dW2self 16*32][db2 32]) and, when grad_x
 * is given, d loss / d x per branch into grad_x float [n_branch][N][F]. */
int64_t drgnn_net_partial_elems(int32_t kind, int32_t n_feat);
int64_t drgnn_net_scratch_elems(int32_t kind, int32_t n_feat, int64_t n_nodes, int64_t n_edges,
                                int64_t n_graphs);
int drgnn_net_backward(const drgnn_net_desc* net, const float* x, const float* grad_readout,
                       const int32_t* ws_i32, const float* ws_f32,
                       int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                       int32_t max_nodes, int32_t max_edges, int32_t max_c0,
                       const float* xp, const int32_t* arg0, const int32_t* arg1,
                       float* grad_x, float* partials, float* scratch_f32,
                       int32_t* step_inc /* optional: ++*step_inc once per launch */, void* stream);

/* Fixed-order (deterministic) sum of the per-graph partials into the strided gradient
 * tensors (overwritten, not accumulated); with grad_x, branches 1.. are summed into
 * branch 0.  Replaces the scatter-add autograd performs for the shared weights. */
int drgnn_net_reduce_grads(const drgnn_net_desc* net, const float* partials, int64_t n_nodes,
                           int64_t n_graphs, drgnn_conv_grads* g_conv1, drgnn_conv_grads* g_conv2,
                           float* grad_x, void* stream);

/* ---- stand-alone layers and pooling functions (the reference's function-level API) ----------
 * For custom nets built from the reference's layers (README "custom GNN" snippet).  A single
 * convolution of arbitrary width H <= 128 on ONE graph described by a graph-only topology
 * workspace (drgnn_topology_build with n_graphs = 1, cluster0 = NULL):
 *   GINetConvLayer.forward (ginet.py:50-73), sGraphAttentionLayer.forward (sGAT.py:62-93),
 *   FoutLayer.forward (foutnet.py:56-82).  `u` / `du` are [N, H] (GINet) or [N, 2H] scratch;
 *   partials holds drgnn_conv_layer_slabs(N) * drgnn_conv_layer_partial_elems() floats.
 */
int64_t drgnn_conv_layer_slabs(int64_t n_nodes);
int64_t drgnn_conv_layer_partial_elems(int32_t kind, int32_t F, int32_t H);
int drgnn_conv_layer_forward(int32_t kind, const float* x, int64_t n_nodes, int32_t F, int32_t H,
                             const drgnn_conv_params* p, const int32_t* ws_i32, const float* ws_f32,
                             int64_t n_edges, float* u, float* out, void* stream);
int drgnn_conv_layer_backward(int32_t kind, const float* x, int64_t n_nodes, int32_t F, int32_t H,
                              const drgnn_conv_params* p, const int32_t* ws_i32, const float* ws_f32,
                              int64_t n_edges, const float* grad_out, float* du, float* partials,
                              const drgnn_conv_grads* g, float* grad_x, void* stream);
/* Cluster pooling over the depth-0 member lists of a FINALIZED topology workspace:
 * op 0 = max with argmax (scatter_max inside community_pooling.py:197 / max_pool_x [3P]; first
 * maximum in member order, empty cluster -> 0 / arg = N), op 1 = mean (scatter_mean,
 * community_pooling.py:212).  out [C0_total, H] compact, arg = GLOBAL node id. */
int drgnn_segpool_forward(const int32_t* ws_i32, int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                          const float* x, int32_t H, int32_t op, float* out, int64_t* arg, void* stream);
int drgnn_segmax_backward(const float* grad_out, const int64_t* arg, int64_t n_clusters, int32_t H,
                          int64_t n_nodes, float* grad_x /* zero-filled */, void* stream);
/* pool_edge [3P] result of a FINALIZED workspace in the reference's form: edge_index int64
 * [2, e1_total] (consecutive global cluster ids, sorted by (row, col)), edge_attr [e1_total]. */
int drgnn_pooled_edges_export(const int32_t* ws_i32, const float* ws_f32, int64_t n_nodes, int64_t n_edges,
                              int64_t n_graphs, int64_t e1_total, int64_t* edge_index, float* edge_attr,
                              void* stream);
/* get_preloaded_cluster (community_pooling.py:25-30): cluster[batch == g] += running offset, in
 * place, no host round trips.  scratch: n_graphs + 1 int64. */
int drgnn_cluster_offset(int64_t* cluster, const int32_t* node_ptr, int64_t n_graphs, int64_t* scratch,
                         void* stream);

/* ---- dense head, loss and optimiser (the rest of one training step) -----------------------
 * What the reference trainer runs around the message-passing body for every mini-batch
 * (NeuralNet.py:489-506): the FC head of the nets (ginet.py:136-139, sGAT.py:134-135,
 * foutnet.py:121-122: fc1 -> relu -> dropout(p) -> fc2), MSELoss / (weighted)
 * CrossEntropyLoss with mean reduction (NeuralNet.py:239-263), their backward, and the Adam
 * update (NeuralNet.py:183-184, torch defaults).  torch.nn.Linear layouts: w1 [H,R], b1 [H],
 * w2 [O,H], b2 [O].
 */
#define DRGNN_TASK_REG   0
#define DRGNN_TASK_CLASS 1
/* DRGNN_TASK_GRAD -- the autograd boundary (NeuralNet.py:493-502: pred = model(batch); loss = loss_fn(pred, y); loss.backward()):
 * the loss lives OUTSIDE the library, `target` is float [B, O] = d loss / d pred as the caller's autograd hands it over, and
 * the launch back-propagates exactly that (the loss slot of the head slabs is written as 0).  With transform_sigmoid the
 * upstream gradient is taken with respect to the transformed prediction.  Fused step launches of the aggregation-first
 * family on a per-mini-batch workspace only (drgnn_net_train_step; DRGNN_E_ARG elsewhere). */
#define DRGNN_TASK_GRAD  2
typedef struct drgnn_head_desc {
    int32_t R, H, O;          /* readout width, hidden width, outputs (O <= 16)              */
    int32_t task;             /* DRGNN_TASK_REG: target float [B]; _CLASS: target int64 [B]   */
    int32_t train;            /* 1: dropout + loss + gradients; 0: predictions only (dropout off);
                                 2 (fused step launches only): the FORWARD of a training step -- predictions only, dropout ON
                                 with the mask of optimiser step step2[0], i.e. the mask a train = 1 launch draws until
                                 step2[0] is committed (model(batch) in training mode, its backward being a later launch) */
    float   p_drop;           /* dropout probability (GINet 0.4, others 0)                    */
    uint32_t seed;            /* dropout stream seed (mixed with the device step counter)     */
    int32_t transform_sigmoid; /* regression only: pred = sigmoid(fc2 output) before the loss (reference
                                  NeuralNet.format_output, NeuralNet.py:616-631); predictions are reported transformed */
    const float* w1; const float* b1; const float* w2; const float* b2;
    const float* class_w;     /* [O] class weights or NULL                                    */
    const float* drop_mask;   /* NULL (product): the counter-hash dropout stream.  Otherwise float [B, H] of 0 / 1: hidden unit h
                                 of the launch's graph g is kept iff drop_mask[g*H + h] != 0 and scaled by 1 / (1 - p_drop) --
                                 exactly F.dropout's arithmetic (ginet.py:138) with the mask given, so that a dropout-on launch
                                 can be compared element-wise with the oracle (tests; fused step kernels only)      */
} drgnn_head_desc;

/* The arguments of drgnn_topology_build bundled, to ask a body launch to ALSO build the topology
 * of the NEXT mini-batch in the same launch (its workgroups are appended to the grid).  The two
 * jobs are independent -- the builder only reads index tensors -- so one hides behind the other and
 * a kernel boundary disappears (software pipelining across training steps).  Falls back to
 * separate launches when LDS does not fit or the per-graph offsets are not supplied. */
/* The dataset resident in HBM, graph-major (described at drgnn_collate below). */
typedef struct drgnn_graph_set {
    int64_t n_graphs, n_nodes, n_edges, len_cluster1;
    int32_t n_feat, y_bytes;
    const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* c1_ptr;   /* c1_ptr null: no cluster1 */
    const float* x; const int64_t* edge_index; const float* edge_attr;          /* edge_attr may be null */
    const int64_t* cluster0; const int64_t* cluster1; const void* y;            /* each may be null */
} drgnn_graph_set;
typedef struct drgnn_topology_request {
    const int64_t* edge_index; const float* edge_attr; const int64_t* batch;
    const int64_t* cluster0; const int64_t* cluster1;
    const int32_t* node_ptr; const int32_t* edge_ptr; const int32_t* c1_ptr;
    int64_t n_nodes, n_edges, len_cluster1, n_graphs;
    int32_t max_nodes, max_edges;
    int32_t* ws_i32; float* ws_f32; int32_t* scratch_i32;
    /* Resident-set mode (set != NULL; the five tensor pointers above are ignored): slot g of the mini-batch is
     * graph ids[g] of `set`, whose index data is read in place (local ids, no collate); node_ptr / edge_ptr /
     * c1_ptr are the mini-batch's slot offset tables (drgnn_batch_offsets) and are required.  The builder also
     * gathers the slots' node features into x_out [n_nodes, F] and targets into y_out [n_graphs] (either may be
     * NULL).  Pooled edge weights are built when ws_f32 and set->edge_attr are both given. */
    const drgnn_graph_set* set; const int32_t* ids; float* x_out; void* y_out;
    int32_t flags, reserved;      /* DRGNN_TOPO_* below */
    /* DRGNN_TOPO_TILES: node features the level-0 aggregation is formed from -- x [n_nodes, n_feat] of the mini-batch (NULL in
     * resident-set mode: the set's x) -- and where it goes: tiles [drgnn_topology_tiles_elems(n_nodes, n_feat)] */
    const float* x; float* tiles;
    int32_t n_feat, reserved2;
} drgnn_topology_request;
/* request flags.  DRGNN_TOPO_HIER: also build the hierarchical node order (DRGNN_TI_HORD / HMP0 / HSPLIT; needs cluster1) --
 * what the node-split step kernels of the single-branch nets consume (4 more phases on the builder's member-list chain, so
 * callers that never run those kernels -- GINet -- leave it out).  drgnn_topology_build always builds it. */
#define DRGNN_TOPO_HIER 1
/* DRGNN_TOPO_LEAN (with DRGNN_TOPO_HIER and cluster1): build ONLY what the aggregation-first training kernels read
 * (csrc/drgnn_step2.h, drgnn_step3.h): ROWPTR0 / COL0 / EID0 (+ W0), CL0 / NC0, ROWPTR1 / COL1 / NE1 (+ W1), COLPTR1 / ROWIDX1
 * (+ TSLOT1 with edge weights), CL1 / NC1 / MPTR1 / MEM1, HORD / HMP0 / HSPLIT.  NOT built: CSC0 (COLPTR0 / ROWIDX0 / TSLOT0)
 * and the depth-0 member lists (MPTR0 / MEM0) -- those arrays keep whatever an earlier build left there.  The builder then
 * runs two short chains (8 barrier-separated phases each instead of ~19: one concatenated scan for the row pointers and
 * both cluster rankings, orders by counting instead of bucket sorts, the pooled CSC from a transposed bitmap), which keeps
 * it hidden behind the step workgroups it is co-launched with.  A launch that is not an aggregation-first training step
 * refuses a workspace built this way (drgnn_step_hints.topo_flags): DRGNN_E_ARG. */
#define DRGNN_TOPO_LEAN 2
/* DRGNN_TOPO_TILES (with DRGNN_TOPO_HIER): the builder also forms the LEVEL-0 NEIGHBOUR AGGREGATION of every node -- it depends
 * on the inputs only (node features, edges, edge weights), not on a parameter -- so that the training step of the mini-batch
 * starts from it instead of gathering x rows over edge_index inside the step kernel: the aggregation rides in the builder's
 * workgroups of the PREVIOUS launch like the topology itself (cached-topology mode: it is formed once per graph).  Layout of
 * `tiles` (node order, n = n_nodes of the workspace, F = n_feat, TF = F rounded up to a multiple of 4: rows are zero padded so
 * that the step kernels load them with 128-bit requests whatever the feature count):
 *     S [n][TF]  S_i = sum over the edges e = (i, j) in edge-id order of [w_e] x_j     (w_e: with edge weights only)
 *     D [n]      1 / deg_i (without weights: 0 for an isolated node; with weights: 1 / max(deg_i, 1))
 *     C [n]      with weights: mean edge weight of the row (sum_e w_e) D_i; without: 1
 *     X [n][TF]  only when F % 4 != 0: the node features, rows zero padded (what sGAT / FoutNet multiply with their self weights);
 *                starts at element n TF + (2 n rounded up to a multiple of 4): 16-byte aligned rows whatever the parity of n
 * GINetConvLayer (ginet.py:50-73) is relu(S W); FoutLayer (foutnet.py:56-82) relu(D (S Wn) + x Wc + b); sGraphAttentionLayer
 * (sGAT.py:62-93) relu(D (S Wn) + C (x Ws) + b).  Needs drgnn_topology_tiles_ok() and, when F % 4 == 0, 16-byte aligned x. */
#define DRGNN_TOPO_TILES 4
/* elements of a tiles buffer / 1 when the builder can form tiles for graphs of these bounds (its LDS holds an x tile then) */
int64_t drgnn_topology_tiles_elems(int64_t n_nodes, int32_t n_feat);
int32_t drgnn_topology_tiles_ok(int32_t max_nodes, int32_t max_edges, int32_t n_feat);
/* The same tiles from a workspace that is already built (its CSR0, and with use_weights its W0): a second flavour for a
 * workspace shared by nets with and without edge weights (a resident set's cached topology).  x [n_nodes, n_feat]: the node
 * features the workspace's graphs are laid out over.  Own launch; not a hot path. */
int drgnn_topology_tiles(const int32_t* ws_i32, const float* ws_f32, int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                         const float* x, int32_t n_feat, int32_t use_weights, float* tiles, void* stream);
/* drgnn_topology_build from a request (either mode), own launch. */
int drgnn_topology_build_request(const drgnn_topology_request* request, void* stream);
/* Slot offset tables of EVERY mini-batch of an epoch in one launch: mini-batch k = ids[k*batch_size, ...) gets
 * ptrs[k][0] = node offsets, ptrs[k][1] = edge offsets, ptrs[k][2] = cluster1 offsets, each batch_size+1 int32
 * (ptrs: [n_batches][3][batch_size+1]; a short last mini-batch uses a prefix of each row).  batch_size <= 4096. */
int drgnn_batch_offsets(const drgnn_graph_set* set, const int32_t* ids, int64_t n_ids, int32_t batch_size,
                        int32_t* ptrs, void* stream);

/* Backward of the body with the FC head, loss and their backward evaluated per graph INSIDE the
 * same launch (the head is row-wise), instead of taking grad_readout from drgnn_head_step:
 * reads readout [B,32*n_branch] (forward output) and the targets, writes pred [B,O], one head
 * partial slab per GRAPH (head_partials [B][drgnn_head_partial_elems]) and the conv partials.
 * Dropout stream id = *step - 1 (the forward launch of the same step has incremented it).
 * The launch keeps the head's weights in LDS when drgnn_net_head_stage_bytes() more than the backward's
 * drgnn_net_lds_bytes() still fit the LDS limit, and reads them from global memory otherwise. */
int64_t drgnn_net_head_stage_bytes(int32_t R, int32_t H, int32_t O);
int drgnn_net_backward_fused_head(const drgnn_net_desc* net, const drgnn_head_desc* head, const float* x,
                                  const float* readout, const void* target, const int32_t* step,
                                  const int32_t* ws_i32, const float* ws_f32, int64_t n_nodes,
                                  int64_t n_edges, int64_t n_graphs, int32_t max_nodes, int32_t max_edges,
                                  int32_t max_c0, const float* xp, const int32_t* arg0, const int32_t* arg1,
                                  float* pred, float* head_partials, float* grad_x, float* partials,
                                  float* scratch_f32,
                                  const drgnn_topology_request* next_topology /* optional */,
                                  void* stream);

/* One workgroup per tile of graphs (16 for B <= 512, else 64; drgnn_head_num_slabs()).  Writes pred [B,O]; when train: grad_readout [B,R]
 * (d loss / d readout for the mean loss over the B graphs) and one partial slab per workgroup
 * ([dW1 H*R][db1 H][dW2 O*H][db2 O][loss][weight], drgnn_head_partial_elems() floats).
 * `step` (device int32) selects the dropout stream; it is NOT modified here. */
int64_t drgnn_head_partial_elems(int32_t R, int32_t H, int32_t O);
int64_t drgnn_head_num_slabs(int64_t n_graphs);
/* Hidden units an INFERENCE drgnn_head_step of n_graphs keeps in LDS at a time: H when the head fits whole, fewer (a multiple
 * of 16) when the launch goes over the hidden units in passes, 0 when no pass fits.  A training launch takes a head only whole. */
int32_t drgnn_head_pass_units(int32_t R, int32_t H, int32_t O, int64_t n_graphs);
int drgnn_head_step(const drgnn_head_desc* head, const float* readout, const void* target,
                    int64_t n_graphs, const int32_t* step, float* pred, float* grad_readout,
                    float* partials, void* stream);
/* Fixed-order sum of the head partials into grad_block = [fc1.weight | fc1.bias | fc2.weight |
 * fc2.bias] (contiguous), the batch loss into *loss, and ++*step (the optimiser step count). */
int drgnn_head_reduce(const float* partials, int64_t n_graphs, int32_t R, int32_t H, int32_t O,
                      float* grad_block, float* loss, int32_t* step, void* stream);
/* torch.optim.Adam single-tensor semantics on flat fp32 buffers; *step must already count
 * this update (>= 1).  The hyper-parameters are doubles, as torch keeps them: the bias corrections are formed
 * from them in double, and 1 - beta1, 1 - beta2, lr / bc1 and sqrt(bc2) reach the fp32 arithmetic rounded once. */
int drgnn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                    const int32_t* step, int64_t n, double lr, double beta1, double beta2, double eps,
                    double weight_decay, void* stream);

/* Single-launch parameter update for one process: fixed-order reduction of the conv partials
 * (as drgnn_net_reduce_grads) and of the head partials (as drgnn_head_reduce, without
 * touching the step counter), each reduced element immediately followed by its Adam update.
 * g_conv1/g_conv2 must point INTO flat_grad; head_offset = element offset of fc1.weight in
 * the flat buffers; *step must already count this update (the forward launch's step_inc).
 * apply_adam = 0 only produces the flat gradient + loss (data parallel: all-reduce, then
 * drgnn_adam_step).  weight_decay is not supported here (coupled L2: drgnn_adam_step; decoupled: drgnn_train_update_opt). */
int drgnn_train_update(const drgnn_net_desc* net, const float* conv_partials, int64_t n_graphs,
                       drgnn_conv_grads* g_conv1, drgnn_conv_grads* g_conv2,
                       const float* head_partials, int64_t head_slabs /* rows of head_partials */,
                       int32_t R, int32_t H, int32_t O, int64_t head_offset, float* flat_param, float* flat_grad, float* exp_avg,
                       float* exp_avg_sq, int64_t n_param, const int32_t* step, float* loss,
                       double lr, double beta1, double beta2, double eps, int32_t apply_adam, void* stream);

/* ---- fused training step --------------------------------------------------------------------
 * Body forward + FC head + loss + body backward of one mini-batch in ONE launch (every workgroup
 * keeps its graph, activations and argmax indices in LDS between the forward and the backward
 * half), optionally sharing the grid with the topology build of the NEXT mini-batch.  Replaces,
 * together with drgnn_step_update, the whole loop body of NeuralNet._epoch (NeuralNet.py:489-506:
 * zero_grad, model(batch), loss, backward, optimizer.step) for GINet / sGAT / FoutNet.
 *   step2     device int32[4], zero-initialised by the owner: [0] = optimiser steps completed (selects the dropout
 *             stream, read only); [1] = index of this step, written here (drgnn_step_update commits [0] = [1]);
 *             [2] = sticky fault bits (DRGNN_FAULT_*), only ever OR-ed into by the kernels; [3] reserved.
 *   readout   OUT [B, 32*n_branch]; pred OUT [B, O]
 *   head_partials OUT [B][drgnn_head_compact_elems]: [dhid H][dW_fc2 O*H][db_fc2 O][loss][weight]
 *             (dW_fc1 = dhid^T readout is formed by drgnn_step_update)
 *   partials  OUT [B*n_branch][drgnn_net_partial_elems]  (split layout: [B*2][...], one slab per half graph)
 *   xchg      uint64 [B][drgnn_net_step_xchg_elems], zero-filled ONCE by the caller and then left alone: the two
 *             branch workgroups of a GINet graph hand each other their 32 readout values through it, the two half-graph
 *             workgroups of the split layout their pooled rows (may be NULL when n_branch == 1 and no plan with wgs_per_graph == 2 is passed)
 * head->train == 0: inference -- forward + head only (dropout off), writes pred and readout; target,
 * head_partials and partials may be NULL and the step counters are left alone.
 * Needs max_nodes/max_edges/max_c0 bounds; returns DRGNN_E_CAPACITY when a graph of that size does
 * not fit the 160 KiB LDS (drgnn_net_step_lds_bytes): use drgnn_net_forward +
 * drgnn_net_backward_fused_head + drgnn_train_update then. */
/* ---- launch plan of the fused step ---------------------------------------------------------------------------------------
 * Which kernel family and launch layout a fused step of a given shape takes, as ONE function of the launch's description:
 * drgnn_net_step_plan() fills the `out` members from the `in` members, drgnn_net_train_step* and drgnn_train_epoch decide
 * through the same code, so a caller that sizes its buffers from a plan and passes that plan along (drgnn_step_hints.plan)
 * gets the layout it planned or an error, never a silent third one.
 *   family   DRGNN_STEP_FAMILY_AGGREGATE: csrc/drgnn_step2.h (sGAT / FoutNet) / drgnn_step3.h (GINet) -- conv1 starts from the
 *            aggregation tiles the topology builder formed (DRGNN_TOPO_TILES), rows in the builder's hierarchical order
 *            (DRGNN_TOPO_HIER); padded feature widths 16 / 32 / 48 / 64, the reference heads (fc1 width 128 / 64), training and
 *            inference launches.  DRGNN_STEP_FAMILY_NONE: no fused kernel covers the launch -- a graph beyond the LDS budget,
 *            more than 64 features, a head that is not the reference's, a workspace without hierarchical order / tiles (use
 *            drgnn_net_forward + drgnn_net_backward_fused_head).  DRGNN_STEP_FAMILY_PRODUCT: the host emulation's stand-in (the
 *            CPU test suite's build, which has no aggregation-first kernels); never returned by the device library.
 *   wgs_per_graph  GINet (ginet.py:99-141: two branches over the same edge_index): 2 = one workgroup per branch, readouts
 *            exchanged, taken ONLY while all 2 * n_graphs (+ the co-launched builder's) workgroups are resident at once (one
 *            workgroup per CU: HIP promises nothing about dispatch order); 1 = both branches in one workgroup, no cross-workgroup
 *            wait.  sGAT / FoutNet: 2 = the node-split layout (each workgroup owns the depth-1 clusters of one half of the graph;
 *            training launches of the aggregation-first family under the same residency rule); 1 otherwise.
 *   slabs_per_graph  conv gradient slabs per graph in `partials` (what drgnn_step_update must be told)
 *   width    the padded feature width of the specialised kernel instance, 0 = the generic instance
 *   cls      1: the instance with the compile-time LDS layout of the capacity class (200 nodes, 1024 edges, 52 depth-0 clusters
 *            per graph; 32-wide kernels and the 48-wide aggregation-first training kernels) -- the same arithmetic in the same
 *            order, bit-identical results
 *   lean_ok  1: the launch reads nothing a DRGNN_TOPO_LEAN build leaves out
 *   builder_wgs_per_graph  of the topology the same launch builds: 2 / 1; 0 = it gets a launch of its own
 *   lds_bytes  LDS one workgroup needs (<= 160 KiB whenever family != NONE); xchg_words: uint64 exchange words per graph
 *   from_memory  1: graphs beyond the LDS budget of the staged kernels (200 - 270 nodes, by width) -- the instance that reads the
 *            node-sized input tile from memory (L2) where it is used instead of staging it: GINet's one-workgroup kernel with the S
 *            rows of the tiles left in memory, sGAT / FoutNet with the x rows -- and, where that is not enough, the S rows too --
 *            left in memory; run-time LDS layout; every net and width up to ~400 nodes / 2048 edges per graph.  Beyond what the
 *            builder stages an x tile for (drgnn_topology_tiles_ok) the tiles come from drgnn_topology_tiles on the built workspace
 * Overrides (0 = automatic; tests and same-box A/B runs): force_wgs 1 / 2 = always that many workgroups per graph (2 beyond the
 * resident size is MEASUREMENT ONLY: the exchange then leans on in-order dispatch; bounded wait + fault bit); no_class;
 * no_aggregate (never the aggregation-first family: family NONE on the device, the launch pair steps the mini-batch);
 * no_split (sGAT / FoutNet never divided); no_paired is ignored (kept for the ABI).  The environment variable
 * DRGNN_STEP_PLAN (comma list of one, two, noclass, product, nosplit; read once) sets the defaults of a process for plans
 * that override nothing. */
#define DRGNN_STEP_FAMILY_NONE 0
#define DRGNN_STEP_FAMILY_PRODUCT 1
#define DRGNN_STEP_FAMILY_AGGREGATE 2
typedef struct drgnn_step_plan {
    /* in: the launch */
    int32_t kind, n_feat, max_nodes, max_edges, max_c0, R, H, O;
    int64_t n_graphs;
    int64_t co_built_graphs;   /* graphs of the topology the same launch builds for the next mini-batch (0: none) */
    int32_t train;             /* 1: training launch; 0: inference */
    int32_t topo_flags;        /* DRGNN_TOPO_* flags of the workspace the launch READS.  DRGNN_TOPO_TILES only if it comes with
                                  tiles of this kind's flavour (sGAT: weighted sums) and x is 16-byte aligned */
    /* in: overrides */
    int32_t force_wgs, no_class, no_aggregate, no_split, no_paired;
    /* out */
    int32_t family, wgs_per_graph, slabs_per_graph, width, cls, lean_ok, builder_wgs_per_graph;
    int64_t lds_bytes, xchg_words;
    int32_t from_memory, reserved;   /* (ABI 4) 1: the instance that leaves the node-sized input tile in memory */
} drgnn_step_plan;
/* Returns wgs_per_graph (0: family NONE).  Host-side only. */
int32_t drgnn_net_step_plan(drgnn_step_plan* plan);

/* Host-known offsets / sizes of the mini-batch's graphs (Batch.from_data_list and the resident set record them): for up to
 * 64 graphs they travel in the kernel arguments, so a workgroup need not fetch them from the workspace
 * first (one dependent memory round trip less).  All members optional. */
typedef struct drgnn_step_hints {
    const int32_t* host_node_ptr; const int32_t* host_edge_ptr;       /* per mini-batch (drgnn_net_train_step) */
    const int64_t* set_node_ptr; const int64_t* set_edge_ptr; const int32_t* host_ids;   /* cached mode */
    /* topo_flags: the DRGNN_TOPO_* flags the topology workspace was BUILT with -- what the caller vouches for (0: a caller
     *             that knows nothing of the hierarchical order: no fused kernel, DRGNN_E_CAPACITY) */
    int32_t topo_flags, reserved;
    /* DRGNN_TOPO_TILES in topo_flags: the aggregation tiles the builder formed for this workspace (DEVICE memory, laid out
     * for the workspace's node count): the aggregation-first kernels start conv1 from them. */
    const float* tiles;
    /* the plan the caller sized `partials` (slabs_per_graph) and `xchg` (xchg_words) from, and its overrides.  NULL: no
     * overrides, and a single-branch net is never divided between two workgroups (one slab per graph).  A launch that
     * cannot take the plan's wgs_per_graph returns DRGNN_E_CAPACITY. */
    const drgnn_step_plan* plan;
    /* cached-topology launches (drgnn_net_train_step_cached) only, optional: the graph numbers of the NEXT mini-batch (DEVICE
     * memory, n_next of them).  While the launch leaves CUs idle, one extra workgroup per such graph requests everything its
     * step will stage, so that the next launch finds it in the L2 of the XCD that steps it (no effect on any result; numbers
     * outside the cached set are skipped). */
    const int32_t* next_ids; int64_t n_next;
} drgnn_step_hints;
/* uint64 exchange words per graph the fused step needs for these bounds (GINet: n_branch x max(H, 32); the split layout
 * of sGAT / FoutNet: two hand-offs of max_c0 x 16 values per half + the partial readouts) */
int64_t drgnn_net_step_xchg_elems(int32_t kind, int32_t max_nodes, int32_t max_c0, int32_t H);
int64_t drgnn_net_step_lds_bytes(int32_t kind, int32_t n_feat, int32_t max_nodes, int32_t max_edges,
                                 int32_t max_c0, int32_t R, int32_t H, int32_t O);
int64_t drgnn_head_compact_elems(int32_t R, int32_t H, int32_t O);
/* drgnn_net_step_lds_bytes / drgnn_net_step_variant describe the retired product-first step kernel of rounds 2 - 3 (kept in
 * the ABI for hosts that query them): its LDS bytes per workgroup, and the padded feature width (16/32/48/64) of the
 * width-specialised instance a launch of these bounds would have taken, or 0 for the generic one.  The library's launches
 * are described by drgnn_net_step_plan (lds_bytes / width / cls).  Host-side only. */
int32_t drgnn_net_step_variant(int32_t kind, const float* x, int32_t n_feat, int32_t max_nodes, int32_t max_edges,
                               int32_t max_c0, int32_t H, int32_t O);
int drgnn_net_train_step(const drgnn_net_desc* net, const drgnn_head_desc* head, const float* x,
                         const void* target, int32_t* step2, const int32_t* ws_i32, const float* ws_f32,
                         int64_t n_nodes, int64_t n_edges, int64_t n_graphs, int32_t max_nodes,
                         int32_t max_edges, int32_t max_c0, float* pred, float* readout,
                         float* head_partials, float* partials, uint64_t* xchg,
                         const drgnn_topology_request* next_topology /* optional */,
                         const drgnn_step_hints* hints /* optional */, void* stream);
/* drgnn_train_update for the slabs of drgnn_net_train_step: also forms dW_fc1 from head_partials'
 * dhid rows and readout, applies Adam with step index step2[1] and commits step2[0] = step2[1]
 * (also when apply_adam = 0: data parallel, all-reduce + drgnn_adam_step(step2) follow). */
/* slabs_per_graph: conv slabs per graph in conv_partials -- 0 = n_branch (every layout but one); 2 for the split layout of a
 * single-branch net (drgnn_step_plan.slabs_per_graph of the plan the launch was given). */
int drgnn_step_update(const drgnn_net_desc* net, const float* conv_partials, int64_t n_graphs,
                      drgnn_conv_grads* g_conv1, drgnn_conv_grads* g_conv2, const float* head_partials,
                      const float* readout, int32_t R, int32_t H, int32_t O, int64_t head_offset,
                      float* flat_param, float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_param,
                      int32_t* step2, float* loss, double lr, double beta1, double beta2, double eps,
                      int32_t apply_adam, int32_t slabs_per_graph, void* stream);

/* The gradient half of drgnn_step_update alone, for a caller whose optimiser lives outside the library (the drop-in boundary:
 * an unchanged NeuralNet._epoch runs torch.optim.Adam over model.parameters(), NeuralNet.py:183-184,502-503): fixed-order sum of
 * the conv slabs into g_conv1 / g_conv2 and of the head slabs (+ dW_fc1 = dhid^T readout) into head_grad = [fc1.weight |
 * fc1.bias | fc2.weight | fc2.bias] (contiguous), no parameter update.
 *   graph_weight  NULL, or float [n_graphs]: slab g enters the sum multiplied by graph_weight[g].  Every quantity of a graph's
 *                 slab is linear in d loss / d pred_g, so a DRGNN_TASK_GRAD launch with O = 1 and an upstream gradient of ONE
 *                 leaves d pred_g / d theta in the slabs, and this call with graph_weight = d loss / d pred contracts them with
 *                 the real gradient of ANY loss: model(batch) is one launch, loss.backward() is this one.
 *   zero_ptr / zero_len  up to DRGNN_ZERO_RANGES float ranges filled with 0 by the same launch (parameters the step kernels
 *                 never touch: GINetConvLayer's fc_attention / fc_edge_attr, whose gradient is identically 0, ginet.py:63-66)
 *   step2         optional: commit step2[0] = step2[1] (a new dropout stream for the next step), as drgnn_step_update does. */
#define DRGNN_ZERO_RANGES 8
int drgnn_step_gradients(const drgnn_net_desc* net, const float* conv_partials, int64_t n_graphs,
                         drgnn_conv_grads* g_conv1, drgnn_conv_grads* g_conv2, const float* head_partials,
                         const float* readout, int32_t R, int32_t H, int32_t O, float* head_grad,
                         const float* graph_weight, float* const* zero_ptr, const int64_t* zero_len, int32_t n_zero,
                         int32_t* step2, int32_t slabs_per_graph, void* stream);

/* ---- graclus ---------------------------------------------------------------------
 * Greedy maximal matching of every graph of a built topology (CSR0), the clustering the README's custom net
 * feeds to max_pool / max_pool_x (README.md:98-126; torch_geometric.nn.graclus -> torch_cluster, whose node
 * visiting order is a random permutation: pass it as `perm`, LOCAL ids per graph, to reproduce a given run;
 * NULL = identity).  An unmatched node takes its unmatched neighbour of largest weight (weight [E] indexed by
 * input edge id; NULL or ties: first in edge-id order); both are labelled min(u, v).  cluster [N] int64 receives
 * batch-global labels.  max_nodes / max_edges size the LDS carve (DRGNN_E_CAPACITY beyond 160 KiB). */
int drgnn_graclus(const int32_t* ws_i32, int64_t n_nodes, int64_t n_edges, int64_t n_graphs, int32_t max_nodes,
                  int32_t max_edges, const float* weight, const int64_t* perm, int64_t* cluster, void* stream);

/* ---- offline clustering --------------------------------------------------------
 * Markov clustering of every graph of a batch: community_detection(edge_index, num_nodes,
 * method='mcl') (community_pooling.py:95-158; markov_clustering.run_mcl defaults), as PreCluster
 * runs it on the internal-contact graph (DataSet.py:77-86).  One workgroup per graph, dense fp64.
 * mat_ptr int64 [B+1] = prefix sums of N_g^2; mat_scratch 3 * mat_ptr[B] doubles; int_scratch
 * 4 * N ints; labels int64 [N] (per-graph cluster ids, the reference's numbering); info int32 [B]
 * = iterations used (negative: no convergence within 100). */
int drgnn_mcl(const int64_t* edge_index, int64_t n_edges, const int32_t* node_ptr, const int32_t* edge_ptr,
              const int64_t* mat_ptr, int64_t n_graphs, double* mat_scratch, int32_t* int_scratch,
              int64_t* labels, int32_t* info, void* stream);

/* Deterministic Louvain community detection of every graph of a batch: community_detection(edge_index,
 * num_nodes, method='louvain') (community_pooling.py:95-158; python-louvain best_partition, resolution 1) on
 * the unweighted graph, as PreCluster runs it on the internal-contact graph (DataSet.py:77-86).  Nodes are
 * visited in id order and ties go to the smallest community id (python-louvain draws random orders); labels
 * int64 [N] are per-graph local labels 0..k-1 in order of first appearance.  Each distinct pair {u, v} of a
 * graph's edge slice (either direction, any repetition) has weight 1; all arithmetic is exact int64.
 * info int32 [B, 2] = (recorded levels, total passes), (0, 0) for a graph without pairs, (-1, -1) for a graph
 * beyond max_nodes / max_edges (labels untouched); modularity [B] = Q of the result.  One 64-lane workgroup
 * per graph; max_nodes / max_edges (largest graph; edges counted as listed, so list each pair once to get the
 * most out of the carve, as the Python louvain_labels does) size its LDS carve, louvain_lds_words() in
 * drgnn_louvain.h: 4 * (199 + 6 * max_nodes + 8 * max(max_edges, 1)) bytes, DRGNN_E_CAPACITY beyond 160 KiB
 * (1 024 nodes with 4 096 pairs listed once fit).  No allocation, no synchronisation. */
int drgnn_louvain(const int64_t* edge_index, int64_t n_edges, const int32_t* node_ptr, const int32_t* edge_ptr,
                  int64_t n_graphs, int32_t max_nodes, int32_t max_edges, int64_t* labels, int32_t* info,
                  double* modularity, void* stream);

/* Evaluation scores of n predictions against their targets: the reference's Metrics (Metrics.py) and the ranking its
 * hitrate() / auc() read.  pred, y: float64 [n] on the device, 1 <= n <= 2^31 - 1.  `what` is a mask:
 *   DRGNN_METRICS_COUNTS      confusion counts (sklearn confusion_matrix(y, pred, labels)) and the first-read sums;
 *   DRGNN_METRICS_REGRESSION  also the second read (centred sums) and the median of |y - pred| (a stable sort);
 *   DRGNN_METRICS_RANKING     stable ascending argsort of pred into order int32 [n] (ties in index order, -0 == +0,
 *                             NaN last, as np.argsort(kind='stable')), reversed when direction = +1, and hits int64 [n]
 *                             = cumsum of gt[idx] along that ranking, gt = y binarised.
 * direction +1: 1 means x > threshold (fnat, bin_class); -1: 1 means x < threshold.  n_labels = 0: both vectors are
 * binarised that way (labels {0, 1}); n_labels = K in 1..8: labels label_lo .. label_lo + K - 1 as given, a value that is
 * not one of them is left out of the counts.
 * counts int64 [8 + 64]: [0] pairs with a non-finite value, [1] pairs with a finite non-integral value, [2] y values
 * among the labels, [3] P = number of gt == 1, [4] S = sum over i with gt[i] == 1 of idx[i] (the reference's AUC ranks
 * the argsort indices: AUC = (S + P - P(P + 1) / 2) / (P N)), [8 + K a + b] samples with y label a and pred label b.
 * scores float64 [16]: min y, min pred, sum y, sum r, sum |r|, sum r^2, max |r|, sum (log1p y - log1p pred)^2 (r = y -
 * pred), sum (y - ybar)^2, sum (r - rbar)^2, median |r|.  Sums combine per-workgroup partials in a fixed order; there are
 * no floating-point atomics, so the results repeat bit for bit.  workspace: drgnn_metrics_workspace_bytes(n) bytes
 * (about 20 n + 1 KiB per 4 096 samples).  No allocation, no synchronisation. */
#define DRGNN_METRICS_COUNTS     1
#define DRGNN_METRICS_REGRESSION 2
#define DRGNN_METRICS_RANKING    4
int64_t drgnn_metrics_workspace_bytes(int64_t n);
int drgnn_metrics(const double* pred, const double* y, int64_t n, int32_t what, int32_t direction, double threshold,
                  int32_t label_lo, int32_t n_labels, void* workspace, int64_t workspace_bytes, int64_t* counts,
                  double* scores, int32_t* order, int64_t* hits, void* stream);

/* ---- interface graphs from atom coordinates (drgnn_iface.h) ------------------------------------------
 * The geometric half of the reference's graph generation (ResidueGraph.get_graph, ResidueGraph.py:108-145; the contact
 * search, :272-316; the edge distance, :364-381) for a ragged batch of M complexes of two chains.  Atoms are sorted
 * by residue, residues by complex with chain A before chain B:
 *   xyz f32 [T,3]; atom_ptr i32 [R+1] atom range of each residue; res_ptr i32 [M+1] residue range of each complex;
 *   res_split i32 [M] first chain-B residue of each complex; res_type i32 [R] 0..19, or -1: non-standard residue.
 * The three offset tables are also given as HOST arrays (host_*): the grid, the tile and the argument checks come from
 * them, so nothing is read back from the device.
 * Rule: residues a of A and b of B are an interface pair when an atom pair has d^2 < contact_distance^2 (strict),
 * its dist the smallest atom distance; nodes are the standard residues of the pairs whose two residues are standard;
 * two nodes i < j of one chain with an atom pair at d^2 < internal_contact_distance^2 form an internal edge.
 * Order: nodes by (chain, residue), interface edges (A node, B node) and internal edges (i < j) sorted by their pair;
 * node ids are local to the complex.  d^2 comes from fp32 coordinate differences; results repeat bit for bit and do
 * not depend on the other complexes of the batch, on tile_atoms or on the workspace's size.
 * tile_atoms: B-chain atoms staged in LDS at a time (0: 4 096; raised to the largest residue, DRGNN_E_CAPACITY when
 * that is beyond 160 KiB).  workspace: drgnn_iface_workspace_bytes() of (M, the largest chain A, the largest chain B, R)
 * or more, 16-byte aligned: the dense min-d^2 matrix [M, max_res_a, max_res_b] f32, 16 + 16 bytes per residue, 12 per
 * complex.  M <= 65 535 and M * max_res_a * max_res_b <= 2^31 - 1 (the edge offsets are int32): split larger batches. */
typedef struct drgnn_iface_request {
    const float* xyz;
    const int32_t* atom_ptr;
    const int32_t* res_ptr;
    const int32_t* res_split;
    const int32_t* res_type;
    const int32_t* host_atom_ptr;      /* the same tables in host memory */
    const int32_t* host_res_ptr;
    const int32_t* host_res_split;
    int64_t n_atoms, n_residues, n_complexes;
    double contact_distance, internal_contact_distance;
    int32_t tile_atoms, reserved;
    void* workspace;
    int64_t workspace_bytes;
    int32_t* node_ptr;                 /* device i32 [M+1] each: written by drgnn_iface_count, read by drgnn_iface_fill */
    int32_t* edge_ptr;
    int32_t* iedge_ptr;
} drgnn_iface_request;

/* bytes of workspace for n_complexes complexes whose chains have at most max_res_a / max_res_b residues, n_residues
 * in all; -1: a negative argument.  Pure host. */
int64_t drgnn_iface_workspace_bytes(int64_t n_complexes, int64_t max_res_a, int64_t max_res_b, int64_t n_residues);

/* Spheres, interface pairs, node flags, internal pairs and the scans (five launches): leaves the prefix sums of the
 * complexes' node / interface-edge / internal-edge counts in node_ptr / edge_ptr / iedge_ptr.  The caller reads their
 * last entries to size the outputs of drgnn_iface_fill: the only synchronisation of a build.
 * DRGNN_E_ARG: a null pointer, an offset table that does not start at 0, decreases or ends elsewhere than n_atoms /
 * n_residues, a split outside its complex, a negative cut-off; DRGNN_E_CAPACITY: workspace_bytes too small, M beyond
 * 65 535, a dense matrix beyond 2^31 - 1 entries, a residue beyond the LDS tile.  Both without a launch.  No allocation, no synchronisation. */
int drgnn_iface_count(const drgnn_iface_request* req, void* stream);

/* The graphs, after drgnn_iface_count on the same request and workspace (one launch):
 *   node_residue i32 [N] residue index (into res_type) of each node; pos f32 [N,3] mean of the residue's atoms (an
 *   fp64 sum rounded once); chain i32 [N] 0 / 1; type i32 [N] res_type of the node;
 *   edge_index i64 [E,2], dist f32 [E]; internal_edge_index i64 [Ei,2], internal_dist f32 [Ei].
 * n_nodes / n_edges / n_iedges: the totals read from the ptr arrays (capacities: nothing is written beyond them). */
int drgnn_iface_fill(const drgnn_iface_request* req, int64_t n_nodes, int64_t n_edges, int64_t n_iedges,
                     int32_t* node_residue, float* pos, int32_t* chain, int32_t* type, int64_t* edge_index, float* dist,
                     int64_t* internal_edge_index, float* internal_dist, void* stream);

/* ---- docking scores of pose batches (drgnn_score.h) ---------------------------------------------------
 * The targets the reference writes in Graph.get_score (Graph.py:27-59, through pdb2sql's StructureSimilarity) for M
 * poses of one topology against one reference structure: irmsd, lrmsd, fnat, dockQ, bin_class, capri_class.  The
 * once-per-complex work is the caller's (deeprank_gnn_amd.interface.ScoreReference); its rules:
 *   matching   a decoy atom and a reference atom correspond when (chain, res_seq, atom name) are equal; unmatched
 *              atoms are ignored on both sides.  Backbone atoms: CA, C, N, O.
 *   fnat       a reference residue pair (a in A, b in B) exists when an atom pair of the reference lies at d <= 5.0 A,
 *              over all atoms; it is preserved in a pose when an atom pair of the pose's residues a, b lies at
 *              d^2 <= fnat_cutoff^2 (d^2 from fp32 coordinate differences, no contraction).  fnat = n_preserved /
 *              n_ref_pairs; pair_res lists the P <= n_ref_pairs pairs whose two residues exist in the decoy, as residue
 *              indices into atom_ptr: the others stay in the denominator.
 *   irmsd      zone 0: the matched backbone atoms of the residues of the reference pairs found at d <= 10.0 A.  The
 *              decoy is fitted onto the reference with the optimal proper rotation + translation; RMSD over the zone.
 *   lrmsd      zone 1: the matched backbone atoms of the long chain (more residues in the reference; A on a tie), zone 2:
 *              those of the short chain.  The fit is on zone 1, the RMSD over zone 2 under that transform.
 *   dockQ      (fnat + 1 / (1 + (irmsd / 1.5)^2) + 1 / (1 + (lrmsd / 8.5)^2)) / 3
 *   binclass   irmsd < 4.0;  capri_class: 5, lowered to 4, 3, 2, 1 while irmsd < 6.0, 4.0, 2.0, 1.0
 * Inputs (device unless host_*): xyz f32 [M,T,3] the poses, atoms in one order; zone_atom i32 [Z] atom indices of the
 * three zones back to back, zone_ptr i32 [4] (host only); zone_ref f64 [Z,3] the matched reference coordinates;
 * pair_res i32 [P,2]; atom_ptr i32 [R+1] atom range of each residue.  The index tables are also given as HOST arrays:
 * every check comes from them.  Outputs: scores f64 [M,4] irmsd, lrmsd (A), fnat, dockQ; classes i32 [M,2] binclass,
 * capri_class; n_preserved i32 [M].  Distances are in the unit of the coordinates (A).
 * Arithmetic: one pass over the zones' atoms gathers fp64 moments (sum p, sum q, sum |p|^2, sum |q|^2, sum p q^T) in a
 * fixed slot order, reduced by a fixed tree; the rotation is the largest eigenpair of Horn's 4 x 4 matrix (cyclic
 * Jacobi, fp64), the residual E0 - 2 lambda.  No floating-point atomics: a pose's result repeats bit for bit and does
 * not depend on M, on its place in the batch or on the run.  One workgroup per pose, one launch. */
typedef struct drgnn_score_request {
    const float* xyz;
    const int32_t* zone_atom;
    const double* zone_ref;
    const int32_t* pair_res;
    const int32_t* atom_ptr;
    const int32_t* host_zone_atom;     /* the index tables in host memory */
    const int32_t* host_zone_ptr;      /* [4], host only */
    const int32_t* host_pair_res;
    const int32_t* host_atom_ptr;
    int64_t n_poses, n_atoms, n_residues, n_pairs, n_ref_pairs;
    double fnat_cutoff;
    double* scores;
    int32_t* classes;
    int32_t* n_preserved;
} drgnn_score_request;

/* DRGNN_E_ARG, before any launch: a null pointer, an atom index outside [0, T) or a residue index outside [0, R), an
 * atom_ptr that does not start at 0, decreases or ends elsewhere than T, a zone_ptr that does not start at 0 or
 * decreases, a zone of fewer than 3 atoms, n_ref_pairs < 1, P > n_ref_pairs, a negative cut-off or count.
 * DRGNN_E_CAPACITY: M or 3 T beyond 2^31 - 1.  No allocation, no synchronisation. */
int drgnn_dock_scores(const drgnn_score_request* req, void* stream);

/* ---- lDDT and interface lDDT of pose batches (drgnn_lddt.h) ---------------------------------------------
 * The local distance difference test (Mariani et al. 2013) of M poses of one topology against one reference structure,
 * as integers: per pose and threshold the preserved reference pairs over all pairs, over the inter-chain ones and per
 * residue.  The once-per-complex work and the fp64 quotients are the caller's (deeprank_gnn_amd.interface.LddtReference,
 * lddt_scores); the rule (tests/lddt_ref.py states it in numpy; conventions at exact ties are this project's own):
 *   atoms      heavy atoms only, on both sides; a reference atom and a table atom correspond when (chain, res_seq, atom
 *              name) are equal.  Unmatched table atoms are ignored, unmatched reference atoms stay in the denominators.
 *   pairs      two reference heavy atoms on the table's two chains, of different residues (chain, res_seq), with
 *              d_ref < inclusion_radius (strict), d_ref = sqrt((dx dx + dy dy) + dz dz) in fp64 on the host
 *   preserved  at threshold t: lo = max(d_ref - t, 0), hi = d_ref + t, lo lo <= d2 <= hi hi with d2 = (dx dx + dy dy) +
 *              dz dz in fp64 from the pose's fp32 coordinates, every product and sum rounded on its own
 * Inputs (device unless host_*): xyz f32 [M,T,3]; the matched pairs as entries grouped by owning residue, every pair in
 * both directions: entry_ptr i32 [R+1], self_atom i32 [E] (an atom of the owning residue), other_atom i32 [E], d_ref f64
 * [E]; n_chain_a_atoms: the first atom of chain B (a pair is inter-chain when exactly one of its atoms lies before it);
 * thresholds[n_thresholds], increasing.  The index tables are also given as HOST arrays: every check comes from them.
 * poses_per_pass: 0 the library's choice (4 once such passes make 1 024 workgroups of 64 residues, else 1), 1 or 4 the
 * poses that share one pass over the entries (the counts do not depend on it).  Outputs: counts i32 [M,2,K] (all, inter-chain), each pair counted once; residue_counts i32 [M,R,2,K]
 * or NULL, a pair counted for both of its residues.  Everything is an integer: no floating-point atomics; a pose's counts
 * do not depend on M, on its place in the batch or on the run.  A clear, one launch per 65 535 passes, a halving launch. */
typedef struct drgnn_lddt_request {
    const float* xyz;
    const int32_t* entry_ptr;
    const int32_t* self_atom;
    const int32_t* other_atom;
    const double* d_ref;
    const int32_t* host_entry_ptr;     /* the index tables in host memory */
    const int32_t* host_self_atom;
    const int32_t* host_other_atom;
    int64_t n_poses, n_atoms, n_residues, n_entries, n_chain_a_atoms;
    double thresholds[8];
    int32_t n_thresholds, poses_per_pass;
    int32_t* counts;
    int32_t* residue_counts;
} drgnn_lddt_request;

/* DRGNN_E_ARG, before any launch: a null pointer, an entry_ptr that does not start at 0, decreases or ends elsewhere than
 * n_entries, an atom index outside [0, T), n_chain_a_atoms outside [0, T], n_thresholds outside 1..8, thresholds that are
 * negative or not increasing, poses_per_pass other than 0, 1 or 4, a negative count.  DRGNN_E_CAPACITY: M, 3 T or the entry
 * count beyond 2^31 - 1 (or R beyond 2^28).  No allocation, no synchronisation. */
int drgnn_pose_lddt(const drgnn_lddt_request* req, void* stream);

/* ---- buried surface area of residues (drgnn_bsa.h) -----------------------------------------------------
 * The reference's `bsa` node feature (tools/BSA.py, through freesasa's Lee-Richards method) for K chosen residues of a
 * ragged batch of M two-chain complexes laid out as for drgnn_iface_count: xyz f32 [T,3], atom_ptr i32 [R+1], res_ptr
 * i32 [M+1], res_split i32 [M].
 *   bsa(residue) = SASA_unbound(residue) - SASA_complex(residue); a SASA is the sum of the Lee-Richards areas of the
 *   residue's atoms: n_slices planes through the atom's expanded sphere (R = r + probe), slice k at z_i - R_i + delta
 *   (k + 1/2), delta = 2 R_i / n_slices, contributing R_i delta (2 pi - the union of the arcs its neighbours bury).
 * Two radius arrays f32 [n_radii] say who takes part: rad_complex in the complex (both chains), rad_unbound in the
 * residue's chain alone; 0: the atom is absent from that state.  Atom t reads entry t % n_radii (n_radii divides T:
 * poses of one topology share one table).  The radius tables of the reference are the caller's
 * (deeprank_gnn_amd.interface.bsa_radii).  Targets: target_res i32 [K] residue indices into atom_ptr, target_complex i32
 * [K] their complexes; only their atoms are evaluated, every atom of the state acts as a neighbour.
 * Outputs: out f64 [K,3] sasa_unbound, sasa_complex, bsa (A^2); status i32 [1], to be zeroed by the caller: bit 0 is
 * set when a residue met more than drgnn_bsa_capacity(1) candidate atoms around its bounding box or an atom more than
 * drgnn_bsa_capacity(0) neighbours; that residue's three outputs are NaN (DRGNN_E_CAPACITY, reported through status
 * because the call does not synchronise).
 * One workgroup per target, one launch.  Arc arithmetic fp32 (fp64 for nearly tangent circles), gaps summed as 2^-40 rad integers, areas and residue
 * sums fp64 in atom order: no floating-point atomics, a residue's bits do not depend on the batch, the target list, its
 * place or the run.  The offset and target tables are also given as HOST arrays: every check comes from them. */
typedef struct drgnn_bsa_request {
    const float* xyz;
    const int32_t* atom_ptr;
    const int32_t* res_ptr;
    const int32_t* res_split;
    const float* rad_complex;
    const float* rad_unbound;
    const int32_t* target_res;
    const int32_t* target_complex;
    const int32_t* host_atom_ptr;      /* the tables in host memory */
    const int32_t* host_res_ptr;
    const int32_t* host_res_split;
    const int32_t* host_target_res;
    const int32_t* host_target_complex;
    int64_t n_atoms, n_residues, n_complexes, n_targets, n_radii;
    double probe;
    int32_t n_slices, reserved;
    double* out;
    int32_t* status;
} drgnn_bsa_request;

/* the documented capacities: what = 0 neighbours of one atom (256), 1 candidate atoms of one residue, 2 the most
 * slices, 3 the most targets of one call (one workgroup each: the grid's limit); -1 otherwise.  Pure host. */
int32_t drgnn_bsa_capacity(int32_t what);

/* DRGNN_E_ARG, before any launch: a null pointer, an offset table that does not start at 0, decreases or ends elsewhere
 * than n_atoms / n_residues, a split outside its complex, a target outside its complex, n_radii that does not divide
 * n_atoms, a negative probe, n_slices < 1.  DRGNN_E_CAPACITY: n_slices beyond drgnn_bsa_capacity(2), n_targets beyond
 * drgnn_bsa_capacity(3) (split the call).  No allocation, no
 * workspace, no synchronisation. */
int drgnn_bsa_residues(const drgnn_bsa_request* req, void* stream);

/* ---- half-sphere exposure of residues (drgnn_hse.h) ---------------------------------------------------
 * The reference's `hse` node feature (Biopython's HSExposureCA, radius 12 A, offset 0: up, down, angle) for K chosen
 * residues of a ragged batch of M complexes laid out as for drgnn_bsa_residues: xyz f32 [T,3], atom_ptr i32 [R+1],
 * res_ptr i32 [M+1].  Atoms are found through bb i32 [n_rows,5]: the offsets of N, CA, C, CB inside the residue (-1:
 * absent) and flags (bit 0 a standard amino acid, bit 1 GLY, bit 2 the first residue of its chain); residue r reads row
 * r % n_rows (n_rows divides R: poses of one topology share one table; deeprank_gnn_amd.interface.hse_table).
 *   Links: residues r, r+1 are linked iff both are standard and have a CA, r+1 does not start a chain, and atom
 *   connect_a of r (a column of bb) and atom connect_b of r+1 exist and lie closer than connect_cutoff: (1, 1, 4.3) is
 *   Biopython's CaPPBuilder, (2, 0, 1.8) its PPBuilder.  Members: the residues linked on at least one side.
 *   direction 0: a residue linked on both sides has a value; b = unit(unit(c2 - c1) + unit(c2 - c3)) over the CAs of
 *   r-1, r, r+1; every other member o (with offset k > 0: outside the stretch of r's peptide within k positions of r)
 *   with |CA(o) - c2| < radius counts up when (CA(o) - c2).b > 0, else down; angle: between b and CB - CA, or for a GLY
 *   with N and C the N turned by -120 degrees about C - CA, else 0.  direction 1 (HSExposureCB): every member with that
 *   side-chain vector has a value, b is the vector itself, angle 0.
 * Targets: target_res i32 [K] residue indices into atom_ptr, target_complex i32 [K] their complexes, grouped into
 * n_tiles tiles by tile_ptr i32 [n_tiles+1]; the targets of a tile belong to ONE complex (one workgroup per tile: it
 * stages that complex's CAs once; the tile size changes no bit).
 * Outputs: out f64 [K,3] up, down, angle, a NaN row for a residue without a value; status i32 [1], to be zeroed by the
 * caller: bit 0 is set when a complex with targets has more than drgnn_hse_capacity(0) residues; its targets are NaN
 * rows (DRGNN_E_CAPACITY, reported through status because the call does not synchronise).
 * All decisions and the angle in fp64 on the fp32 coordinates, counts by integer popcounts: no floating-point atomics,
 * a residue's bits do not depend on the batch, the tiles, the target list, its place or the run.  The offset, target,
 * tile and bb tables are also given as HOST arrays: every check comes from them. */
typedef struct drgnn_hse_request {
    const float* xyz;
    const int32_t* atom_ptr;
    const int32_t* res_ptr;
    const int32_t* bb;
    const int32_t* target_res;
    const int32_t* target_complex;
    const int32_t* tile_ptr;
    const int32_t* host_atom_ptr;      /* the tables in host memory */
    const int32_t* host_res_ptr;
    const int32_t* host_bb;
    const int32_t* host_target_res;
    const int32_t* host_target_complex;
    const int32_t* host_tile_ptr;
    int64_t n_atoms, n_residues, n_complexes, n_targets, n_tiles, n_rows;
    double radius, connect_cutoff;
    int32_t offset, connect_a, connect_b, direction;
    double* out;
    int32_t* status;
} drgnn_hse_request;

/* the documented capacities: what = 0 residues of one complex (4096), 1 the most tiles of one call (one workgroup
 * each: the grid's limit); -1 otherwise.  Pure host. */
int32_t drgnn_hse_capacity(int32_t what);

/* DRGNN_E_ARG, before any launch: a null pointer, an offset table that does not start at 0, decreases or ends elsewhere
 * than n_atoms / n_residues / n_targets, a target outside its complex, a tile over two complexes, n_rows that does not
 * divide n_residues, a bb offset outside its residue, connect_a / connect_b outside 0..3, direction outside 0..1,
 * radius or connect_cutoff <= 0, offset < 0.  DRGNN_E_CAPACITY: n_tiles beyond drgnn_hse_capacity(1) (split the call).
 * No allocation, no workspace, no synchronisation. */
int drgnn_hse_residues(const drgnn_hse_request* req, void* stream);

/* ---- residue depth (drgnn_depth.h) --------------------------------------------------------------------
 * The reference's `depth` node feature (Biopython's residue depth: the mean, over a residue's atoms, of the distance to
 * the molecular surface) for K chosen residues of a ragged batch of M complexes laid out as for drgnn_bsa_residues: xyz
 * f32 [T,3], atom_ptr i32 [R+1], res_ptr i32 [M+1].  The surface is a dot surface of the solvent-accessible surface of
 * ALL atoms of the complex, restricted to its outer component (tests/depth_ref.py states the rule):
 *   radii f64 [n_radii], atom t reads entry t % n_radii (n_radii divides T: poses of one topology share one array); an
 *   atom of radius 0 takes no part in the surface, its depth is still measured.  R_i = r_i + probe.
 *   dots f64 [n_dots,3]: the unit vectors S_k (deeprank_gnn_amd.interface.depth_dots).  p_ik = x_i + R_i S_k is accessible
 *   when |p_ik - x_j|^2 >= R_j^2 for every other atom j of the complex with a radius.  Two accessible dots are linked when
 *   |p - q|^2 <= link^2; a component is labelled by its smallest dot id i n_dots + k.  components 0: the component with
 *   the most dots is kept, ties to the smallest label; 1: every accessible dot is kept.
 *   depth(atom) = sqrt(min over the kept dots of |x - p|^2) - probe (+inf when no dot is kept); depth(residue) = the mean
 *   over its atoms, summed in order (NaN for a residue without atoms).
 * Every product and sum in fp64 on the fp32 coordinates, one by one: the accessible set, the links and the labels are
 * integers that equal the float64 rule's, the depth has its bits.  No floating-point atomics; a residue's bits do not
 * depend on the batch, the target list, its place or the run.
 * Workspace: drgnn_depth_workspace(n_atoms, n_complexes, n_dots, offsets) bytes, 8-byte aligned, allocated by the caller,
 * contents undefined on entry.  After the call it holds (offsets[0..8], offsets[9] the size; a complex whose first atom
 * is a0 owns [a0 n_dots, (a0 + atoms) n_dots) of the per-dot arrays and fills the first cx_nd of it, in dot-id order):
 *   0 mask u64 [T, ceil(n_dots/64)] bit k of atom t: dot (t, k) is accessible    1 pos f64 [T n_dots, 3]
 *   2 id i32 [T n_dots] (t - a0) n_dots + k    3 label i32 [T n_dots] index within the complex of the component's first dot
 *   4 size i32 [T n_dots] (at a label: the dots of the component)    5 cnt i32 [T]    6 ptr i32 [T]
 *   7 cx_nd i32 [M] accessible dots    8 cx_outer i32 [M] the label kept (-1: all are kept, or there is none; -2: refused)
 * Outputs: out f64 [K]; status i32 [1], to be zeroed by the caller: bit 0 is set when a complex has more than
 * drgnn_depth_capacity(1) atoms x n_dots; its targets are NaN (DRGNN_E_CAPACITY, reported through status because the call
 * does not synchronise).  The offset and target tables are also given as HOST arrays: every check comes from them.
 * phases: a later launch reads what the earlier ones left in the workspace, so a caller may run 1 | 2 once and 4 again for
 * other targets of the same batch, or time the launches one by one; repeating a launch changes no bit. */
typedef struct drgnn_depth_request {
    const float* xyz;
    const int32_t* atom_ptr;
    const int32_t* res_ptr;
    const double* radii;
    const double* dots;
    const int32_t* target_res;
    const int32_t* target_complex;
    const int32_t* host_atom_ptr;      /* the tables in host memory */
    const int32_t* host_res_ptr;
    const int32_t* host_target_res;
    const int32_t* host_target_complex;
    int64_t n_atoms, n_residues, n_complexes, n_targets, n_radii;
    double probe, link;
    int32_t n_dots, components;
    int32_t phases;                    /* 0: the whole call; else a set of 1 dots, 2 components, 4 residues: only these launches */
    int32_t reserved;                  /* 0 */
    void* workspace;
    int64_t workspace_bytes;
    double* out;
    int32_t* status;
} drgnn_depth_request;

/* the documented capacities: what = 0 dots per atom (4096), 1 atoms x n_dots of one complex (4 194 304), 2 the most
 * targets, complexes and atoms / 16 of one call (one workgroup each: the grid's limit); -1 otherwise.  Pure host. */
int32_t drgnn_depth_capacity(int32_t what);

/* bytes of workspace for a call, -1 for counts the call refuses; offsets (may be null): int64 [10], see above.  Pure host. */
int64_t drgnn_depth_workspace(int64_t n_atoms, int64_t n_complexes, int32_t n_dots, int64_t* offsets);

/* DRGNN_E_ARG, before any launch: a null pointer, an offset table that does not start at 0, decreases or ends elsewhere
 * than n_atoms / n_residues, a target outside its complex, n_radii that does not divide n_atoms, n_dots < 1, probe <= 0,
 * link < 0, components outside 0..1, phases outside 0..7, a workspace that is not 8-byte aligned.  DRGNN_E_CAPACITY: n_dots, n_targets,
 * n_complexes or n_atoms beyond drgnn_depth_capacity, workspace_bytes too small.  Three launches, no allocation, no
 * synchronisation. */
int drgnn_depth_residues(const drgnn_depth_request* req, void* stream);

/* ---- clustering of poses by their fraction of common contacts (drgnn_fcc.h) ---------------------------
 * FCC clustering (Rodrigues et al. 2012; the rule of HADDOCK's cluster_fcc with the tie between equally connected
 * centres broken towards the smaller index) of M poses of one two-chain topology.  tests/fcc_ref.py states the rule.
 *
 * drgnn_pose_contacts: xyz f32 [M, T, 3], the COUNTED atoms of every pose (the caller leaves out hydrogens that do not
 * count), grouped into residues by atom_ptr i32 [R+1]; residues [0, n_chain_a) are chain 0, the rest chain 1.  Residue
 * pair (a, b) across the chains is a contact iff an atom pair lies at ((dx dx + dy dy) + dz dz) <= cut2 in fp32
 * without contraction, cut2 = (float)(cutoff * cutoff) with the product taken in fp64.  Outputs: bits u64 [M, nA, WB],
 * WB = ceil(nB / 64): bit b % 64 of word b / 64 of row a, the bits past nB zero; n_contacts i32 [M].  One workgroup
 * per pose, one launch.  atom_ptr is also given as a HOST array: every check comes from it. */
typedef struct drgnn_pose_contacts_request {
    const float* xyz;
    const int32_t* atom_ptr;
    const int32_t* host_atom_ptr;
    int64_t n_poses, n_atoms, n_residues, n_chain_a;
    double cutoff;
    uint64_t* bits;
    int32_t* n_contacts;
} drgnn_pose_contacts_request;

/* drgnn_pose_common: common[i, j] = the number of bits set in both bits_a[i] and bits_b[j] (rows of n_words words;
 * bits_b may be bits_a), i32 [n_a, n_b].  One launch. */
typedef struct drgnn_pose_common_request {
    const uint64_t* bits_a;
    const uint64_t* bits_b;
    int64_t n_a, n_b, n_words;
    int32_t* common;
} drgnn_pose_common_request;

/* drgnn_pose_cluster: from common i32 [M, M] and n_contacts i32 [M] (device arrays; common need not be symmetric):
 * fcc(i, j) = n_i == 0 ? 0 : (double)common[i, j] / (double)n_i; j is a neighbour of i iff i != j, fcc(i, j) >= cutoff_fcc
 * and fcc(j, i) >= cutoff_reverse (the caller's cutoff_fcc * strictness, formed once in fp64).  Outputs: neighbours u64
 * [M, ceil(M/64)] (bit j of row i) and transposed (bit j of row i: i is a neighbour of j), tail bits zero; then, greedily
 * over the alive poses: the centre is the alive pose with the most alive neighbours (the smallest index on a tie); with
 * fewer than min_size - 1 of them the loop stops; else the centre and its alive neighbours form cluster k and die.
 * labels i32 [M] (-1: in no cluster), centres / sizes i32 [M] of which the first n_clusters[0] are written, n_clusters
 * i32 [1].  Two launches, no host round trip. */
typedef struct drgnn_pose_cluster_request {
    const int32_t* common;
    const int32_t* n_contacts;
    int64_t n_poses;
    double cutoff_fcc, cutoff_reverse;
    int32_t min_size;
    uint64_t* neighbours;
    uint64_t* transposed;
    int32_t* labels;
    int32_t* centres;
    int32_t* sizes;
    int32_t* n_clusters;
} drgnn_pose_cluster_request;

/* the documented capacities: what = 0 residues of a complex, both chains (3072: their bounding spheres sit in LDS),
 * 1 poses on either side of one drgnn_pose_common call (16384: the output stays below 2^28 entries), 2 poses of one
 * drgnn_pose_cluster call (4096: the degrees and the member list sit in LDS); -1 otherwise.  Pure host. */
int32_t drgnn_fcc_capacity(int32_t what);

/* All three: DRGNN_E_ARG before any launch for a null request or pointer, a negative count, and
 *   contacts: n_chain_a outside [0, n_residues], an atom_ptr that does not start at 0, decreases or ends elsewhere than
 *             n_atoms, a cutoff that is not a positive number whose square fits fp32
 *   cluster:  cutoff_fcc or cutoff_reverse outside (0, 1], min_size < 1
 * DRGNN_E_CAPACITY beyond drgnn_fcc_capacity (split the call; clustering cannot be split).  No allocation, no workspace,
 * no synchronisation; empty inputs return 0 without a launch. */
int drgnn_pose_contacts(const drgnn_pose_contacts_request* req, void* stream);
int drgnn_pose_common(const drgnn_pose_common_request* req, void* stream);
int drgnn_pose_cluster(const drgnn_pose_cluster_request* req, void* stream);

/* ---- contact consensus of poses (drgnn_consensus.h) ----------------------------------------------------
 * The consensus of a set of poses of one two-chain topology, or of every group of it (CONSRANK; Oliva, Vangone and Cavallo
 * 2013): how many poses have each residue pair in contact, how well a pose agrees with that, and the contacts at least
 * min_count poses share.  Linear in the poses; integers from end to end.  tests/consensus_ref.py states the rule.
 *
 * Shared by the three calls: bits u64 [M, nA, WB] as drgnn_pose_contacts leaves them, nA = n_chain_a, nB = n_chain_b,
 * WB = ceil(nB / 64).  The bits of a row's last word at or past nB are ignored on input (never counted, never used as an
 * index) and zero on output.  Index lists are also given as HOST arrays: every check comes from them.
 *
 * drgnn_pose_contact_counts: a grouping as lists, order i32 [n_listed] of pose indices and group_ptr i32 [G+1] of offsets
 * into order; a pose may be listed in no group, in one, in several, or several times in one (it then counts as often).
 * Outputs: counts i32 [G, nA, nB], counts[g, a, b] = the listed poses of g with bit (a, b) set; residues i32 [G, nA+nB]: for
 * r < nA the listed poses of g with any bit in row r, for r >= nA those with bit (a, r - nA) set for some a (poses, not
 * contacts).  A group without listed poses gets rows of zeros.  The call zeroes both outputs on the stream and one launch,
 * a wave per list entry, adds into them with integer atomics: integer adds commute, so no result depends on an order. */
typedef struct drgnn_contact_counts_request {
    const uint64_t* bits;
    const int32_t* order;
    const int32_t* group_ptr;
    const int32_t* host_order;         /* the lists in host memory */
    const int32_t* host_group_ptr;
    int64_t n_poses, n_chain_a, n_chain_b, n_groups, n_listed;
    int32_t* counts;
    int32_t* residues;
} drgnn_contact_counts_request;

/* drgnn_pose_consensus_numerators: for the n_poses poses of bits (any poses of the topology of counts i32 [G, nA, nB]) and
 * row i32 [n_poses]: numerators[m] = 0 when row[m] < 0, else the sum of counts[row[m], a, b] over the set bits (a, b) of
 * pose m; i64 [n_poses].  Over the set it was counted from this is the row sum of drgnn_pose_common.  One launch. */
typedef struct drgnn_consensus_numerators_request {
    const uint64_t* bits;
    const int32_t* counts;
    const int32_t* row;
    const int32_t* host_row;           /* row in host memory */
    int64_t n_poses, n_chain_a, n_chain_b, n_groups;
    int64_t* numerators;
} drgnn_consensus_numerators_request;

/* drgnn_pose_consensus_bits: bits u64 [G, nA, WB] with bit (a, b) set iff counts[g, a, b] >= min_count[g], in the layout of
 * drgnn_pose_contacts (what drgnn_pose_common and the rest take like any pose), and n_contacts i32 [G], the set bits of
 * every group.  The call zeroes n_contacts on the stream; one launch writes the words and adds their popcounts to it. */
typedef struct drgnn_consensus_bits_request {
    const int32_t* counts;
    const int32_t* min_count;
    const int32_t* host_min_count;     /* min_count in host memory */
    int64_t n_chain_a, n_chain_b, n_groups;
    uint64_t* bits;
    int32_t* n_contacts;
} drgnn_consensus_bits_request;

/* the documented capacities: what = 0 residues of a complex, both chains (drgnn_fcc_capacity(0), 3072: what
 * drgnn_pose_contacts serves), 1 groups of one call (65535: the launch's second grid dimension), 2 entries of counts,
 * G nA nB (2^31 - 1: 32-bit indices), 3 poses of one drgnn_pose_consensus_numerators call (4194303: a workgroup each, the
 * launch stays below 2^32 work-items; split the call), 4 poses and entries of order of one drgnn_pose_contact_counts call
 * (2^31 - 1: 32-bit indices); -1 otherwise.  Pure host. */
int32_t drgnn_consensus_capacity(int32_t what);

/* All three: DRGNN_E_ARG before any launch for a null request or pointer, a negative count, and
 *   counts:      a group_ptr that does not start at 0, decreases or ends elsewhere than n_listed, an order entry outside
 *                [0, n_poses)
 *   numerators:  a row entry outside [-1, n_groups)
 *   bits:        a min_count below 1
 * DRGNN_E_CAPACITY beyond drgnn_consensus_capacity (split the groups or the poses over several calls).  No allocation, no
 * workspace, no synchronisation, no floating point; the outputs do not depend on what their buffers held.  Empty inputs
 * return 0 without a launch. */
int drgnn_pose_contact_counts(const drgnn_contact_counts_request* req, void* stream);
int drgnn_pose_consensus_numerators(const drgnn_consensus_numerators_request* req, void* stream);
int drgnn_pose_consensus_bits(const drgnn_consensus_bits_request* req, void* stream);

/* ---- pairwise pose RMSD and RMSD clustering of poses (drgnn_rmsd.h) ------------------------------------
 * The pose-by-pose RMSD matrix of poses of one topology (pairwise l-RMSD / i-RMSD) and the clustering rule of HADDOCK's
 * cluster_struc and of ClusPro on it.  tests/rmsd_ref.py states both rules.
 *
 * drgnn_pose_rmsd: xyz_a f32 [n_a, T, 3], xyz_b f32 [n_b, T, 3] (may be xyz_a; with n_b == n_a the call is then the
 * square matrix of one batch: pairs i < j are computed and mirrored, the diagonal is written as 0); rms_idx i32 [n_rms]
 * and fit_idx i32 [n_fit] atoms of a pose (fit_idx null with n_fit 0: no superposition), also given as HOST arrays: every
 * check comes from them.  Poses go to fp64.  Without fit: d[i, j] = sqrt(sum_a |a_i[a] - b_j[a]|^2 / n_rms) over rms_idx.
 * With fit: the optimal proper rotation and translation of pose a_i's fit atoms onto pose b_j's (Horn's quaternion, the
 * Jacobi routine of drgnn_dock_scores), applied to a_i, then the same sum over rms_idx, taken from fp64 moments about the
 * fit centroids.  Output d f64 [n_a, n_b].  d[i, j] of a pair of poses has the same bits in both directions, on
 * whichever side of whichever call the two poses are; it does not depend on n_a, n_b, a pose's place or the run.  A
 * collinear or coincident fit set leaves the rotation undetermined: the result is then undefined.
 * Workspace: drgnn_rmsd_workspace(n_a, n_b, n_fit, n_rms, offsets) bytes, 8-byte aligned, allocated by the caller, contents
 * undefined on entry.  After the call it holds a record of 3 n_fit + 3 n_rms + 2 doubles per pose, side a at offsets[0],
 * side b at offsets[1] (unused when the call is a square matrix), offsets[2] the size: the fit atoms and the rms atoms
 * about the fit centroid, then sum |x|^2 of either list.
 * phases: 0 the whole call; else a set of 1 records, 2 pairs: only these launches (the pairs read what an earlier call
 * left in the workspace; repeating a launch changes no bit). */
typedef struct drgnn_pose_rmsd_request {
    const float* xyz_a;
    const float* xyz_b;
    const int32_t* fit_idx;
    const int32_t* rms_idx;
    const int32_t* host_fit_idx;       /* the lists in host memory */
    const int32_t* host_rms_idx;
    int64_t n_a, n_b, n_atoms, n_fit, n_rms;
    int32_t phases;
    int32_t reserved;                  /* 0 */
    void* workspace;
    int64_t workspace_bytes;
    double* d;
} drgnn_pose_rmsd_request;

/* drgnn_pose_cluster_dist: from a distance matrix d f64 [M, M] (a device array; it need not be symmetric): j is a
 * neighbour of i iff i != j and d[i, j] <= cutoff, decided in fp64 on the stored value (a NaN is no neighbour).  Then the
 * outputs and the greedy loop of drgnn_pose_cluster.  Two launches, no host round trip. */
typedef struct drgnn_pose_cluster_dist_request {
    const double* d;
    int64_t n_poses;
    double cutoff;
    int32_t min_size;
    int32_t reserved;                  /* 0 */
    uint64_t* neighbours;
    uint64_t* transposed;
    int32_t* labels;
    int32_t* centres;
    int32_t* sizes;
    int32_t* n_clusters;
} drgnn_pose_cluster_dist_request;

/* the documented capacities: what = 0 poses on either side of one drgnn_pose_rmsd call (4096: split the call), 1 poses
 * of one drgnn_pose_cluster_dist call (drgnn_fcc_capacity(2), 4096: clustering cannot be split); -1 otherwise.  Pure host. */
int32_t drgnn_rmsd_capacity(int32_t what);

/* bytes of workspace for a drgnn_pose_rmsd call, -1 for counts the call refuses; offsets (may be null): int64 [3], see
 * above.  Pure host. */
int64_t drgnn_rmsd_workspace(int64_t n_a, int64_t n_b, int64_t n_fit, int64_t n_rms, int64_t* offsets);

/* Both: DRGNN_E_ARG before any launch for a null request or pointer, a negative count, and
 *   rmsd:         an index outside [0, n_atoms), n_fit of 1 or 2, n_rms 0, fit_idx without n_fit or n_fit without fit_idx,
 *                 phases outside 0..3, a workspace that is not 8-byte aligned
 *   cluster_dist: a cutoff that is not a positive finite number, min_size < 1
 * DRGNN_E_CAPACITY beyond drgnn_rmsd_capacity, or workspace_bytes too small.  No allocation, no synchronisation; empty
 * inputs return 0 without a launch. */
int drgnn_pose_rmsd(const drgnn_pose_rmsd_request* req, void* stream);
int drgnn_pose_cluster_dist(const drgnn_pose_cluster_dist_request* req, void* stream);

/* ---- the builder's output packed into a resident set's arrays (drgnn_pack.h) --------------------------
 * After drgnn_iface_fill on the same batch (and the optional drgnn_bsa_residues / drgnn_hse_residues /
 * drgnn_depth_residues over exactly its nodes, in node order): the arrays a drgnn_graph_set holds, written on the
 * device in one launch, one workgroup per complex.  What GraphDataSet.load_one_graph and ResidentGraphSet assemble per graph on the host.
 * Inputs as they lie on the device: node_ptr / edge_ptr / iedge_ptr i32 [M+1]; node_residue, chain, type i32 [N]; pos
 * f32 [N,3]; edge_index i64 [E,2] and internal_edge_index i64 [Ei,2] with ids local to their complex; dist f32 [E];
 * optional bsa f64 [N,3], hse f64 [N,3] (a row whose first entry is NaN reads 0, 0, 0) and depth f64 [N]; optional
 * res_feat f32 [n_rows, res_width]: a node reads row node_residue % n_rows (n_rows divides n_residues: poses of one topology share
 * one table); type_table f32 [20, type_width]: row = the node's type, holding every column that depends on the residue
 * type alone (the kernel carries no copy of such constants).
 * cols i32 [n_cols, 2] = (source, column of the source) of every column of x, sources 0 type_table, 1 pos, 2 chain,
 * 3 bsa, 4 hse, 5 res_feat, 6 depth (column 0 only); also given as the HOST array host_cols: every check comes from
 * it.  f64 sources are rounded once to f32 (round to nearest even: what torch.tensor(..., dtype=torch.float) does).
 * Outputs (a null pointer skips one): x f32 [N, n_cols]; edge_index_out i64 [2, 2E], graph k's columns 2 edge_ptr[k]
 * .. 2 edge_ptr[k+1] holding its pairs and then the same pairs reversed, local ids; edge_attr f32 [2E] in that order,
 * edge_mode 0 the distance, 1 tanh(-d/2 + 2) + 1 evaluated in fp64 on the f32 distance and rounded once;
 * internal_edge_index_out i64 [2, 2Ei], the same layout with ids + node_ptr[k] (batch-global); batch i64 [N], the
 * complex of every node.  Every element has one writer: no atomics, a complex's bits do not depend on the batch, its
 * place or the run.  The kernel clips the device offset tables to n_nodes / n_edges / n_iedges. */
typedef struct drgnn_pack_request {
    const int32_t* node_ptr;
    const int32_t* edge_ptr;
    const int32_t* iedge_ptr;
    const int32_t* node_residue;
    const int32_t* chain;
    const int32_t* type;
    const float* pos;
    const int64_t* edge_index;
    const float* dist;
    const int64_t* internal_edge_index;
    const double* bsa;
    const double* hse;
    const float* res_feat;
    const float* type_table;
    const int32_t* cols;
    const int32_t* host_cols;          /* cols in host memory */
    int64_t n_complexes, n_nodes, n_edges, n_iedges, n_residues, n_rows;
    int32_t res_width, type_width, n_cols, edge_mode;
    float* x;
    int64_t* edge_index_out;
    float* edge_attr;
    int64_t* internal_edge_index_out;
    int64_t* batch;
    const double* depth;               /* the last field: every field before it lies where it lay before depth was a source */
} drgnn_pack_request;

/* the documented capacities: what = 0 columns of x (256), 1 columns of type_table (64), both staged in LDS once per
 * workgroup, 2 complexes of one call (65 535, one workgroup each); -1 otherwise.  Pure host. */
int32_t drgnn_pack_capacity(int32_t what);

/* DRGNN_E_ARG, before any launch: a null offset table, with x a null cols / host_cols or n_cols < 1, a descriptor row
 * with a source outside 0..6, a column outside its source, a source whose array is null, n_rows that does not divide
 * n_residues, an output whose input is null, a negative count, edge_mode outside 0..1.  DRGNN_E_CAPACITY: n_complexes,
 * n_cols or type_width beyond drgnn_pack_capacity, n_nodes * n_cols beyond 2^31 - 1 (split the call).  No allocation,
 * no workspace, no synchronisation. */
int drgnn_iface_pack(const drgnn_pack_request* req, void* stream);

/* ---- device-resident graph set and mini-batch assembly --------------------
 * Replaces the host collate of every mini-batch: torch_geometric DataLoader -> Batch.from_data_list over
 * HDF5DataSet.load_one_graph's Data objects (NeuralNet.py:153-154, DataSet.py:231-366).  The set is the
 * whole dataset uploaded once, graph-major: x [sumN, F]; edge_index [2, sumE] with LOCAL node ids (the
 * per-graph tensors of DataSet.py:266-269 back to back, row block then column block); edge_attr [sumE];
 * cluster0 [sumN]; cluster1 [sumC0]; y [G] (4- or 8-byte elements); int64 offset tables [G+1].
 * drgnn_collate assembles the mini-batch ids[0..B) (graph numbers, any order, repeats allowed) exactly as
 * the PyG collate does: x / cluster0 / cluster1 / edge_attr concatenated, both rows of edge_index shifted by
 * the slot's node offset, batch[n] = slot, y gathered; plus the int32 per-slot offset tables node_ptr /
 * edge_ptr / c1_ptr [B+1] that drgnn_topology_build and the step kernels take.  The caller sizes the
 * outputs from its host copy of the tables (N = sum of the selected node counts, ...).  One workgroup per
 * slot; ids outside [0, G) select an empty graph. */
int drgnn_collate(const drgnn_graph_set* set, const int32_t* ids, int64_t n_graphs, int64_t n_nodes,
                  int64_t n_edges, float* x, int64_t* edge_index, float* edge_attr, int64_t* batch,
                  int64_t* cluster0, int64_t* cluster1, void* y, int32_t* node_ptr, int32_t* edge_ptr,
                  int32_t* c1_ptr, void* stream);

/* ---- one training epoch, driven natively --------------------------------------------
 * The body of NeuralNet._epoch's loop (NeuralNet.py:486-506) for EVERY mini-batch of an epoch, enqueued on
 * `stream` without touching the host language in between and without any synchronisation: for mini-batch k
 *     drgnn_collate(k+1)  ->  drgnn_net_train_step(k)  [+ topology of k+1 in the same launch]  ->  drgnn_step_update
 * -- in fact without the collate launch: the topology builder of mini-batch k+1 (extra workgroups of step k's
 * launch) reads the graphs' index data in place from the resident set and gathers their node features and
 * targets into the slot's compact buffers (drgnn_topology_request, resident-set mode); two mini-batch slots are
 * carved out of `scratch` (k trains from one while k+1 is assembled in the other).
 * ids / host_ids: the epoch's visiting order (graph numbers of `set`) on the device and on the host; mini-batch k
 * = ids[k*batch_size, min((k+1)*batch_size, n_ids)).  host_*_ptr: host copies of the set's offset tables (they size
 * every launch).  Outputs: pred [n_ids, O] in visiting order, losses [ceil(n_ids / batch_size)] (mean loss of each
 * mini-batch, what the reference accumulates with loss.item()).  Model / optimiser arguments as for
 * drgnn_net_train_step / drgnn_step_update.  Returns DRGNN_E_CAPACITY when some graph does not fit the fused step
 * kernel's or the topology builder's LDS budget (the caller then steps mini-batch by mini-batch).
 * drgnn_train_epoch_scratch_bytes: bytes of device scratch the plan needs (< 0: error code). */
/* ---- cached topology (declared mode) -----------------------------------------------------------------
 * Per-graph topology does not depend on the mini-batch (all ids inside a graph's segment are local), so a
 * resident graph set can build it ONCE: one topology workspace over the whole set (drgnn_topology_build_request
 * in resident-set mode with ids = 0..G-1 and the set's own offset tables), kept next to the set's node features
 * and targets.  A mini-batch is then just a list of graph numbers: the fused step reads graph ids[g]'s segments
 * of the cached workspace in place -- no builder workgroups, no per-step index work at all.
 * (The reference redoes this work in every forward pass: community_pooling.py:25-30,197-201; "rebuilt every
 * step" stays the default mode of this library and of bench.py's headline.) */
typedef struct drgnn_topology_cache {
    int64_t n_graphs, n_nodes, n_edges;          /* of the WHOLE set = the shape the workspace was laid out for */
    const int32_t* ws_i32; const float* ws_f32;  /* ws_f32 may be NULL (nets without edge weights) */
    const float* x;                              /* [n_nodes, F] node features, graph-major (the set's x) */
    const void* y; int32_t y_bytes, flags;       /* [n_graphs] targets: 4 = float32, 8 = int64; may be NULL (inference);
                                                    flags: the DRGNN_TOPO_* flags the workspace was built with */
    const float* tiles;                          /* flags & DRGNN_TOPO_TILES: the set's aggregation tiles (n_nodes rows), else NULL */
} drgnn_topology_cache;
/* drgnn_net_train_step over the graphs ids[0..n_graphs) of a cached set: same outputs, same arithmetic (slot g
 * of every output = graph ids[g]); max_* bound the graphs of THIS mini-batch. */
int drgnn_net_train_step_cached(const drgnn_net_desc* net, const drgnn_head_desc* head,
                                const drgnn_topology_cache* cache, const int32_t* ids, int64_t n_graphs,
                                int32_t max_nodes, int32_t max_edges, int32_t max_c0, int32_t* step2, float* pred,
                                float* readout, float* head_partials, float* partials, uint64_t* xchg,
                                const drgnn_step_hints* hints /* optional */, void* stream);

/* Ensemble inference: K checkpoints of one net (same kind, F, R, H, O) over the same cached graphs in ONE launch, one
 * workgroup per (model, graph).  The member table lives in DEVICE memory, K entries, written once by the caller: member m's
 * conv parameters (same strides as a single model's) and FC head. */
typedef struct drgnn_ens_member {
    drgnn_net_desc net;
    const float* w1; const float* b1; const float* w2; const float* b2;
} drgnn_ens_member;
/* The plan of an ensemble launch of K models over plan->n_graphs graphs (inference; the `in` members as for
 * drgnn_net_step_plan, whose `out` members it fills).  Returns 1 when the fused ensemble launch takes these bounds (its
 * workgroups never wait for each other: every K x n_graphs), 0 otherwise (family NONE: the caller launches the K models
 * one by one). */
int32_t drgnn_ens_step_plan(drgnn_step_plan* plan, int32_t K);
/* The ensemble launch over the graphs ids[0..n_graphs) of a cached set: pred [K][n_graphs][O], readout [K][n_graphs][R]
 * (member m's slot g = what drgnn_net_train_step_cached of that member alone writes for graph ids[g] with the plan's
 * layout).  `net` / `head`: member 0's descriptors (shapes, task, sigmoid; their pointers are not read).  hints->plan: the
 * plan drgnn_ens_step_plan returned (required). */
int drgnn_ens_predict_cached(const drgnn_net_desc* net, const drgnn_head_desc* head, const drgnn_ens_member* members,
                             int32_t K, const drgnn_topology_cache* cache, const int32_t* ids, int64_t n_graphs,
                             int32_t max_nodes, int32_t max_edges, int32_t max_c0, int32_t* step2, float* pred,
                             float* readout, const drgnn_step_hints* hints, void* stream);

/* Cohort training: K members of one net (same kind, F, R, H, O: cross-validation folds, seeds, a learning-rate sweep) stepped
 * over the same cached set in TWO launches per optimisation step of all K -- the training counterpart of the ensemble launch.
 * drgnn_cohort_train_step_cached: one workgroup per (member, graph) with the ensemble's block numbering (a graph's K members
 * sit on one XCD); only the one-workgroup-per-graph forms, so no workgroup waits for another and any K x B is safe.
 * drgnn_cohort_update: drgnn_step_update's fixed-order sums and Adam once per member (second grid dimension).
 * Member m's result is what drgnn_net_train_step_cached (plan force_wgs = 1) + drgnn_step_update give for that member alone,
 * bit for bit.  The member table lives in DEVICE memory, K entries, written once by the caller.  The members' parameters have
 * the same layout: every gradient tensor sits at the same offset of its member's flat gradient buffer. */
typedef struct drgnn_cohort_member {
    drgnn_net_desc net;                                          /* conv parameters (same strides as member 0's) */
    const float* w1; const float* b1; const float* w2; const float* b2;   /* FC head */
    float* flat_param; float* flat_grad; float* exp_avg; float* exp_avg_sq;   /* [n_param] each */
    int32_t* step2;                                              /* the member's own int32[4], as drgnn_net_train_step's */
    float* pred; float* readout; float* head_partials; float* partials;   /* outputs / slabs, sized for the largest mini-batch */
    float* loss;                                                 /* [1] the member's loss word */
    double lr, beta1, beta2, eps;                                /* Adam, as for drgnn_adam_step */
    uint32_t seed; int32_t reserved;                             /* dropout stream seed */
} drgnn_cohort_member;
/* The plan of a cohort launch of K members over plan->n_graphs graphs each (training; otherwise as drgnn_ens_step_plan).
 * Returns 1 when the fused cohort launches take these bounds, 0 otherwise (family NONE: the caller steps the members one by
 * one; the host emulation always answers NONE). */
int32_t drgnn_cohort_step_plan(drgnn_step_plan* plan, int32_t K);
/* The fused step of all members.  ids: DEVICE int32, member m's graph numbers of this step at ids + m * ids_stride;
 * counts: DEVICE int32 [K], member m's mini-batch size B_m <= n_graphs (= the largest, which sizes the grid).  A slot
 * g >= B_m returns at once; a member with B_m = 0 is not stepped (step index, slabs, loss word untouched).  Graph numbers must
 * lie inside the cached set (the caller checks: they are device memory here).  Targets come from cache->y.
 * `net` / `head`: member 0's descriptors (shapes, task, dropout probability, class weights; their parameter pointers and the
 * seed are not read).  hints->plan: the plan drgnn_cohort_step_plan returned (required).  hints->host_ids (+ set_node_ptr /
 * set_edge_ptr): ONLY when every member steps exactly these n_graphs graphs -- the host-known sizes then travel in the launch
 * arguments as for a single model; otherwise leave them NULL (sizes come from the workspace tables).  Never allocates or
 * synchronises; hipGraph-capturable. */
int drgnn_cohort_train_step_cached(const drgnn_net_desc* net, const drgnn_head_desc* head, const drgnn_cohort_member* members,
                                   int32_t K, const drgnn_topology_cache* cache, const int32_t* ids, const int32_t* counts,
                                   int64_t ids_stride, int64_t n_graphs, int32_t max_nodes, int32_t max_edges, int32_t max_c0,
                                   const drgnn_step_hints* hints, void* stream);
/* The update of all members: member m sums its counts[m] slabs in drgnn_step_update's fixed order, applies Adam with its own
 * learning rate and step index, commits its step2[0] = step2[1] and writes its loss word.  g_conv1 / g_conv2 / head_offset:
 * member 0's gradient destinations (member m's are those shifted by members[m].flat_grad - members[0].flat_grad).
 * losses: optional DEVICE float [K]: a stepped member's loss goes there too (an epoch's [steps, K] record, row by row). */
int drgnn_cohort_update(const drgnn_net_desc* net, const drgnn_cohort_member* members, int32_t K, const int32_t* counts,
                        drgnn_conv_grads* g_conv1, drgnn_conv_grads* g_conv2, int32_t R, int32_t H, int32_t O,
                        int64_t head_offset, int64_t n_param, float* losses /* optional */, int32_t apply_adam, void* stream);

/* Data-parallel hook of the native epoch loop: called on the host once per mini-batch, after the launches that leave
 * this rank's gradient of mini-batch `batch_index` in flat_grad have been ENQUEUED on `stream`; it must enqueue the
 * exchange (one all-reduce of flat_grad, weighted n_local / n_global) on the same stream and return 0.  The loop then
 * enqueues Adam (drgnn_adam_step).  No host synchronisation is implied. */
typedef int (*drgnn_exchange_fn)(void* user, int64_t batch_index, int64_t n_local, void* stream);

typedef struct drgnn_epoch_plan {
    const drgnn_graph_set* set;
    const int64_t* host_node_ptr; const int64_t* host_edge_ptr; const int64_t* host_c1_ptr;
    const int32_t* ids; const int32_t* host_ids; int64_t n_ids;
    int32_t batch_size, need_weights;
    int32_t inference, reserved;   /* inference != 0: forward + head only (dropout off), pred is the only output;
                                      the optimiser members, step2 excepted, and the set's targets may be NULL */
    const drgnn_net_desc* net; const drgnn_head_desc* head;
    drgnn_conv_grads* g_conv1; drgnn_conv_grads* g_conv2;
    int64_t head_offset;
    float* flat_param; float* flat_grad; float* exp_avg; float* exp_avg_sq; int64_t n_param;
    int32_t* step2;
    double lr, beta1, beta2, eps;
    /* cached-topology mode (non-NULL): mini-batches are stepped straight out of the cache, the loop issues no
     * offset-table, builder or gather work; `set` is then only consulted for the graphs' sizes on the host */
    const drgnn_topology_cache* cache;
    /* data parallel (non-NULL): per mini-batch  gradient launches -> exchange(...) -> Adam launch  instead of the fused
     * reduce+Adam launch; every rank must run the same number of mini-batches */
    drgnn_exchange_fn exchange; void* exchange_user;
    /* optional: the override members of this plan apply to every step launch of the loop (tests, A/B runs) */
    const drgnn_step_plan* step_overrides;
    /* optional: one more destination of the LAST mini-batch's loss (its update launch writes losses[n_batches - 1] and this
     * word): a trainer's fixed "loss of the last step" word stays current without a copy behind the epoch */
    float* last_loss;
} drgnn_epoch_plan;
int64_t drgnn_train_epoch_scratch_bytes(const drgnn_epoch_plan* plan);
int drgnn_train_epoch(const drgnn_epoch_plan* plan, void* scratch, int64_t scratch_bytes, float* pred,
                      float* losses, void* stream);

/* ---- optimiser options: decoupled weight decay (AdamW), gradient-norm clipping, learning-rate table ----------
 * The `_opt` siblings below take Adam's scalars from this record instead of their argument lists and otherwise do what
 * the entry point they are named after does; with every option off they compute the same bits.
 *   weight_decay / decoupled   decoupled != 0: before the Adam step, p <- p * (float)(1 - lr_t * weight_decay), the factor
 *                  formed in double (torch.optim.AdamW); the gradient is not touched.  decoupled == 0: the coupled L2 term of
 *                  drgnn_adam_step (g + weight_decay * p), which only the flat kernel knows: the update siblings then leave
 *                  the gradient and run the flat kernel behind it.
 *   lr_table       NULL, or DEVICE double [lr_n]: optimiser step t >= 1 uses entry min(t, lr_n) - 1 in place of lr, loaded
 *                  by the step index the kernel reads anyway -- nothing of a schedule is a kernel argument, so a recorded
 *                  step advances through it on replay.
 *   clip / max_grad_norm   clip != 0: torch.nn.utils.clip_grad_norm_(params, max_grad_norm), norm_type 2.  N = ||g||_2 over
 *                  the whole flat gradient, every square formed and summed in double in a fixed order (per block, then the
 *                  per-block words in index order); s = (float)min(1, max_grad_norm / (N + 1e-6)); g <- g * s is stored back
 *                  to the flat gradient and consumed by Adam.  Two launches, no workgroup waits for another: the sums launch
 *                  (Adam off) leaves one double per block in norm_words, the Adam launch adds them up in every block.
 *                  norm_words: DEVICE scratch of norm_cap doubles, at least max(update blocks, ceil(n_param / 256)): see
 *                  drgnn_optim_norm_words.  norm_out: optional DEVICE float [1], receives N (before clipping).
 *   dead_off / dead_len   element ranges of the flat buffers that belong to parameters without a gradient (GINet's
 *                  fc_attention / fc_edge_attr): the flat kernel leaves parameter, moments and gradient there untouched, as
 *                  torch skips a parameter whose grad is None.  (The update launches never visit them.)  A caller that wants
 *                  coupled L2 to decay them, as drgnn_adam_step does, passes n_dead = 0. */
typedef struct drgnn_optim {
    double lr, beta1, beta2, eps;
    double weight_decay;
    double max_grad_norm;
    const double* lr_table;
    double* norm_words;
    float* norm_out;
    int32_t lr_n, decoupled, clip, norm_cap;
    int32_t n_dead, reserved;
    int64_t dead_off[DRGNN_ZERO_RANGES], dead_len[DRGNN_ZERO_RANGES];
} drgnn_optim;
/* doubles of norm_words scratch that any `_opt` call over a net of n_param parameters needs */
int64_t drgnn_optim_norm_words(int64_t n_param);
/* drgnn_adam_step with the options; with clip it first leaves one word per 256 elements of grad (one more small launch),
 * then scales grad in place. */
int drgnn_adam_step_opt(float* param, float* grad, float* exp_avg, float* exp_avg_sq, const int32_t* step, int64_t n,
                        const drgnn_optim* optim, void* stream);
int drgnn_train_update_opt(const drgnn_net_desc* net, const float* conv_partials, int64_t n_graphs,
                           drgnn_conv_grads* g_conv1, drgnn_conv_grads* g_conv2,
                           const float* head_partials, int64_t head_slabs, int32_t R, int32_t H, int32_t O,
                           int64_t head_offset, float* flat_param, float* flat_grad, float* exp_avg, float* exp_avg_sq,
                           int64_t n_param, const int32_t* step, float* loss, const drgnn_optim* optim,
                           int32_t apply_adam, void* stream);
int drgnn_step_update_opt(const drgnn_net_desc* net, const float* conv_partials, int64_t n_graphs,
                          drgnn_conv_grads* g_conv1, drgnn_conv_grads* g_conv2, const float* head_partials,
                          const float* readout, int32_t R, int32_t H, int32_t O, int64_t head_offset,
                          float* flat_param, float* flat_grad, float* exp_avg, float* exp_avg_sq, int64_t n_param,
                          int32_t* step2, float* loss, const drgnn_optim* optim,
                          int32_t apply_adam, int32_t slabs_per_graph, void* stream);
/* drgnn_cohort_update with a DEVICE table of K records next to the member table: member m's Adam scalars and options are
 * optims[m] (members[m].lr / beta1 / beta2 / eps are not read; decoupled decay only: a coupled weight_decay is ignored, as
 * drgnn_cohort_update knows none).  any_clip: non-zero when any record clips -- the clipping members then take their Adam
 * step in a second launch (once per member, second grid dimension); every record's norm_cap must be at least
 * drgnn_optim_norm_words(n_param).  A member without a mini-batch (counts[m] == 0) is left alone, norm_out included.
 * Member m's result is what drgnn_step_update_opt gives for that member alone, bit for bit. */
int drgnn_cohort_update_opt(const drgnn_net_desc* net, const drgnn_cohort_member* members, const drgnn_optim* optims, int32_t K,
                            const int32_t* counts, drgnn_conv_grads* g_conv1, drgnn_conv_grads* g_conv2, int32_t R, int32_t H,
                            int32_t O, int64_t head_offset, int64_t n_param, float* losses /* optional */, int32_t apply_adam,
                            int32_t any_clip, void* stream);
/* drgnn_train_epoch with the options (plan->lr / beta1 / beta2 / eps are not read) */
int drgnn_train_epoch_opt(const drgnn_epoch_plan* plan, const drgnn_optim* optim, void* scratch, int64_t scratch_bytes,
                          float* pred, float* losses, void* stream);

/* ---- one-shot all-reduce over peer-mapped exchange buffers (csrc/drgnn_p2p.h) ------------------------------
 * Data-parallel exchange of the flat gradient without a ring: each rank owns a fine-grained exchange buffer
 * (drgnn_p2p_alloc), hands its 64-byte IPC handle to the peers (e.g. torch.distributed.all_gather), maps theirs
 * (drgnn_p2p_open) and then every step  drgnn_allreduce_oneshot  = publish own weighted vector, read all W vectors
 * over xGMI, add them in rank order.  One launch, no host work, hipGraph-capturable; sums are bit-identical on all
 * ranks.  `seq` = DRGNN_P2P_SEQ_WORDS zero-initialised uint32 device words, `status` one int32 device word (non-zero
 * after a wait that expired: a peer did not arrive).  world <= DRGNN_P2P_MAX_RANKS. */
#define DRGNN_P2P_MAX_RANKS 16
#define DRGNN_P2P_SEQ_WORDS 16
int64_t drgnn_p2p_bytes(int64_t n_floats);
int drgnn_p2p_alloc(int64_t bytes, void** dev_ptr, void* ipc_handle_64);     /* zero-filled, fine-grained */
int drgnn_p2p_open(const void* ipc_handle_64, void** dev_ptr);
int drgnn_p2p_close(void* dev_ptr);
int drgnn_p2p_free(void* dev_ptr);
/* part: 0 = the whole exchange (product); 1 = publish only, 2 = consume only (single-process protocol tests) */
int drgnn_allreduce_oneshot(float* grad, int64_t n, void* const* peer_bufs, int32_t world, int32_t rank,
                            float weight, uint32_t* seq, int32_t* status, int32_t part, void* stream);

int drgnn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DRGNN_H */
