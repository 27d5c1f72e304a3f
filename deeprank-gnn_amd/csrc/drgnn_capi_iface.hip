// drgnn_capi_iface.hip -- the entry points of iface_graphs.py and resident.py's packing: interface graphs from atom
// coordinates (count, fill) and the builder's output packed into a resident set's arrays, with the __global__ wrappers they
// launch.  One of the drgnn_capi*.hip units (drgnn_capi.hip says how they are built and what an entry point looks like).
#include "drgnn_capi_common.h"
#include "drgnn_iface.h"
#include "drgnn_pack.h"

#ifndef DRGNN_EMU
// interface graphs from atom coordinates (drgnn_iface.h)
__global__ void __launch_bounds__(IF_NT) k_iface_sphere(IfaceArgs a) {
    const int r = blockIdx.x * IF_NT + threadIdx.x;
    if (r < a.n_residues) iface_sphere_item(a, r);
}
__global__ void __launch_bounds__(IF_NT) k_iface_pairs(IfaceArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem_if[];
    iface_pairs_block(a, blockIdx.y, blockIdx.x, smem_if);
}
__global__ void __launch_bounds__(IF_NT) k_iface_rows(IfaceArgs a, int write) { iface_rows_block(a, blockIdx.y, blockIdx.x, write != 0); }
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_iface_scan(IfaceArgs a) {
    __shared__ int part[DRGNN_NTHREADS + 1];
    iface_scan_block(a, blockIdx.x, part);
}
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_iface_offsets(IfaceArgs a) {
    __shared__ int part[DRGNN_NTHREADS + 1];
    iface_offsets_block(a, part);
}
// the builder's output packed into a resident set's arrays (drgnn_pack.h): one workgroup per complex
__global__ void __launch_bounds__(PK_NT) k_iface_pack(PackArgs a) {
    __shared__ PackShared smem_pk;
    pack_block(a, (int)blockIdx.x, smem_pk);
}
#endif  // !DRGNN_EMU

extern "C" {

// ---- interface graphs from atom coordinates (drgnn_iface.h) ------------------------------------------
int64_t drgnn_iface_workspace_bytes(int64_t n_complexes, int64_t max_res_a, int64_t max_res_b, int64_t n_residues) {
    if (n_complexes < 0 || max_res_a < 0 || max_res_b < 0 || n_residues < 0) return -1;
    int64_t off[8];
    iface_layout(n_complexes, max_res_a, max_res_b, n_residues, off);
    return off[7];
}

// checks the request on the host and fills the launch record; *max_res: the longest complex
static int iface_prepare(const drgnn_iface_request* q, IfaceArgs& a, int* max_res) {
    if (!q || !q->host_atom_ptr || !q->host_res_ptr || !q->node_ptr || !q->edge_ptr || !q->iedge_ptr) return DRGNN_E_ARG;
    const int64_t T = q->n_atoms, R = q->n_residues, M = q->n_complexes;
    if (T < 0 || R < 0 || M < 0 || T > INT32_MAX / 3 || R >= INT32_MAX) return DRGNN_E_ARG;
    if (M > 0 && (!q->host_res_split || !q->res_ptr || !q->res_split)) return DRGNN_E_ARG;
    if (R > 0 && (!q->atom_ptr || !q->res_type || !q->workspace)) return DRGNN_E_ARG;
    if (T > 0 && !q->xyz) return DRGNN_E_ARG;
    if (!(q->contact_distance >= 0.0) || !(q->internal_contact_distance >= 0.0) || q->tile_atoms < 0) return DRGNN_E_ARG;
    const int32_t *ap = q->host_atom_ptr, *rp = q->host_res_ptr, *sp = q->host_res_split;
    if (!ragged_check(ap, rp, sp, T, R, M)) return DRGNN_E_ARG;
    int max_atoms = 0, maxA = 0, maxB = 0, maxR = 0, maxB_atoms = 0;
    for (int64_t r = 0; r < R; ++r) max_atoms = std::max(max_atoms, ap[r + 1] - ap[r]);
    for (int64_t c = 0; c < M; ++c) {
        maxA = std::max(maxA, sp[c] - rp[c]);
        maxB = std::max(maxB, rp[c + 1] - sp[c]);
        maxR = std::max(maxR, rp[c + 1] - rp[c]);
        maxB_atoms = std::max(maxB_atoms, ap[rp[c + 1]] - ap[sp[c]]);
    }
    if (M > 65535) return DRGNN_E_CAPACITY;
    if (M * (int64_t)maxA * maxB > INT32_MAX) return DRGNN_E_CAPACITY;      // (the edge counts and their prefix sums are int32)
    int tile = q->tile_atoms > 0 ? q->tile_atoms : IF_TILE_DEFAULT;
    tile = std::max(std::max(std::min(tile, maxB_atoms), max_atoms), 1);
    if (iface_pairs_lds_bytes(tile) > DRGNN_LDS_LIMIT) return DRGNN_E_CAPACITY;
    int64_t off[8];
    iface_layout(M, maxA, maxB, R, off);
    if (q->workspace_bytes < off[7]) return DRGNN_E_CAPACITY;
    if (off[7] > 0 && ((uintptr_t)q->workspace & 15) != 0) return DRGNN_E_ARG;
    char* ws = (char*)q->workspace;
    memset(&a, 0, sizeof(a));
    a.xyz = q->xyz; a.atom_ptr = q->atom_ptr; a.res_ptr = q->res_ptr; a.res_split = q->res_split; a.res_type = q->res_type;
    a.n_complexes = (int)M; a.n_residues = (int)R; a.maxA = maxA; a.maxB = maxB; a.tile_atoms = tile;
    a.cut = (float)q->contact_distance; a.cut2 = (float)(q->contact_distance * q->contact_distance);
    a.icut = (float)q->internal_contact_distance;
    a.icut2 = (float)(q->internal_contact_distance * q->internal_contact_distance);
    a.D = (float*)(ws + off[0]); a.sphere = (float*)(ws + off[1]); a.flag = (int*)(ws + off[2]); a.nloc = (int*)(ws + off[3]);
    a.eoff = (int*)(ws + off[4]); a.ioff = (int*)(ws + off[5]); a.cnt = (int*)(ws + off[6]);
    a.node_ptr = q->node_ptr; a.edge_ptr = q->edge_ptr; a.iedge_ptr = q->iedge_ptr;
    *max_res = maxR;
    return 0;
}

// the rows kernel over (blocks of IF_AB residues, complexes): counting (write 0) or filling (1)
static int iface_rows(const IfaceArgs& a, int max_res, int write, void* stream) {
    DRGNN_LAUNCH(k_iface_rows, grid2((max_res + IF_AB - 1) / IF_AB, a.n_complexes, IF_NT), stream,
                 iface_rows_block(a, (int)by, (int)bx, write != 0), a, write);
    return 0;
}

int drgnn_iface_count(const drgnn_iface_request* req, void* stream) {
    IfaceArgs a;
    int max_res = 0;
    int rc = iface_prepare(req, a, &max_res);
    if (rc) return rc;
    const int M = a.n_complexes, R = a.n_residues;
    // (without residues, complexes or chain-A residues the grids of the first three launches are empty: skipped)
    const int64_t lds_bytes = iface_pairs_lds_bytes(a.tile_atoms);
    DRGNN_EMU_ONLY(std::vector<float> lds((size_t)(lds_bytes / 4) + 4); std::vector<int> part(DRGNN_NTHREADS + 1);)
    DRGNN_LAUNCH(k_iface_sphere, grid_items(R, IF_NT), stream, iface_sphere_item(a, (int)bx), a);
    DRGNN_LAUNCH(k_iface_pairs, (Grid{(a.maxA + IF_AB - 1) / IF_AB, M, IF_NT, lds_bytes}), stream,
                 iface_pairs_block(a, (int)by, (int)bx, lds.data()), a);
    if ((rc = iface_rows(a, max_res, 0, stream))) return rc;
    DRGNN_LAUNCH(k_iface_scan, grid1(M), stream, iface_scan_block(a, (int)bx, part.data()), a);
    DRGNN_LAUNCH(k_iface_offsets, grid1(1), stream, iface_offsets_block(a, part.data()), a);
    return 0;
}

int drgnn_iface_fill(const drgnn_iface_request* req, int64_t n_nodes, int64_t n_edges, int64_t n_iedges,
                     int32_t* node_residue, float* pos, int32_t* chain, int32_t* type, int64_t* edge_index, float* dist,
                     int64_t* internal_edge_index, float* internal_dist, void* stream) {
    IfaceArgs a;
    int max_res = 0;
    const int rc = iface_prepare(req, a, &max_res);
    if (rc) return rc;
    if (n_nodes < 0 || n_edges < 0 || n_iedges < 0) return DRGNN_E_ARG;
    if (n_nodes > 0 && (!node_residue || !pos || !chain || !type)) return DRGNN_E_ARG;
    if (n_edges > 0 && (!edge_index || !dist)) return DRGNN_E_ARG;
    if (n_iedges > 0 && (!internal_edge_index || !internal_dist)) return DRGNN_E_ARG;
    a.node_residue = node_residue; a.pos = pos; a.chain = chain; a.type = type;
    a.edge_index = edge_index; a.dist = dist; a.iedge_index = internal_edge_index; a.idist = internal_dist;
    a.n_nodes = n_nodes; a.n_edges = n_edges; a.n_iedges = n_iedges;
    if (a.n_complexes == 0 || max_res == 0 || n_nodes == 0) return 0;
    return iface_rows(a, max_res, 1, stream);
}

// ---- the builder's output packed into a resident set's arrays (drgnn_pack.h) --------------------------
DRGNN_CAPACITY(drgnn_pack_capacity, PK_FCAP, PK_TCAP, PK_MAX_COMPLEXES)

int drgnn_iface_pack(const drgnn_pack_request* q, void* stream) {
    if (!q || !q->node_ptr || !q->edge_ptr || !q->iedge_ptr) return DRGNN_E_ARG;
    const int64_t M = q->n_complexes, N = q->n_nodes, E = q->n_edges, Ei = q->n_iedges, R = q->n_residues, NB = q->n_rows;
    const int64_t F = q->n_cols, W = q->res_width, Wt = q->type_width;
    if (M < 0 || N < 0 || E < 0 || Ei < 0 || R < 0 || NB < 0 || F < 0 || W < 0 || Wt < 0) return DRGNN_E_ARG;
    if (N > INT32_MAX || E > INT32_MAX / 2 || Ei > INT32_MAX / 2) return DRGNN_E_ARG;
    if (q->edge_mode < 0 || q->edge_mode > 1) return DRGNN_E_ARG;
    if (M > PK_MAX_COMPLEXES || F > PK_FCAP || Wt > PK_TCAP) return DRGNN_E_CAPACITY;
    if (q->x) {
        if (F < 1 || !q->cols || !q->host_cols) return DRGNN_E_ARG;
        if (N * F > INT32_MAX) return DRGNN_E_CAPACITY;
        const int64_t width[PK_NSRC] = {Wt, 3, 1, 3, 3, W, 1};
        for (int64_t f = 0; f < F; ++f) {
            const int32_t src = q->host_cols[2 * f], c = q->host_cols[2 * f + 1];
            if (src < 0 || src >= PK_NSRC || c < 0 || c >= width[src]) return DRGNN_E_ARG;
            if (src == PK_TYPE && !q->type_table) return DRGNN_E_ARG;
            if (src == PK_RES && (!q->res_feat || NB < 1 || R % NB != 0)) return DRGNN_E_ARG;
            if (N > 0) {                                               // (an empty batch has no arrays)
                const void* need = src == PK_TYPE ? (const void*)q->type : src == PK_POS ? (const void*)q->pos :
                                   src == PK_CHAIN ? (const void*)q->chain : src == PK_BSA ? (const void*)q->bsa :
                                   src == PK_HSE ? (const void*)q->hse : src == PK_DEPTH ? (const void*)q->depth :
                                   (const void*)q->node_residue;
                if (!need) return DRGNN_E_ARG;
            }
        }
    }
    if (E > 0 && (q->edge_index_out || q->edge_attr) && !q->edge_index) return DRGNN_E_ARG;
    if (E > 0 && q->edge_attr && !q->dist) return DRGNN_E_ARG;
    if (Ei > 0 && q->internal_edge_index_out && !q->internal_edge_index) return DRGNN_E_ARG;
    if (M == 0 || (N == 0 && E == 0 && Ei == 0)) return 0;
    PackArgs a;
    memset(&a, 0, sizeof(a));
    a.node_ptr = q->node_ptr; a.edge_ptr = q->edge_ptr; a.iedge_ptr = q->iedge_ptr;
    a.node_residue = q->node_residue; a.chain = q->chain; a.type = q->type; a.pos = q->pos;
    a.edge_index = q->edge_index; a.dist = q->dist; a.iedge_index = q->internal_edge_index;
    a.bsa = q->bsa; a.hse = q->hse; a.depth = q->depth; a.res_feat = q->res_feat; a.type_table = q->type_table; a.cols = q->cols;
    a.n_rows = (int)std::max<int64_t>(NB, 1); a.W = (int)W; a.Wt = (int)Wt; a.F = (int)F; a.edge_mode = q->edge_mode;
    a.N = (int)N; a.E = (int)E; a.Ei = (int)Ei;
    a.x = q->x; a.edge_index_out = q->edge_index_out; a.edge_attr = q->edge_attr;
    a.iedge_index_out = q->internal_edge_index_out; a.batch = q->batch;
    DRGNN_EMU_ONLY(std::unique_ptr<PackShared> lds(new PackShared);)
    DRGNN_LAUNCH(k_iface_pack, grid1(M, PK_NT), stream, pack_block(a, (int)bx, *lds), a);
    return 0;
}

}  // extern "C"
