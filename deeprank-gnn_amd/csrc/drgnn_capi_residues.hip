// drgnn_capi_residues.hip -- the entry points of residue_features.py: buried surface area, half-sphere exposure and residue
// depth of interface residues, the request checks the three share, and the __global__ wrappers they launch.  One of the
// drgnn_capi*.hip units (drgnn_capi.hip says how they are built and what an entry point looks like).
#include "drgnn_capi_common.h"
#include "drgnn_bsa.h"
#include "drgnn_hse.h"
#include "drgnn_depth.h"

#ifndef DRGNN_EMU
// buried surface area (drgnn_bsa.h): one workgroup per target residue
// (8 waves per SIMD: two workgroups per CU; the fp64 path of nearly tangent circles must not cost the others their registers)
__global__ void __launch_bounds__(DRGNN_NTHREADS, 8) k_bsa_residues(BsaArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_bs[];
    bsa_residue(a, (int64_t)blockIdx.x, *(BsaShared*)smem_bs);
}
// half-sphere exposure (drgnn_hse.h): one workgroup per tile of targets of one complex
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_hse_residues(HseArgs a) {
    __shared__ HseShared smem_hs;
    hse_tile(a, (int)blockIdx.x, smem_hs);
}
// residue depth (drgnn_depth.h): a wave per atom; one workgroup per complex; one workgroup per target residue
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_depth_dots(DepthArgs a) { depth_dots_tile(a, (int64_t)blockIdx.x); }
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_depth_components(DepthArgs a) {
    __shared__ DepthShared smem_dp;
    depth_components(a, (int)blockIdx.x, smem_dp);
}
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_depth_residues(DepthArgs a) {
    __shared__ DepthShared smem_dp;
    depth_residue(a, (int64_t)blockIdx.x, smem_dp);
}
#endif  // !DRGNN_EMU

// The checks the residue-feature requests (bsa, hse, depth) share; `q` is any of them: the shared fields have the same names.
// residue_request_check: the counts and pointers, in front of the entry point's own ARG and CAPACITY checks (k_max: the largest
// n_targets its indices allow); residue_tables_check: the host tables, behind them (sp: the chain split, or null).
template <class Request>
static int residue_request_check(const Request* q, int64_t k_max) {
    if (!q || !q->host_atom_ptr || !q->host_res_ptr || !q->status) return DRGNN_E_ARG;
    const int64_t T = q->n_atoms, R = q->n_residues, M = q->n_complexes, K = q->n_targets;
    if (T < 0 || R < 0 || M < 0 || K < 0 || T > INT32_MAX / 3 || R >= INT32_MAX || K > k_max) return DRGNN_E_ARG;
    if ((M > 0 && !q->res_ptr) || (R > 0 && !q->atom_ptr) || (T > 0 && !q->xyz)) return DRGNN_E_ARG;
    if (K > 0 && (!q->host_target_res || !q->host_target_complex || !q->target_res || !q->target_complex || !q->out)) return DRGNN_E_ARG;
    return 0;
}
template <class Request>
static int residue_tables_check(const Request* q, const int32_t* sp) {
    const int32_t* rp = q->host_res_ptr;
    if (!ragged_check(q->host_atom_ptr, rp, sp, q->n_atoms, q->n_residues, q->n_complexes) ||
        !targets_check(q->host_target_complex, q->host_target_res, rp, q->n_complexes, q->n_targets))
        return DRGNN_E_ARG;
    return 0;
}

extern "C" {

// ---- buried surface area of residues (drgnn_bsa.h) ---------------------------------------------------
DRGNN_CAPACITY(drgnn_bsa_capacity, BS_NCAP, BS_CCAP, BS_MAX_SLICES, BS_MAX_TARGETS)

int drgnn_bsa_residues(const drgnn_bsa_request* q, void* stream) {
    if (int rc = residue_request_check(q, INT32_MAX)) return rc;
    const int64_t T = q->n_atoms, M = q->n_complexes, K = q->n_targets, NR = q->n_radii;
    if (NR < 0 || (M > 0 && (!q->host_res_split || !q->res_split))) return DRGNN_E_ARG;
    if (T > 0 && (!q->rad_complex || !q->rad_unbound || NR < 1 || T % NR != 0)) return DRGNN_E_ARG;
    if (!(q->probe >= 0.0) || q->n_slices < 1) return DRGNN_E_ARG;
    if (q->n_slices > BS_MAX_SLICES || K > BS_MAX_TARGETS) return DRGNN_E_CAPACITY;
    if (int rc = residue_tables_check(q, q->host_res_split)) return rc;
    if (K == 0) return 0;
    BsaArgs a;
    memset(&a, 0, sizeof(a));
    a.xyz = q->xyz; a.atom_ptr = q->atom_ptr; a.res_ptr = q->res_ptr; a.res_split = q->res_split;
    a.rad_c = q->rad_complex; a.rad_u = q->rad_unbound; a.tgt_res = q->target_res; a.tgt_cx = q->target_complex;
    a.n_radii = (int)NR; a.n_slices = q->n_slices; a.probe = (float)q->probe; a.probe_d = q->probe;
    a.out = q->out; a.status = q->status;
    static_assert(sizeof(BsaShared) <= DRGNN_LDS_LIMIT, "the workgroup's lists fit the LDS");
    DRGNN_EMU_ONLY(std::unique_ptr<BsaShared> lds(new BsaShared);)
    DRGNN_LAUNCH(k_bsa_residues, grid1(K, DRGNN_NTHREADS, sizeof(BsaShared)), stream, bsa_residue(a, bx, *lds), a);
    return 0;
}

// ---- half-sphere exposure of residues (drgnn_hse.h) --------------------------------------------------
DRGNN_CAPACITY(drgnn_hse_capacity, HS_RCAP, HS_MAX_TILES)

int drgnn_hse_residues(const drgnn_hse_request* q, void* stream) {
    if (int rc = residue_request_check(q, INT32_MAX / 3)) return rc;
    const int64_t R = q->n_residues, K = q->n_targets, NT = q->n_tiles, NB = q->n_rows;
    if (!q->host_tile_ptr || NT < 0 || NB < 0) return DRGNN_E_ARG;
    if (R > 0 && (!q->bb || !q->host_bb || NB < 1 || R % NB != 0)) return DRGNN_E_ARG;
    if (K > 0 && (!q->tile_ptr || NT < 1)) return DRGNN_E_ARG;
    if (!(q->radius > 0.0) || !(q->radius < 1.0e150) || !(q->connect_cutoff > 0.0) || !(q->connect_cutoff < 1.0e150) ||
        q->offset < 0)
        return DRGNN_E_ARG;
    if (q->connect_a < 0 || q->connect_a > 3 || q->connect_b < 0 || q->connect_b > 3 || q->direction < 0 || q->direction > 1)
        return DRGNN_E_ARG;
    if (NT > HS_MAX_TILES) return DRGNN_E_CAPACITY;
    const int32_t *ap = q->host_atom_ptr, *tp = q->host_tile_ptr, *hb = q->host_bb;
    if (int rc = residue_tables_check(q, nullptr)) return rc;
    if (tp[0] != 0 || tp[NT] != K) return DRGNN_E_ARG;
    for (int64_t r = 0; r < R; ++r) {
        const int32_t* row = hb + 5 * (r % NB);                       // every offset the kernel may add lies in its residue
        for (int j = 0; j < 4; ++j)
            if (row[j] < -1 || row[j] >= ap[r + 1] - ap[r]) return DRGNN_E_ARG;
    }
    for (int64_t t = 0; t < NT; ++t) {
        if (tp[t + 1] < tp[t] || tp[t + 1] > K) return DRGNN_E_ARG;
        for (int64_t k = tp[t] + 1; k < tp[t + 1]; ++k)               // a tile serves one complex
            if (q->host_target_complex[k] != q->host_target_complex[tp[t]]) return DRGNN_E_ARG;
    }
    if (K == 0) return 0;
    HseArgs a;
    memset(&a, 0, sizeof(a));
    a.xyz = q->xyz; a.atom_ptr = q->atom_ptr; a.res_ptr = q->res_ptr; a.bb = q->bb;
    a.tgt_res = q->target_res; a.tgt_cx = q->target_complex; a.tile_ptr = q->tile_ptr;
    a.n_rows = (int)NB; a.offset = q->offset; a.con_a = q->connect_a; a.con_b = q->connect_b; a.direction = q->direction;
    a.radius2 = q->radius * q->radius; a.cut2 = q->connect_cutoff * q->connect_cutoff;
    a.out = q->out; a.status = q->status;
    static_assert(sizeof(HseShared) <= 64 * 1024, "the staged CAs fit the static LDS of a workgroup");
    DRGNN_EMU_ONLY(std::unique_ptr<HseShared> lds(new HseShared);)
    DRGNN_LAUNCH(k_hse_residues, grid1(NT), stream, hse_tile(a, (int)bx, *lds), a);
    return 0;
}

// ---- residue depth (drgnn_depth.h) -------------------------------------------------------------------
DRGNN_CAPACITY(drgnn_depth_capacity, DP_DOTS_CAP, DP_CX_DOTS_CAP, DP_MAX_GRID)

// the workspace's arrays, one after the other, each a multiple of 8 bytes: mask, pos, id, label, size, cnt, ptr, cx_nd,
// cx_outer; offsets[9] is the size
static int depth_layout(int64_t T, int64_t M, int64_t n_dots, int64_t* off) {
    if (T < 0 || M < 0 || n_dots < 1 || n_dots > DP_DOTS_CAP || T > INT32_MAX / 3 || M > INT32_MAX) return -1;
    const int64_t W = (n_dots + 63) / 64, D = T * n_dots;
    const int64_t i32D = (4 * D + 7) / 8 * 8, i32T = (4 * T + 7) / 8 * 8, i32M = (4 * M + 7) / 8 * 8;
    const int64_t sizes[9] = {8 * T * W, 24 * D, i32D, i32D, i32D, i32T, i32T, i32M, i32M};
    off[0] = 0;
    for (int j = 0; j < 9; ++j) off[j + 1] = off[j] + sizes[j];
    return 0;
}

int64_t drgnn_depth_workspace(int64_t n_atoms, int64_t n_complexes, int32_t n_dots, int64_t* offsets) {
    int64_t off[10];
    if (depth_layout(n_atoms, n_complexes, n_dots, off) != 0) return -1;
    if (offsets) memcpy(offsets, off, sizeof(off));
    return off[9];
}

int drgnn_depth_residues(const drgnn_depth_request* q, void* stream) {
    if (int rc = residue_request_check(q, INT32_MAX)) return rc;
    const int64_t T = q->n_atoms, M = q->n_complexes, K = q->n_targets, NR = q->n_radii;
    if (NR < 0 || (T > 0 && (!q->radii || NR < 1 || T % NR != 0))) return DRGNN_E_ARG;
    if (q->n_dots < 1 || !q->dots || !(q->probe > 0.0) || !(q->probe < 1.0e150) || !(q->link >= 0.0) || !(q->link < 1.0e150) ||
        q->components < 0 || q->components > 1 || q->phases < 0 || q->phases > 7)
        return DRGNN_E_ARG;
    if (q->n_dots > DP_DOTS_CAP || K > DP_MAX_GRID || M > DP_MAX_GRID || T / DRGNN_NWAVES >= DP_MAX_GRID) return DRGNN_E_CAPACITY;
    if (int rc = residue_tables_check(q, nullptr)) return rc;
    int64_t off[10];
    if (depth_layout(T, M, q->n_dots, off) != 0) return DRGNN_E_ARG;
    int ph = q->phases == 0 ? 7 : q->phases;
    if (K == 0) ph = q->phases == 0 ? 0 : ph & ~4;                      // (the whole call without a target: nothing to do)
    if (M == 0) ph = 0;
    if (ph == 0) return 0;
    if (int rc = workspace_check(q->workspace, q->workspace_bytes, off[9], 8)) return rc;
    DepthArgs a;
    memset(&a, 0, sizeof(a));
    a.xyz = q->xyz; a.atom_ptr = q->atom_ptr; a.res_ptr = q->res_ptr; a.rad = q->radii; a.dots = q->dots;
    a.tgt_res = q->target_res; a.tgt_cx = q->target_complex;
    a.n_atoms = (int)T; a.n_cx = (int)M; a.n_radii = (int)NR; a.n_dots = q->n_dots; a.words = (q->n_dots + 63) / 64;
    a.all = q->components;
    a.probe = q->probe; a.link = q->link; a.link2 = q->link * q->link;
    char* w = (char*)q->workspace;
    a.mask = (unsigned long long*)(w + off[0]); a.pos = (double*)(w + off[1]); a.id = (int32_t*)(w + off[2]);
    a.label = (int32_t*)(w + off[3]); a.size = (int32_t*)(w + off[4]); a.cnt = (int32_t*)(w + off[5]);
    a.ptr = (int32_t*)(w + off[6]); a.cx_nd = (int32_t*)(w + off[7]); a.cx_outer = (int32_t*)(w + off[8]);
    a.out = q->out; a.status = q->status;
#ifdef DRGNN_EMU   // the emulation's workgroup is one "wave": its tile is an atom, the device's DRGNN_NWAVES atoms
    const int64_t tiles = T;
#else
    const int64_t tiles = (T + DRGNN_NWAVES - 1) / DRGNN_NWAVES;
#endif
    DRGNN_EMU_ONLY(std::unique_ptr<DepthShared> lds(new DepthShared);)
    if (ph & 1) DRGNN_LAUNCH(k_depth_dots, grid1(tiles), stream, depth_dots_tile(a, bx), a);
    if (ph & 2) DRGNN_LAUNCH(k_depth_components, grid1(M), stream, depth_components(a, (int)bx, *lds), a);
    if (ph & 4) DRGNN_LAUNCH(k_depth_residues, grid1(K), stream, depth_residue(a, bx, *lds), a);
    return 0;
}

}  // extern "C"
