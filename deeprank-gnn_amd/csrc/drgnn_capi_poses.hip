// drgnn_capi_poses.hip -- the entry points of dock_scores.py and poses.py: docking scores, lDDT, contacts / common contacts /
// FCC clustering, contact consensus, pairwise RMSD and RMSD clustering of docking poses, with the __global__ wrappers they
// launch.  Both clusterings launch k_fcc_greedy and one instantiation of the relation kernel (pose_cluster_run), which is why
// they share a unit.  One of the drgnn_capi*.hip units (drgnn_capi.hip says how they are built and what an entry point looks
// like).
#include "drgnn_capi_common.h"
#include "drgnn_score.h"
#include "drgnn_lddt.h"
#include "drgnn_posecluster.h"
#include "drgnn_fcc.h"
#include "drgnn_consensus.h"
#include "drgnn_rmsd.h"

#ifndef DRGNN_EMU
// docking scores (drgnn_score.h): one workgroup per pose
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_dock_scores(ScoreArgs a) {
    __shared__ double smem_sc[SC_LDS_BYTES / 8];
    score_pose(a, (int64_t)blockIdx.x, smem_sc);
}
// fraction of common contacts (drgnn_fcc.h): one workgroup per pose; per tile of pose pairs; a wave per word of the
// neighbour relation; ONE workgroup for the greedy clustering of either rule (drgnn_posecluster.h)
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_fcc_contacts(FccContactArgs a) {
    __shared__ FccContactShared smem_fc;
    fc_pose(a, (int64_t)blockIdx.x, smem_fc);
}
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_fcc_common(FccCommonArgs a) {
    __shared__ FccCommonShared smem_fm;
    fc_common(a, (int)blockIdx.y, (int)blockIdx.x, smem_fm);
}
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_fcc_relation(FccRule r, PoseClusterArgs a) { pc_relation(r, a, (int64_t)blockIdx.x); }
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_fcc_greedy(PoseClusterArgs a) {
    __shared__ PoseGreedyShared smem_fg;
    pc_greedy(a, smem_fg);
}
// contact consensus of poses (drgnn_consensus.h): a wave per list entry; one workgroup per pose; per CS_BW words of a group (the
// group by y)
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_cons_count(ConsCountArgs a) { cs_count(a, (int)blockIdx.x, (int)gridDim.x); }
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_cons_numer(ConsNumerArgs a) {
    __shared__ ConsNumerShared smem_cn;
    cs_numer(a, (int64_t)blockIdx.x, smem_cn);
}
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_cons_bits(ConsBitsArgs a) { cs_bits(a, (int)blockIdx.y, (int)blockIdx.x); }
// lDDT of poses (drgnn_lddt.h): one workgroup per LD_RB residues (x) and PP poses (y); an item per word of counts
template <int PP, int KT> __global__ void __launch_bounds__(DRGNN_NTHREADS) k_pose_lddt(LddtArgs a) {
    __shared__ LddtShared smem_ld;
    ld_block<PP, KT>(a, (int)blockIdx.x, a.m0 + (int64_t)blockIdx.y * PP, smem_ld);
}
__global__ void __launch_bounds__(256) k_lddt_halve(LddtArgs a) { ld_halve_item(a, a.m0 + (int64_t)blockIdx.x * 256 + threadIdx.x); }
// pairwise pose RMSD (drgnn_rmsd.h): one workgroup per pose of one side; per tile of pose pairs; a wave per word of the
// neighbour relation (the greedy clustering is k_fcc_greedy)
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_rmsd_prepare(RmsdArgs a, int side) {
    __shared__ RmsdPrepShared smem_rp;
    rm_prepare(a, side, (int64_t)blockIdx.x, smem_rp);
}
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_rmsd_pairs(RmsdArgs a) {
    __shared__ RmsdPairShared smem_rq;
    rm_pairs(a, (int)blockIdx.y, (int)blockIdx.x, smem_rq);
}
__global__ void __launch_bounds__(DRGNN_NTHREADS) k_rmsd_relation(DistRule r, PoseClusterArgs a) { pc_relation(r, a, (int64_t)blockIdx.x); }
#endif  // !DRGNN_EMU

// ---- clustering of poses (drgnn_posecluster.h) ---------------------------------------------------------
// The part of drgnn_pose_cluster / drgnn_pose_cluster_dist that does not depend on the rule, after the entry point's own checks:
// the shared checks, then the relation of `rule` and the greedy loop on it.  `q` is either request: their shared fields
// have the same names; `relation` is the rule's instantiation of the relation kernel, DRGNN_KERNEL(k_..._relation).
template <class Rule, class Request, class Kernel>
static int pose_cluster_run(Rule rule, const Request* q, Kernel relation, void* stream) {
    const int64_t M = q->n_poses;
    if (M < 0 || q->min_size < 1 || !q->n_clusters) return DRGNN_E_ARG;
    if (M > 0 && (!q->neighbours || !q->transposed || !q->labels || !q->centres || !q->sizes)) return DRGNN_E_ARG;
    if (M > PC_CCAP) return DRGNN_E_CAPACITY;
    if (M == 0) return 0;
    PoseClusterArgs a;
    memset(&a, 0, sizeof(a));
    rule.n = a.n = (int)M; a.min_size = q->min_size;
    a.nb = (pc_word*)q->neighbours; a.nbt = (pc_word*)q->transposed;
    a.labels = q->labels; a.centres = q->centres; a.sizes = q->sizes; a.n_clusters = q->n_clusters;
    const int64_t words = M * ((M + 63) / 64), blocks = (words + DRGNN_NWAVES - 1) / DRGNN_NWAVES;
    DRGNN_EMU_ONLY(std::unique_ptr<PoseGreedyShared> lds(new PoseGreedyShared);)
    DRGNN_LAUNCH(relation, grid1(blocks), stream, pc_relation(rule, a, bx), rule, a);
    DRGNN_LAUNCH(k_fcc_greedy, grid1(1), stream, pc_greedy(a, *lds), a);
    return 0;
}

// the launches of drgnn_pose_lddt for PP poses per pass and KT thresholds at most: at most LD_MAX_Y passes and LD_MAX_WGS
// workgroups each (a template cannot stand inside extern "C")
template <int PP, int KT>
static int lddt_launches(LddtArgs a, int64_t n_blocks, void* stream) {
    DRGNN_EMU_ONLY(std::unique_ptr<LddtShared> lds(new LddtShared);)
    const int64_t passes = (a.n_poses + PP - 1) / PP, step = std::max<int64_t>(1, std::min<int64_t>(LD_MAX_Y, LD_MAX_WGS / n_blocks));
    for (int64_t p0 = 0; p0 < passes; p0 += step) {
        a.m0 = p0 * PP;
        DRGNN_LAUNCH((k_pose_lddt<PP, KT>), grid2(n_blocks, std::min(step, passes - p0)), stream,
                     (ld_block<PP, KT>(a, (int)bx, a.m0 + by * PP, *lds)), a);
    }
    return 0;
}

extern "C" {

// ---- docking scores of pose batches (drgnn_score.h) -------------------------------------------------
int drgnn_dock_scores(const drgnn_score_request* q, void* stream) {
    if (!q || !q->host_zone_ptr || !q->host_zone_atom || !q->host_atom_ptr || !q->zone_atom || !q->zone_ref ||
        !q->atom_ptr || !q->xyz || !q->scores || !q->classes || !q->n_preserved)
        return DRGNN_E_ARG;
    const int64_t M = q->n_poses, T = q->n_atoms, R = q->n_residues, P = q->n_pairs;
    if (M < 0 || T < 1 || R < 1 || P < 0 || q->n_ref_pairs < 1 || P > q->n_ref_pairs || !(q->fnat_cutoff >= 0.0))
        return DRGNN_E_ARG;
    if (P > 0 && (!q->pair_res || !q->host_pair_res)) return DRGNN_E_ARG;
    if (M > INT32_MAX || T > INT32_MAX / 3 || R >= INT32_MAX || q->n_ref_pairs > INT32_MAX) return DRGNN_E_CAPACITY;
    const int32_t *zp = q->host_zone_ptr, *za = q->host_zone_atom, *ap = q->host_atom_ptr, *pr = q->host_pair_res;
    if (zp[0] != 0) return DRGNN_E_ARG;
    for (int z = 0; z < 3; ++z)
        if (zp[z + 1] < zp[z] || zp[z + 1] - zp[z] < 3) return DRGNN_E_ARG;
    for (int64_t i = 0; i < zp[3]; ++i)
        if (za[i] < 0 || za[i] >= T) return DRGNN_E_ARG;
    if (!ragged_check(ap, nullptr, nullptr, T, R, 0)) return DRGNN_E_ARG;
    int amax = 1;
    for (int64_t p = 0; p < P; ++p) {
        const int32_t ra = pr[2 * p], rb = pr[2 * p + 1];
        if (ra < 0 || ra >= R || rb < 0 || rb >= R) return DRGNN_E_ARG;
        amax = std::max(amax, ap[ra + 1] - ap[ra]);
    }
    if ((int64_t)amax * SC_PCHUNK > INT32_MAX) return DRGNN_E_CAPACITY;
    if (M == 0) return 0;
    ScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.xyz = q->xyz; a.zone_atom = q->zone_atom; a.zone_ref = q->zone_ref; a.pair_res = q->pair_res; a.atom_ptr = q->atom_ptr;
    for (int z = 0; z < 4; ++z) a.zp[z] = zp[z];
    a.n_atoms = (int)T; a.n_pairs = (int)P; a.n_ref_pairs = (int)q->n_ref_pairs; a.amax = amax;
    a.cut2 = (float)(q->fnat_cutoff * q->fnat_cutoff);
    a.scores = q->scores; a.classes = q->classes; a.n_preserved = q->n_preserved;
    DRGNN_EMU_ONLY(std::vector<double> lds(SC_LDS_BYTES / 8 + 1);)
    DRGNN_LAUNCH(k_dock_scores, grid1(M), stream, score_pose(a, bx, lds.data()), a);
    return 0;
}

// ---- lDDT and interface lDDT of pose batches (drgnn_lddt.h) -------------------------------------------
int drgnn_pose_lddt(const drgnn_lddt_request* q, void* stream) {
    if (!q || !q->host_entry_ptr || !q->entry_ptr || !q->xyz || !q->counts) return DRGNN_E_ARG;
    const int64_t M = q->n_poses, T = q->n_atoms, R = q->n_residues, E = q->n_entries, K = q->n_thresholds;
    if (M < 0 || T < 1 || R < 1 || E < 0 || q->n_chain_a_atoms < 0 || q->n_chain_a_atoms > T) return DRGNN_E_ARG;
    if (K < 1 || K > LD_KMAX || (q->poses_per_pass != 0 && q->poses_per_pass != 1 && q->poses_per_pass != LD_PPMAX)) return DRGNN_E_ARG;
    for (int64_t k = 0; k < K; ++k)                                    // (a NaN fails both)
        if (!(q->thresholds[k] >= 0.0) || !(q->thresholds[k] < 1.0e150) || (k > 0 && !(q->thresholds[k] > q->thresholds[k - 1])))
            return DRGNN_E_ARG;
    if (E > 0 && (!q->self_atom || !q->other_atom || !q->d_ref || !q->host_self_atom || !q->host_other_atom)) return DRGNN_E_ARG;
    const int64_t n_blocks = (R + LD_RB - 1) / LD_RB;
    if (M > INT32_MAX || T > INT32_MAX / 3 || E > INT32_MAX || R >= INT32_MAX || n_blocks > LD_MAX_WGS) return DRGNN_E_CAPACITY;
    const int32_t *ep = q->host_entry_ptr, *sa = q->host_self_atom, *oa = q->host_other_atom;
    if (ep[0] != 0 || ep[R] != E) return DRGNN_E_ARG;
    for (int64_t r = 0; r < R; ++r)
        if (ep[r + 1] < ep[r]) return DRGNN_E_ARG;
    for (int64_t e = 0; e < E; ++e)
        if (sa[e] < 0 || sa[e] >= T || oa[e] < 0 || oa[e] >= T) return DRGNN_E_ARG;
    if (M == 0) return 0;
    LddtArgs a;
    memset(&a, 0, sizeof(a));
    a.xyz = q->xyz; a.entry_ptr = q->entry_ptr; a.self_atom = q->self_atom; a.other_atom = q->other_atom; a.d_ref = q->d_ref;
    for (int64_t k = 0; k < K; ++k) a.t[k] = q->thresholds[k];
    a.n_thresholds = (int)K; a.n_atoms = (int)T; a.n_residues = (int)R; a.first_b = (int)q->n_chain_a_atoms; a.n_poses = M;
    a.counts = q->counts; a.residue_counts = q->residue_counts;
    if (int rc = drgnn_clear(q->counts, (size_t)(M * 2 * K) * sizeof(int32_t), stream)) return rc;
    // four poses to a pass share an entry's loads and bounds: taken once such passes still give every compute unit several
    // workgroups (profiles/lddt_ab.txt: 1 024 poses of 1ATN 6.1 against 6.9 ms; at 64 poses, 160 such workgroups, the two are
    // within their spread, 0.88 - 0.91 ms, of which the checks above are 0.76)
    const int pp = q->poses_per_pass ? q->poses_per_pass : (n_blocks * ((M + LD_PPMAX - 1) / LD_PPMAX) >= LD_FILL ? LD_PPMAX : 1);
    int rc;
    if (pp == 1) rc = K <= 4 ? lddt_launches<1, 4>(a, n_blocks, stream) : lddt_launches<1, LD_KMAX>(a, n_blocks, stream);
    else rc = K <= 4 ? lddt_launches<LD_PPMAX, 4>(a, n_blocks, stream) : lddt_launches<LD_PPMAX, LD_KMAX>(a, n_blocks, stream);
    if (rc) return rc;
    const int64_t words = M * 2 * K, span = (int64_t)LD_MAX_WGS * 256;
    for (a.m0 = 0; a.m0 < words; a.m0 += span)                         // (m0: here the first word of the launch)
        DRGNN_LAUNCH(k_lddt_halve, grid_items(std::min(span, words - a.m0)), stream, ld_halve_item(a, a.m0 + bx), a);
    return 0;
}

// ---- clustering of poses by their fraction of common contacts (drgnn_fcc.h) --------------------------
DRGNN_CAPACITY(drgnn_fcc_capacity, FC_RCAP, FC_PCAP, PC_CCAP)

int drgnn_pose_contacts(const drgnn_pose_contacts_request* q, void* stream) {
    if (!q || !q->host_atom_ptr) return DRGNN_E_ARG;
    const int64_t M = q->n_poses, T = q->n_atoms, R = q->n_residues, A = q->n_chain_a;
    if (M < 0 || T < 0 || R < 0 || A < 0 || A > R || M > INT32_MAX || T > INT32_MAX / 3) return DRGNN_E_ARG;
    if (!(q->cutoff > 0.0) || !(q->cutoff < 1.0e18)) return DRGNN_E_ARG;              // (its square is a finite fp32)
    if (!q->atom_ptr || (M > 0 && !q->n_contacts) || (M > 0 && T > 0 && !q->xyz)) return DRGNN_E_ARG;
    if (R > FC_RCAP) return DRGNN_E_CAPACITY;
    const int64_t WB = (R - A + 63) / 64;
    if (M > 0 && A * WB > 0 && !q->bits) return DRGNN_E_ARG;
    const int32_t* ap = q->host_atom_ptr;
    if (!ragged_check(ap, nullptr, nullptr, T, R, 0)) return DRGNN_E_ARG;
    if (M == 0) return 0;
    FccContactArgs a;
    memset(&a, 0, sizeof(a));
    a.xyz = q->xyz; a.atom_ptr = q->atom_ptr; a.n_atoms = (int)T; a.n_res = (int)R; a.n_a = (int)A;
    a.cut = (float)q->cutoff; a.cut2 = (float)(q->cutoff * q->cutoff);
    a.bits = (pc_word*)q->bits; a.n_contacts = q->n_contacts;
    static_assert(sizeof(FccContactShared) <= 64 * 1024, "the spheres fit the static LDS of a workgroup");
    DRGNN_EMU_ONLY(std::unique_ptr<FccContactShared> lds(new FccContactShared);)
    DRGNN_LAUNCH(k_fcc_contacts, grid1(M), stream, fc_pose(a, bx, *lds), a);
    return 0;
}

int drgnn_pose_common(const drgnn_pose_common_request* q, void* stream) {
    if (!q) return DRGNN_E_ARG;
    const int64_t Ma = q->n_a, Mb = q->n_b, W = q->n_words;
    if (Ma < 0 || Mb < 0 || W < 0 || W > INT32_MAX) return DRGNN_E_ARG;
    if (Ma > 0 && Mb > 0 && (!q->common || (W > 0 && (!q->bits_a || !q->bits_b)))) return DRGNN_E_ARG;
    if (Ma > FC_PCAP || Mb > FC_PCAP) return DRGNN_E_CAPACITY;
    if (Ma == 0 || Mb == 0) return 0;
    FccCommonArgs a;
    memset(&a, 0, sizeof(a));
    a.a = (const pc_word*)q->bits_a; a.b = (const pc_word*)q->bits_b; a.n_a = (int)Ma; a.n_b = (int)Mb; a.n_words = W;
    a.common = q->common;
    const int ti = (int)((Ma + FC_TILE - 1) / FC_TILE), tj = (int)((Mb + FC_TILE - 1) / FC_TILE);
    static_assert(FC_TILE * FC_TILE == DRGNN_NTHREADS, "one lane per pose pair of a tile");
    static_assert((FC_PCAP + FC_TILE - 1) / FC_TILE <= 65535, "the tiles of a side fit the grid's y");
    DRGNN_EMU_ONLY(std::unique_ptr<FccCommonShared> lds(new FccCommonShared);)
    DRGNN_LAUNCH(k_fcc_common, grid2(tj, ti), stream, fc_common(a, (int)by, (int)bx, *lds), a);
    return 0;
}

int drgnn_pose_cluster(const drgnn_pose_cluster_request* q, void* stream) {
    if (!q) return DRGNN_E_ARG;
    if (!(q->cutoff_fcc > 0.0) || !(q->cutoff_fcc <= 1.0) || !(q->cutoff_reverse > 0.0) || !(q->cutoff_reverse <= 1.0))
        return DRGNN_E_ARG;
    if (q->n_poses > 0 && (!q->common || !q->n_contacts)) return DRGNN_E_ARG;
    FccRule rule;
    memset(&rule, 0, sizeof(rule));
    rule.common = q->common; rule.n_contacts = q->n_contacts; rule.cut_fwd = q->cutoff_fcc; rule.cut_rev = q->cutoff_reverse;
    return pose_cluster_run(rule, q, DRGNN_KERNEL(k_fcc_relation), stream);
}

// ---- contact consensus of poses (drgnn_consensus.h) ----------------------------------------------------
DRGNN_CAPACITY(drgnn_consensus_capacity, FC_RCAP, CS_GCAP, CS_ECAP, CS_NCAP, CS_PCAP)

// the counts shared by the three calls: 0, or the error
static int cons_shape(int64_t nA, int64_t nB, int64_t G) {
    if (nA < 0 || nB < 0 || G < 0) return DRGNN_E_ARG;
    if (nA + nB > FC_RCAP || G > CS_GCAP || G * nA * nB > CS_ECAP) return DRGNN_E_CAPACITY;      // (the product is below 2^38)
    return 0;
}

int drgnn_pose_contact_counts(const drgnn_contact_counts_request* q, void* stream) {
    if (!q || !q->host_group_ptr) return DRGNN_E_ARG;
    const int64_t M = q->n_poses, nA = q->n_chain_a, nB = q->n_chain_b, G = q->n_groups, L = q->n_listed;
    if (M < 0 || L < 0) return DRGNN_E_ARG;
    if (int e = cons_shape(nA, nB, G)) return e;
    if (M > CS_PCAP || L > CS_PCAP) return DRGNN_E_CAPACITY;
    const int64_t WB = (nB + 63) / 64;
    if (!q->group_ptr || (L > 0 && (!q->order || !q->host_order))) return DRGNN_E_ARG;
    if ((L > 0 && nA * WB > 0 && !q->bits) || (G * nA * nB > 0 && !q->counts) || (G * (nA + nB) > 0 && !q->residues)) return DRGNN_E_ARG;
    const int32_t* gp = q->host_group_ptr;
    if (gp[0] != 0 || gp[G] != L) return DRGNN_E_ARG;
    for (int64_t g = 0; g < G; ++g)
        if (gp[g + 1] < gp[g]) return DRGNN_E_ARG;
    for (int64_t p = 0; p < L; ++p)
        if (q->host_order[p] < 0 || q->host_order[p] >= M) return DRGNN_E_ARG;
    ConsCountArgs a;
    memset(&a, 0, sizeof(a));
    a.bits = (const pc_word*)q->bits; a.order = q->order; a.group_ptr = q->group_ptr; a.n_a = (int)nA; a.n_b = (int)nB;
    a.n_groups = (int)G; a.n_listed = L; a.counts = q->counts; a.residues = q->residues;
    const size_t count_bytes = (size_t)(G * nA * nB) * sizeof(int32_t), res_bytes = (size_t)(G * (nA + nB)) * sizeof(int32_t);
    const int blocks = (int)std::min<int64_t>((L + DRGNN_NWAVES - 1) / DRGNN_NWAVES, CS_COUNT_WGS);
    if (int rc = drgnn_clear(q->counts, count_bytes, stream)) return rc;
    if (int rc = drgnn_clear(q->residues, res_bytes, stream)) return rc;
    // (without residues a listed pose has no word to count: cs_count would write nothing)
    if (nA + nB > 0) DRGNN_LAUNCH(k_cons_count, grid1(blocks), stream, cs_count(a, (int)bx, blocks), a);
    return 0;
}

int drgnn_pose_consensus_numerators(const drgnn_consensus_numerators_request* q, void* stream) {
    if (!q) return DRGNN_E_ARG;
    const int64_t M = q->n_poses, nA = q->n_chain_a, nB = q->n_chain_b, G = q->n_groups;
    if (M < 0) return DRGNN_E_ARG;
    if (int e = cons_shape(nA, nB, G)) return e;
    if (M > CS_NCAP) return DRGNN_E_CAPACITY;
    const int64_t WB = (nB + 63) / 64;
    if (M > 0 && (!q->row || !q->host_row || !q->numerators || (nA * WB > 0 && !q->bits) || (G * nA * nB > 0 && !q->counts))) return DRGNN_E_ARG;
    for (int64_t m = 0; m < M; ++m)
        if (q->host_row[m] < -1 || q->host_row[m] >= G) return DRGNN_E_ARG;
    if (M == 0) return 0;
    ConsNumerArgs a;
    memset(&a, 0, sizeof(a));
    a.bits = (const pc_word*)q->bits; a.counts = q->counts; a.row = q->row; a.n_a = (int)nA; a.n_b = (int)nB;
    a.numerators = (long long*)q->numerators;
    DRGNN_EMU_ONLY(std::unique_ptr<ConsNumerShared> lds(new ConsNumerShared);)
    DRGNN_LAUNCH(k_cons_numer, grid1(M), stream, cs_numer(a, bx, *lds), a);
    return 0;
}

int drgnn_pose_consensus_bits(const drgnn_consensus_bits_request* q, void* stream) {
    if (!q) return DRGNN_E_ARG;
    const int64_t nA = q->n_chain_a, nB = q->n_chain_b, G = q->n_groups;
    if (int e = cons_shape(nA, nB, G)) return e;
    const int64_t WB = (nB + 63) / 64;
    if (G > 0 && (!q->min_count || !q->host_min_count || !q->n_contacts || (nA * WB > 0 && !q->bits) || (nA * nB > 0 && !q->counts))) return DRGNN_E_ARG;
    for (int64_t g = 0; g < G; ++g)
        if (q->host_min_count[g] < 1) return DRGNN_E_ARG;
    if (G == 0) return 0;
    ConsBitsArgs a;
    memset(&a, 0, sizeof(a));
    a.counts = q->counts; a.min_count = q->min_count; a.n_a = (int)nA; a.n_b = (int)nB;
    a.bits = (pc_word*)q->bits; a.n_contacts = q->n_contacts;
    const int blocks = (int)((nA * WB + CS_BW - 1) / CS_BW);
    static_assert(CS_GCAP <= 65535, "the groups fit the grid's y");
    if (int rc = drgnn_clear(q->n_contacts, (size_t)G * sizeof(int32_t), stream)) return rc;
    DRGNN_LAUNCH(k_cons_bits, grid2(blocks, G), stream, cs_bits(a, (int)by, (int)bx), a);
    return 0;
}

// ---- pairwise pose RMSD and RMSD clustering of poses (drgnn_rmsd.h) ----------------------------------
DRGNN_CAPACITY(drgnn_rmsd_capacity, RM_PCAP, PC_CCAP)

// records of side a, of side b; off[2] is the size
static int rmsd_layout(int64_t Ma, int64_t Mb, int64_t nF, int64_t nR, int64_t* off) {
    if (Ma < 0 || Mb < 0 || nF < 0 || nR < 0 || Ma > RM_PCAP || Mb > RM_PCAP || nF > INT32_MAX / 8 || nR > INT32_MAX / 8) return -1;
    const int64_t L = 3 * (nF + nR) + 2;
    off[0] = 0; off[1] = 8 * L * Ma; off[2] = 8 * L * (Ma + Mb);
    return 0;
}

int64_t drgnn_rmsd_workspace(int64_t n_a, int64_t n_b, int64_t n_fit, int64_t n_rms, int64_t* offsets) {
    int64_t off[3];
    if (rmsd_layout(n_a, n_b, n_fit, n_rms, off) != 0) return -1;
    if (offsets) memcpy(offsets, off, sizeof(off));
    return off[2];
}

int drgnn_pose_rmsd(const drgnn_pose_rmsd_request* q, void* stream) {
    if (!q) return DRGNN_E_ARG;
    const int64_t Ma = q->n_a, Mb = q->n_b, T = q->n_atoms, nF = q->n_fit, nR = q->n_rms;
    if (Ma < 0 || Mb < 0 || T < 0 || nF < 0 || nR < 1 || T > INT32_MAX / 3 || nF > INT32_MAX / 8 || nR > INT32_MAX / 8) return DRGNN_E_ARG;
    if (nF == 1 || nF == 2 || q->phases < 0 || q->phases > 3) return DRGNN_E_ARG;
    if (!q->rms_idx || !q->host_rms_idx || (nF > 0) != (q->fit_idx != nullptr) || (nF > 0) != (q->host_fit_idx != nullptr)) return DRGNN_E_ARG;
    for (int64_t k = 0; k < nR; ++k)
        if (q->host_rms_idx[k] < 0 || q->host_rms_idx[k] >= T) return DRGNN_E_ARG;
    for (int64_t k = 0; k < nF; ++k)
        if (q->host_fit_idx[k] < 0 || q->host_fit_idx[k] >= T) return DRGNN_E_ARG;
    if ((Ma > 0 && !q->xyz_a) || (Mb > 0 && !q->xyz_b) || (Ma > 0 && Mb > 0 && !q->d)) return DRGNN_E_ARG;
    if (Ma > RM_PCAP || Mb > RM_PCAP) return DRGNN_E_CAPACITY;
    if (Ma == 0 || Mb == 0) return 0;
    int64_t off[3];
    if (rmsd_layout(Ma, Mb, nF, nR, off) != 0) return DRGNN_E_ARG;
    if (int rc = workspace_check(q->workspace, q->workspace_bytes, off[2], 8)) return rc;
    const int ph = q->phases == 0 ? 3 : q->phases;
    RmsdArgs a;
    memset(&a, 0, sizeof(a));
    a.xyz_a = q->xyz_a; a.xyz_b = q->xyz_b; a.fit_idx = q->fit_idx; a.rms_idx = q->rms_idx;
    a.n_atoms = (int)T; a.n_fit = (int)nF; a.n_rms = (int)nR; a.n_a = (int)Ma; a.n_b = (int)Mb;
    a.same = q->xyz_a == q->xyz_b && Ma == Mb;
    a.rec_a = (double*)((char*)q->workspace + off[0]);
    a.rec_b = a.same ? a.rec_a : (double*)((char*)q->workspace + off[1]);
    a.d = q->d;
    const int ti = (int)((Ma + RM_TILE - 1) / RM_TILE), tj = (int)((Mb + RM_TILE - 1) / RM_TILE);
    static_assert(RM_TILE * RM_TILE == DRGNN_NTHREADS, "one lane per pose pair of a tile");
    static_assert(RM_K % 2 == 0 && sizeof(RmsdPairShared) <= 64 * 1024, "odd rows; the staged atoms fit the static LDS of a workgroup");
    static_assert((RM_PCAP + RM_TILE - 1) / RM_TILE <= 65535, "the tiles of a side fit the grid's y");
    if (ph & 1) {
        DRGNN_EMU_ONLY(std::unique_ptr<RmsdPrepShared> lds(new RmsdPrepShared);)
        DRGNN_LAUNCH(k_rmsd_prepare, grid1(Ma), stream, rm_prepare(a, 0, bx, *lds), a, 0);
        if (!a.same) DRGNN_LAUNCH(k_rmsd_prepare, grid1(Mb), stream, rm_prepare(a, 1, bx, *lds), a, 1);
    }
    if (ph & 2) {
        DRGNN_EMU_ONLY(std::unique_ptr<RmsdPairShared> lds(new RmsdPairShared);)
        DRGNN_LAUNCH(k_rmsd_pairs, grid2(tj, ti), stream, rm_pairs(a, (int)by, (int)bx, *lds), a);
    }
    return 0;
}

int drgnn_pose_cluster_dist(const drgnn_pose_cluster_dist_request* q, void* stream) {
    if (!q) return DRGNN_E_ARG;
    if (!(q->cutoff > 0.0) || !(q->cutoff < HUGE_VAL)) return DRGNN_E_ARG;
    if (q->n_poses > 0 && !q->d) return DRGNN_E_ARG;
    DistRule rule;
    memset(&rule, 0, sizeof(rule));
    rule.d = q->d; rule.cutoff = q->cutoff;
    return pose_cluster_run(rule, q, DRGNN_KERNEL(k_rmsd_relation), stream);
}

}  // extern "C"
