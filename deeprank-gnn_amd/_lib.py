"""ctypes binding of the C ABI in include/drgnn.h.

``get()`` loads ``csrc/libdrgnn.so`` (built by ``__graft_entry__.build()`` /
``make -C deeprank-gnn_amd/csrc``) and raises if it is missing: there is no CPU fallback.
``Api`` itself is device-agnostic pointer plumbing (it only reads ``data_ptr()``), which
is what lets the CPU test-suite drive the host-emulation build of the same kernels.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DRGNN_LIB: use another build of the same library (profiling / ablation builds under tools/)
LIB_PATH = os.environ.get("DRGNN_LIB") or os.path.join(_HERE, "csrc", "libdrgnn.so")

GINET, SGAT, FOUT = 0, 1, 2
MAX_BRANCH = 2
LDS_LIMIT = 160 * 1024     # LDS bytes one workgroup may allocate (gfx950)
HEAD_MAX_HIDDEN = 512      # hidden units of the FC head the launch pair takes (drgnn_net_backward_fused_head: DRGNN_E_WIDTH beyond)

# enum drgnn_topo_i32 / drgnn_topo_f32 (include/drgnn.h)
TI = {name: i for i, name in enumerate([
    "NPTR", "EPTR", "ROWPTR0", "COL0", "EID0", "COLPTR0", "ROWIDX0", "TSLOT0", "CL0", "NC0",
    "MPTR0", "MEM0", "ROWPTR1", "COL1", "NE1", "COLPTR1", "ROWIDX1", "TSLOT1", "CL1", "NC1",
    "MPTR1", "MEM1", "CPTR0", "E1PTR", "CPTR1", "ERR", "GSTAT", "HORD", "HMP0", "HSPLIT", "IHORD"])}
TI_COUNT = len(TI)
TF = {"W0": 0, "W1": 1}
TF_COUNT = 2

FAULT_EXCHANGE = 1      # DRGNN_FAULT_EXCHANGE (step2[2])
STATUS_BITS = {1: "edge endpoint outside its graph's node range",
               2: "batch vector / edge list not grouped by graph",
               4: "cluster ids of one graph span too large a range",
               8: "len(cluster1) != number of depth-0 clusters"}

_c_i64 = ctypes.c_int64
_c_i32 = ctypes.c_int32
_vp = ctypes.c_void_p


class ConvParams(ctypes.Structure):
    _fields_ = [("w_nbr", _vp), ("nbr_sk", _c_i64), ("nbr_sh", _c_i64),
                ("w_self", _vp), ("self_sk", _c_i64), ("self_sh", _c_i64),
                ("bias", _vp)]


class ConvGrads(ctypes.Structure):
    _fields_ = [("w_nbr", _vp), ("w_self", _vp), ("bias", _vp)]


class NetDesc(ctypes.Structure):
    _fields_ = [("kind", _c_i32), ("n_branch", _c_i32), ("n_feat", _c_i32), ("reserved", _c_i32),
                ("conv1", ConvParams * MAX_BRANCH), ("conv2", ConvParams * MAX_BRANCH)]


class EnsMember(ctypes.Structure):
    """drgnn_ens_member: one entry of an ensemble's member table (its array lives in device memory)"""
    _fields_ = [("net", NetDesc), ("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp)]


class CohortMember(ctypes.Structure):
    """drgnn_cohort_member: one entry of a training cohort's member table (its array lives in device memory)"""
    _fields_ = EnsMember._fields_ + [
                ("flat_param", _vp), ("flat_grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp),
                ("step2", _vp), ("pred", _vp), ("readout", _vp), ("head_partials", _vp), ("partials", _vp), ("loss", _vp),
                ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("seed", ctypes.c_uint32), ("reserved", _c_i32)]


class TopologyRequest(ctypes.Structure):
    _fields_ = [("edge_index", _vp), ("edge_attr", _vp), ("batch", _vp), ("cluster0", _vp), ("cluster1", _vp),
                ("node_ptr", _vp), ("edge_ptr", _vp), ("c1_ptr", _vp),
                ("n_nodes", _c_i64), ("n_edges", _c_i64), ("len_cluster1", _c_i64), ("n_graphs", _c_i64),
                ("max_nodes", _c_i32), ("max_edges", _c_i32),
                ("ws_i32", _vp), ("ws_f32", _vp), ("scratch_i32", _vp),
                # resident-set mode (include/drgnn.h); left NULL by the Python-level Topology
                ("set", _vp), ("ids", _vp), ("x_out", _vp), ("y_out", _vp),
                ("flags", _c_i32), ("reserved", _c_i32),
                ("x", _vp), ("tiles", _vp), ("n_feat", _c_i32), ("reserved2", _c_i32)]


TOPO_HIER = 1          # drgnn_topology_request.flags: also build the hierarchical node order (HORD / HMP0 / HSPLIT)
TOPO_LEAN = 2          # ... and ONLY what the aggregation-first training kernels read (no CSC0, no depth-0 member lists)
TOPO_TILES = 4         # ... and the level-0 neighbour aggregation of every node (drgnn_topology_request.x / tiles)
METRICS_COUNTS, METRICS_REGRESSION, METRICS_RANKING = 1, 2, 4     # drgnn_metrics: what to compute


class GraphSet(ctypes.Structure):
    """drgnn_graph_set: the dataset resident in HBM, graph-major (include/drgnn.h)."""
    _fields_ = [("n_graphs", _c_i64), ("n_nodes", _c_i64), ("n_edges", _c_i64), ("len_cluster1", _c_i64),
                ("n_feat", _c_i32), ("y_bytes", _c_i32),
                ("node_ptr", _vp), ("edge_ptr", _vp), ("c1_ptr", _vp),
                ("x", _vp), ("edge_index", _vp), ("edge_attr", _vp),
                ("cluster0", _vp), ("cluster1", _vp), ("y", _vp)]


class EpochPlan(ctypes.Structure):
    """drgnn_epoch_plan (include/drgnn.h); pointer members are filled by FusedTrainer.train_epoch."""
    _fields_ = [("set", _vp), ("host_node_ptr", _vp), ("host_edge_ptr", _vp), ("host_c1_ptr", _vp),
                ("ids", _vp), ("host_ids", _vp), ("n_ids", _c_i64),
                ("batch_size", _c_i32), ("need_weights", _c_i32), ("inference", _c_i32), ("reserved", _c_i32),
                ("net", _vp), ("head", _vp), ("g_conv1", _vp), ("g_conv2", _vp),
                ("head_offset", _c_i64),
                ("flat_param", _vp), ("flat_grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("n_param", _c_i64),
                ("step2", _vp),
                ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("cache", _vp), ("exchange", _vp), ("exchange_user", _vp), ("step_overrides", _vp), ("last_loss", _vp)]


class Optim(ctypes.Structure):
    """drgnn_optim (include/drgnn.h): Adam's scalars and the options of the ``_opt`` entry points (AdamW, clipping,
    learning-rate table); pointer members are device addresses."""
    _fields_ = [("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("weight_decay", ctypes.c_double), ("max_grad_norm", ctypes.c_double),
                ("lr_table", _vp), ("norm_words", _vp), ("norm_out", _vp),
                ("lr_n", _c_i32), ("decoupled", _c_i32), ("clip", _c_i32), ("norm_cap", _c_i32),
                ("n_dead", _c_i32), ("reserved", _c_i32),
                ("dead_off", _c_i64 * 8), ("dead_len", _c_i64 * 8)]


class IfaceRequest(ctypes.Structure):
    """drgnn_iface_request (include/drgnn.h): one ragged batch of complexes for drgnn_iface_count / drgnn_iface_fill;
    ``host_*`` are addresses of host copies of the three offset tables."""
    _fields_ = [("xyz", _vp), ("atom_ptr", _vp), ("res_ptr", _vp), ("res_split", _vp), ("res_type", _vp),
                ("host_atom_ptr", _vp), ("host_res_ptr", _vp), ("host_res_split", _vp),
                ("n_atoms", _c_i64), ("n_residues", _c_i64), ("n_complexes", _c_i64),
                ("contact_distance", ctypes.c_double), ("internal_contact_distance", ctypes.c_double),
                ("tile_atoms", _c_i32), ("reserved", _c_i32),
                ("workspace", _vp), ("workspace_bytes", _c_i64),
                ("node_ptr", _vp), ("edge_ptr", _vp), ("iedge_ptr", _vp)]


class ScoreRequest(ctypes.Structure):
    """drgnn_score_request (include/drgnn.h): M poses of one topology for drgnn_dock_scores; ``host_*`` are addresses of
    host copies of the index tables (``host_zone_ptr`` exists on the host only)."""
    _fields_ = [("xyz", _vp), ("zone_atom", _vp), ("zone_ref", _vp), ("pair_res", _vp), ("atom_ptr", _vp),
                ("host_zone_atom", _vp), ("host_zone_ptr", _vp), ("host_pair_res", _vp), ("host_atom_ptr", _vp),
                ("n_poses", _c_i64), ("n_atoms", _c_i64), ("n_residues", _c_i64), ("n_pairs", _c_i64),
                ("n_ref_pairs", _c_i64), ("fnat_cutoff", ctypes.c_double),
                ("scores", _vp), ("classes", _vp), ("n_preserved", _vp)]


class LddtRequest(ctypes.Structure):
    """drgnn_lddt_request (include/drgnn.h): M poses of one topology and the reference's matched pairs, as entries grouped
    by owning residue, for drgnn_pose_lddt; ``host_*`` are addresses of host copies of the index tables."""
    _fields_ = [("xyz", _vp), ("entry_ptr", _vp), ("self_atom", _vp), ("other_atom", _vp), ("d_ref", _vp),
                ("host_entry_ptr", _vp), ("host_self_atom", _vp), ("host_other_atom", _vp),
                ("n_poses", _c_i64), ("n_atoms", _c_i64), ("n_residues", _c_i64), ("n_entries", _c_i64),
                ("n_chain_a_atoms", _c_i64), ("thresholds", ctypes.c_double * 8),
                ("n_thresholds", _c_i32), ("poses_per_pass", _c_i32), ("counts", _vp), ("residue_counts", _vp)]


class BsaRequest(ctypes.Structure):
    """drgnn_bsa_request (include/drgnn.h): K target residues of a ragged batch of complexes for drgnn_bsa_residues;
    ``host_*`` are addresses of host copies of the offset and target tables."""
    _fields_ = [("xyz", _vp), ("atom_ptr", _vp), ("res_ptr", _vp), ("res_split", _vp), ("rad_complex", _vp),
                ("rad_unbound", _vp), ("target_res", _vp), ("target_complex", _vp),
                ("host_atom_ptr", _vp), ("host_res_ptr", _vp), ("host_res_split", _vp), ("host_target_res", _vp),
                ("host_target_complex", _vp),
                ("n_atoms", _c_i64), ("n_residues", _c_i64), ("n_complexes", _c_i64), ("n_targets", _c_i64),
                ("n_radii", _c_i64), ("probe", ctypes.c_double), ("n_slices", _c_i32), ("reserved", _c_i32),
                ("out", _vp), ("status", _vp)]


class HseRequest(ctypes.Structure):
    """drgnn_hse_request (include/drgnn.h): K target residues, in tiles of one complex each, of a ragged batch of
    complexes for drgnn_hse_residues; ``host_*`` are addresses of host copies of the offset, target, tile and bb tables."""
    _fields_ = [("xyz", _vp), ("atom_ptr", _vp), ("res_ptr", _vp), ("bb", _vp), ("target_res", _vp), ("target_complex", _vp),
                ("tile_ptr", _vp),
                ("host_atom_ptr", _vp), ("host_res_ptr", _vp), ("host_bb", _vp), ("host_target_res", _vp),
                ("host_target_complex", _vp), ("host_tile_ptr", _vp),
                ("n_atoms", _c_i64), ("n_residues", _c_i64), ("n_complexes", _c_i64), ("n_targets", _c_i64),
                ("n_tiles", _c_i64), ("n_rows", _c_i64), ("radius", ctypes.c_double), ("connect_cutoff", ctypes.c_double),
                ("offset", _c_i32), ("connect_a", _c_i32), ("connect_b", _c_i32), ("direction", _c_i32),
                ("out", _vp), ("status", _vp)]


class PackRequest(ctypes.Structure):
    """drgnn_pack_request (include/drgnn.h): the outputs of drgnn_iface_fill (and bsa / hse / depth rows of exactly its nodes) for
    drgnn_iface_pack; ``host_cols`` is the address of a host copy of the column descriptor."""
    _fields_ = [("node_ptr", _vp), ("edge_ptr", _vp), ("iedge_ptr", _vp), ("node_residue", _vp), ("chain", _vp), ("type", _vp),
                ("pos", _vp), ("edge_index", _vp), ("dist", _vp), ("internal_edge_index", _vp), ("bsa", _vp), ("hse", _vp),
                ("res_feat", _vp), ("type_table", _vp), ("cols", _vp), ("host_cols", _vp),
                ("n_complexes", _c_i64), ("n_nodes", _c_i64), ("n_edges", _c_i64), ("n_iedges", _c_i64),
                ("n_residues", _c_i64), ("n_rows", _c_i64),
                ("res_width", _c_i32), ("type_width", _c_i32), ("n_cols", _c_i32), ("edge_mode", _c_i32),
                ("x", _vp), ("edge_index_out", _vp), ("edge_attr", _vp), ("internal_edge_index_out", _vp), ("batch", _vp),
                ("depth", _vp)]         # (the last field, as in the header: the fields before it keep their offsets)


PACK_TYPE, PACK_POS, PACK_CHAIN, PACK_BSA, PACK_HSE, PACK_RES, PACK_DEPTH = range(7)   # sources of drgnn_pack_request.cols


class PoseContactsRequest(ctypes.Structure):
    """drgnn_pose_contacts_request (include/drgnn.h): M coordinate sets of the counted atoms of one two-chain topology;
    ``host_atom_ptr`` is the address of a host copy of the offset table."""
    _fields_ = [("xyz", _vp), ("atom_ptr", _vp), ("host_atom_ptr", _vp),
                ("n_poses", _c_i64), ("n_atoms", _c_i64), ("n_residues", _c_i64), ("n_chain_a", _c_i64),
                ("cutoff", ctypes.c_double), ("bits", _vp), ("n_contacts", _vp)]


class PoseCommonRequest(ctypes.Structure):
    """drgnn_pose_common_request (include/drgnn.h): two sets of contact bit rows of ``n_words`` words each."""
    _fields_ = [("bits_a", _vp), ("bits_b", _vp), ("n_a", _c_i64), ("n_b", _c_i64), ("n_words", _c_i64), ("common", _vp)]


class PoseClusterRequest(ctypes.Structure):
    """drgnn_pose_cluster_request (include/drgnn.h): the common-contact matrix and the contact counts of M poses."""
    _fields_ = [("common", _vp), ("n_contacts", _vp), ("n_poses", _c_i64),
                ("cutoff_fcc", ctypes.c_double), ("cutoff_reverse", ctypes.c_double), ("min_size", _c_i32),
                ("neighbours", _vp), ("transposed", _vp), ("labels", _vp), ("centres", _vp), ("sizes", _vp),
                ("n_clusters", _vp)]


class ContactCountsRequest(ctypes.Structure):
    """drgnn_contact_counts_request (include/drgnn.h): contact bit rows of M poses and a grouping of them as lists;
    ``host_*`` are addresses of host copies of the lists."""
    _fields_ = [("bits", _vp), ("order", _vp), ("group_ptr", _vp), ("host_order", _vp), ("host_group_ptr", _vp),
                ("n_poses", _c_i64), ("n_chain_a", _c_i64), ("n_chain_b", _c_i64), ("n_groups", _c_i64), ("n_listed", _c_i64),
                ("counts", _vp), ("residues", _vp)]


class ConsensusNumeratorsRequest(ctypes.Structure):
    """drgnn_consensus_numerators_request (include/drgnn.h): contact bit rows of poses, the counts of G groups and the
    row of counts every pose is scored against; ``host_row`` is the address of a host copy of ``row``."""
    _fields_ = [("bits", _vp), ("counts", _vp), ("row", _vp), ("host_row", _vp),
                ("n_poses", _c_i64), ("n_chain_a", _c_i64), ("n_chain_b", _c_i64), ("n_groups", _c_i64), ("numerators", _vp)]


class ConsensusBitsRequest(ctypes.Structure):
    """drgnn_consensus_bits_request (include/drgnn.h): the counts of G groups and a threshold each;
    ``host_min_count`` is the address of a host copy of ``min_count``."""
    _fields_ = [("counts", _vp), ("min_count", _vp), ("host_min_count", _vp),
                ("n_chain_a", _c_i64), ("n_chain_b", _c_i64), ("n_groups", _c_i64), ("bits", _vp), ("n_contacts", _vp)]


class PoseRmsdRequest(ctypes.Structure):
    """drgnn_pose_rmsd_request (include/drgnn.h): two pose batches of one topology and the fit / rms atom lists;
    ``host_*`` are addresses of host copies of the lists."""
    _fields_ = [("xyz_a", _vp), ("xyz_b", _vp), ("fit_idx", _vp), ("rms_idx", _vp), ("host_fit_idx", _vp), ("host_rms_idx", _vp),
                ("n_a", _c_i64), ("n_b", _c_i64), ("n_atoms", _c_i64), ("n_fit", _c_i64), ("n_rms", _c_i64),
                ("phases", _c_i32), ("reserved", _c_i32), ("workspace", _vp), ("workspace_bytes", _c_i64), ("d", _vp)]


class PoseClusterDistRequest(ctypes.Structure):
    """drgnn_pose_cluster_dist_request (include/drgnn.h): a distance matrix of M poses and the outputs of drgnn_pose_cluster."""
    _fields_ = [("d", _vp), ("n_poses", _c_i64), ("cutoff", ctypes.c_double), ("min_size", _c_i32), ("reserved", _c_i32),
                ("neighbours", _vp), ("transposed", _vp), ("labels", _vp), ("centres", _vp), ("sizes", _vp),
                ("n_clusters", _vp)]


class DepthRequest(ctypes.Structure):
    """drgnn_depth_request (include/drgnn.h): K target residues of a ragged batch of complexes for drgnn_depth_residues;
    ``host_*`` are addresses of host copies of the offset and target tables."""
    _fields_ = [("xyz", _vp), ("atom_ptr", _vp), ("res_ptr", _vp), ("radii", _vp), ("dots", _vp), ("target_res", _vp),
                ("target_complex", _vp),
                ("host_atom_ptr", _vp), ("host_res_ptr", _vp), ("host_target_res", _vp), ("host_target_complex", _vp),
                ("n_atoms", _c_i64), ("n_residues", _c_i64), ("n_complexes", _c_i64), ("n_targets", _c_i64),
                ("n_radii", _c_i64), ("probe", ctypes.c_double), ("link", ctypes.c_double),
                ("n_dots", _c_i32), ("components", _c_i32), ("phases", _c_i32), ("reserved", _c_i32), ("workspace", _vp), ("workspace_bytes", _c_i64),
                ("out", _vp), ("status", _vp)]


# the entry points int f(const request*, hipStream_t): (method of Api, C symbol, record).  The table gives each its
# argtypes and Api a method (self, request, stream) that raises DrgnnError on a non-zero return
REQUEST_CALLS = (
    ("iface_count", "drgnn_iface_count", IfaceRequest), ("dock_scores", "drgnn_dock_scores", ScoreRequest),
    ("bsa_residues", "drgnn_bsa_residues", BsaRequest), ("hse_residues", "drgnn_hse_residues", HseRequest),
    ("depth_residues", "drgnn_depth_residues", DepthRequest), ("iface_pack", "drgnn_iface_pack", PackRequest),
    ("pose_contacts", "drgnn_pose_contacts", PoseContactsRequest), ("pose_common", "drgnn_pose_common", PoseCommonRequest),
    ("pose_cluster", "drgnn_pose_cluster", PoseClusterRequest),
    ("pose_contact_counts", "drgnn_pose_contact_counts", ContactCountsRequest),
    ("pose_consensus_numerators", "drgnn_pose_consensus_numerators", ConsensusNumeratorsRequest),
    ("pose_consensus_bits", "drgnn_pose_consensus_bits", ConsensusBitsRequest),
    ("pose_rmsd", "drgnn_pose_rmsd", PoseRmsdRequest), ("pose_cluster_dist", "drgnn_pose_cluster_dist", PoseClusterDistRequest))
# the entry points of the same form added since (the length of REQUEST_CALLS is pinned by tests/test_interface_split.py):
# bound and given to Api by the same two loops
REQUEST_CALLS_2 = (("pose_lddt", "drgnn_pose_lddt", LddtRequest),)
# the limit queries int32 drgnn_<name>(int32 what): Api gets a method <name>(self, what) for each
CAPACITY_CALLS = ("bsa_capacity", "hse_capacity", "depth_capacity", "pack_capacity", "fcc_capacity", "consensus_capacity",
                  "rmsd_capacity")

EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p)


class StepPlan(ctypes.Structure):
    """drgnn_step_plan (include/drgnn.h): the launch (in), the overrides (in), the layout (out)."""
    _fields_ = [("kind", _c_i32), ("n_feat", _c_i32), ("max_nodes", _c_i32), ("max_edges", _c_i32), ("max_c0", _c_i32),
                ("R", _c_i32), ("H", _c_i32), ("O", _c_i32),
                ("n_graphs", _c_i64), ("co_built_graphs", _c_i64),
                ("train", _c_i32), ("topo_flags", _c_i32),
                ("force_wgs", _c_i32), ("no_class", _c_i32), ("no_aggregate", _c_i32), ("no_split", _c_i32),
                ("no_paired", _c_i32),
                ("family", _c_i32), ("wgs_per_graph", _c_i32), ("slabs_per_graph", _c_i32), ("width", _c_i32),
                ("cls", _c_i32), ("lean_ok", _c_i32), ("builder_wgs_per_graph", _c_i32),
                ("lds_bytes", _c_i64), ("xchg_words", _c_i64),
                ("from_memory", _c_i32), ("reserved", _c_i32)]

    OVERRIDES = ("force_wgs", "no_class", "no_aggregate", "no_split", "no_paired")


STEP_FAMILY_NONE, STEP_FAMILY_PRODUCT, STEP_FAMILY_AGGREGATE = 0, 1, 2


def _plan_inputs(kind, n_feat, max_nodes, max_edges, max_c0, R, H, O, n_graphs, topo_flags):
    """a StepPlan with the input members every plan query sets (an inference launch that co-builds nothing, no overrides)"""
    p = StepPlan()
    p.kind, p.n_feat, p.max_nodes, p.max_edges, p.max_c0 = int(kind), int(n_feat), int(max_nodes), int(max_edges), int(max_c0)
    p.R, p.H, p.O, p.n_graphs, p.topo_flags = int(R), int(H), int(O), int(n_graphs), int(topo_flags)
    return p


class StepHints(ctypes.Structure):
    """drgnn_step_hints: host-side offset tables of a launch's graphs (pointers to HOST memory), what the workspace holds,
    the plan the caller sized its buffers from."""
    _fields_ = [("host_node_ptr", _vp), ("host_edge_ptr", _vp), ("set_node_ptr", _vp), ("set_edge_ptr", _vp),
                ("host_ids", _vp), ("topo_flags", _c_i32), ("reserved", _c_i32), ("tiles", _vp), ("plan", _vp),
                ("next_ids", _vp), ("n_next", _c_i64)]


class TopologyCacheDesc(ctypes.Structure):
    """drgnn_topology_cache: one topology workspace over a whole resident set + its node features / targets."""
    _fields_ = [("n_graphs", _c_i64), ("n_nodes", _c_i64), ("n_edges", _c_i64),
                ("ws_i32", _vp), ("ws_f32", _vp), ("x", _vp), ("y", _vp), ("y_bytes", _c_i32), ("flags", _c_i32),
                ("tiles", _vp)]


class HeadDesc(ctypes.Structure):
    _fields_ = [("R", _c_i32), ("H", _c_i32), ("O", _c_i32), ("task", _c_i32), ("train", _c_i32),
                ("p_drop", ctypes.c_float), ("seed", ctypes.c_uint32), ("transform_sigmoid", _c_i32),
                ("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp), ("class_w", _vp), ("drop_mask", _vp)]


TASK_REG, TASK_CLASS, TASK_GRAD = 0, 1, 2      # (TASK_GRAD: `target` = d loss / d pred, the autograd boundary)
ZERO_RANGES = 8


def _ptr(t):
    return None if t is None else t.data_ptr()


class DrgnnError(RuntimeError):
    pass


def _check(rc, what):
    if rc != 0:
        kind = {-1: "bad argument", -2: "workspace/capacity", -3: "unsupported width"}.get(
            rc, "hipError_t %d" % rc if rc > 0 else "error %d" % rc)
        raise DrgnnError("%s failed: %s" % (what, kind))


class Api(object):
    """Typed wrapper around one loaded libdrgnn*.so."""

    def __init__(self, path):
        self.path = path
        lib = ctypes.CDLL(path)
        self.lib = lib
        lib.drgnn_abi_version.restype = ctypes.c_int
        lib.drgnn_topology_layout.argtypes = [_c_i64, _c_i64, _c_i64, ctypes.POINTER(_c_i64),
                                              ctypes.POINTER(_c_i64)]
        lib.drgnn_topology_scratch_elems.argtypes = [_c_i64] * 3
        lib.drgnn_topology_scratch_elems.restype = _c_i64
        lib.drgnn_topology_lds_bytes.argtypes = [_c_i32, _c_i32]
        lib.drgnn_topology_lds_bytes.restype = _c_i64
        lib.drgnn_topology_build.argtypes = [_vp] * 8 + [_c_i64] * 4 + [_c_i32] * 2 + [_vp] * 4
        lib.drgnn_topology_finalize.argtypes = [_vp, _c_i64, _c_i64, _c_i64, _vp]
        lib.drgnn_topology_status.argtypes = [_vp, _c_i64, _c_i64, _c_i64, ctypes.POINTER(_c_i32), _vp]
        lib.drgnn_net_lds_bytes.argtypes = [_c_i32] * 6
        lib.drgnn_net_lds_bytes.restype = _c_i64
        lib.drgnn_net_partial_elems.argtypes = [_c_i32, _c_i32]
        lib.drgnn_net_partial_elems.restype = _c_i64
        lib.drgnn_net_scratch_elems.argtypes = [_c_i32, _c_i32, _c_i64, _c_i64, _c_i64]
        lib.drgnn_net_scratch_elems.restype = _c_i64
        lib.drgnn_net_forward.argtypes = ([ctypes.POINTER(NetDesc)] + [_vp] * 3 + [_c_i64] * 3 +
                                          [_c_i32] * 3 + [_vp] * 7)
        lib.drgnn_net_backward_fused_head.argtypes = ([ctypes.POINTER(NetDesc), ctypes.POINTER(HeadDesc)] +
                                                      [_vp] * 6 + [_c_i64] * 3 + [_c_i32] * 3 + [_vp] * 8 +
                                                      [ctypes.POINTER(TopologyRequest), _vp])
        lib.drgnn_net_backward.argtypes = ([ctypes.POINTER(NetDesc)] + [_vp] * 4 + [_c_i64] * 3 +
                                           [_c_i32] * 3 + [_vp] * 3 + [_vp] * 5)
        lib.drgnn_train_update.argtypes = ([ctypes.POINTER(NetDesc), _vp, _c_i64] +
                                           [ctypes.POINTER(ConvGrads)] * 2 + [_vp, _c_i64] + [_c_i32] * 3 +
                                           [_c_i64] + [_vp] * 4 + [_c_i64] + [_vp] * 2 +
                                           [ctypes.c_double] * 4 + [_c_i32, _vp])
        lib.drgnn_net_step_lds_bytes.argtypes = [_c_i32] * 8
        lib.drgnn_net_step_lds_bytes.restype = _c_i64
        lib.drgnn_net_step_variant.argtypes = [_c_i32, _vp] + [_c_i32] * 6
        lib.drgnn_net_step_variant.restype = _c_i32
        lib.drgnn_net_step_plan.argtypes = [ctypes.POINTER(StepPlan)]
        lib.drgnn_net_step_plan.restype = _c_i32
        lib.drgnn_head_compact_elems.argtypes = [_c_i32] * 3
        lib.drgnn_head_compact_elems.restype = _c_i64
        lib.drgnn_net_train_step.argtypes = ([ctypes.POINTER(NetDesc), ctypes.POINTER(HeadDesc)] + [_vp] * 5 +
                                             [_c_i64] * 3 + [_c_i32] * 3 + [_vp] * 5 +
                                             [ctypes.POINTER(TopologyRequest), ctypes.POINTER(StepHints), _vp])
        lib.drgnn_net_train_step_cached.argtypes = ([ctypes.POINTER(NetDesc), ctypes.POINTER(HeadDesc),
                                                     ctypes.POINTER(TopologyCacheDesc), _vp, _c_i64] + [_c_i32] * 3 +
                                                    [_vp] * 6 + [ctypes.POINTER(StepHints), _vp])
        lib.drgnn_ens_step_plan.argtypes = [ctypes.POINTER(StepPlan), _c_i32]
        lib.drgnn_ens_step_plan.restype = _c_i32
        lib.drgnn_ens_predict_cached.argtypes = ([ctypes.POINTER(NetDesc), ctypes.POINTER(HeadDesc), _vp, _c_i32,
                                                  ctypes.POINTER(TopologyCacheDesc), _vp, _c_i64] + [_c_i32] * 3 +
                                                 [_vp] * 3 + [ctypes.POINTER(StepHints), _vp])
        lib.drgnn_cohort_step_plan.argtypes = [ctypes.POINTER(StepPlan), _c_i32]
        lib.drgnn_cohort_step_plan.restype = _c_i32
        lib.drgnn_cohort_train_step_cached.argtypes = ([ctypes.POINTER(NetDesc), ctypes.POINTER(HeadDesc), _vp, _c_i32,
                                                        ctypes.POINTER(TopologyCacheDesc), _vp, _vp, _c_i64, _c_i64] +
                                                       [_c_i32] * 3 + [ctypes.POINTER(StepHints), _vp])
        lib.drgnn_cohort_update.argtypes = ([ctypes.POINTER(NetDesc), _vp, _c_i32, _vp] + [ctypes.POINTER(ConvGrads)] * 2 +
                                            [_c_i32] * 3 + [_c_i64, _c_i64, _vp, _c_i32, _vp])
        lib.drgnn_step_update.argtypes = ([ctypes.POINTER(NetDesc), _vp, _c_i64] +
                                          [ctypes.POINTER(ConvGrads)] * 2 + [_vp, _vp] + [_c_i32] * 3 +
                                          [_c_i64] + [_vp] * 4 + [_c_i64] + [_vp] * 2 +
                                          [ctypes.c_double] * 4 + [_c_i32, _c_i32, _vp])
        lib.drgnn_net_step_xchg_elems.argtypes = [_c_i32] * 4
        lib.drgnn_net_step_xchg_elems.restype = _c_i64
        lib.drgnn_net_reduce_grads.argtypes = ([ctypes.POINTER(NetDesc), _vp, _c_i64, _c_i64] +
                                               [ctypes.POINTER(ConvGrads)] * 2 + [_vp] * 2)
        lib.drgnn_conv_layer_slabs.argtypes = [_c_i64]
        lib.drgnn_conv_layer_slabs.restype = _c_i64
        lib.drgnn_conv_layer_partial_elems.argtypes = [_c_i32] * 3
        lib.drgnn_conv_layer_partial_elems.restype = _c_i64
        lib.drgnn_conv_layer_forward.argtypes = ([_c_i32, _vp, _c_i64, _c_i32, _c_i32, ctypes.POINTER(ConvParams)] +
                                                 [_vp] * 2 + [_c_i64] + [_vp] * 3)
        lib.drgnn_conv_layer_backward.argtypes = ([_c_i32, _vp, _c_i64, _c_i32, _c_i32, ctypes.POINTER(ConvParams)] +
                                                  [_vp] * 2 + [_c_i64] + [_vp] * 3 +
                                                  [ctypes.POINTER(ConvGrads)] + [_vp] * 2)
        lib.drgnn_segpool_forward.argtypes = [_vp, _c_i64, _c_i64, _c_i64, _vp, _c_i32, _c_i32, _vp, _vp, _vp]
        lib.drgnn_segmax_backward.argtypes = [_vp, _vp, _c_i64, _c_i32, _c_i64, _vp, _vp]
        lib.drgnn_pooled_edges_export.argtypes = [_vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp]
        lib.drgnn_cluster_offset.argtypes = [_vp, _vp, _c_i64, _vp, _vp]
        lib.drgnn_graclus.argtypes = [_vp, _c_i64, _c_i64, _c_i64, _c_i32, _c_i32, _vp, _vp, _vp, _vp]
        lib.drgnn_mcl.argtypes = [_vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp]
        lib.drgnn_louvain.argtypes = [_vp, _c_i64, _vp, _vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _vp, _vp]
        lib.drgnn_metrics_workspace_bytes.argtypes = [_c_i64]
        lib.drgnn_metrics_workspace_bytes.restype = _c_i64
        lib.drgnn_metrics.argtypes = [_vp, _vp, _c_i64, _c_i32, _c_i32, ctypes.c_double, _c_i32, _c_i32, _vp, _c_i64,
                                      _vp, _vp, _vp, _vp, _vp]
        lib.drgnn_p2p_bytes.argtypes = [_c_i64]
        lib.drgnn_p2p_bytes.restype = _c_i64
        lib.drgnn_p2p_alloc.argtypes = [_c_i64, ctypes.POINTER(_vp), _vp]
        lib.drgnn_p2p_open.argtypes = [_vp, ctypes.POINTER(_vp)]
        lib.drgnn_p2p_close.argtypes = [_vp]
        lib.drgnn_p2p_free.argtypes = [_vp]
        lib.drgnn_allreduce_oneshot.argtypes = [_vp, _c_i64, ctypes.POINTER(_vp), _c_i32, _c_i32, ctypes.c_float, _vp, _vp,
                                                _c_i32, _vp]
        lib.drgnn_train_epoch_scratch_bytes.argtypes = [ctypes.POINTER(EpochPlan)]
        lib.drgnn_train_epoch_scratch_bytes.restype = _c_i64
        lib.drgnn_train_epoch.argtypes = [ctypes.POINTER(EpochPlan), _vp, _c_i64, _vp, _vp, _vp]
        lib.drgnn_topology_build_request.argtypes = [ctypes.POINTER(TopologyRequest), _vp]
        lib.drgnn_topology_tiles.argtypes = [_vp, _vp, _c_i64, _c_i64, _c_i64, _vp, _c_i32, _c_i32, _vp, _vp]
        lib.drgnn_topology_tiles_elems.restype = _c_i64
        lib.drgnn_topology_tiles_elems.argtypes = [_c_i64, _c_i32]
        lib.drgnn_topology_tiles_ok.restype = _c_i32
        lib.drgnn_topology_tiles_ok.argtypes = [_c_i32, _c_i32, _c_i32]
        lib.drgnn_batch_offsets.argtypes = [ctypes.POINTER(GraphSet), _vp, _c_i64, _c_i32, _vp, _vp]
        lib.drgnn_collate.argtypes = [ctypes.POINTER(GraphSet), _vp] + [_c_i64] * 3 + [_vp] * 11
        lib.drgnn_head_partial_elems.argtypes = [_c_i32] * 3
        lib.drgnn_head_partial_elems.restype = _c_i64
        lib.drgnn_head_num_slabs.argtypes = [_c_i64]
        lib.drgnn_head_num_slabs.restype = _c_i64
        lib.drgnn_head_pass_units.argtypes = [_c_i32] * 3 + [_c_i64]
        lib.drgnn_head_pass_units.restype = _c_i32
        lib.drgnn_net_head_stage_bytes.argtypes = [_c_i32] * 3
        lib.drgnn_net_head_stage_bytes.restype = _c_i64
        lib.drgnn_head_step.argtypes = [ctypes.POINTER(HeadDesc), _vp, _vp, _c_i64] + [_vp] * 5
        lib.drgnn_head_reduce.argtypes = [_vp, _c_i64, _c_i32, _c_i32, _c_i32] + [_vp] * 4
        lib.drgnn_adam_step.argtypes = [_vp] * 5 + [_c_i64] + [ctypes.c_double] * 5 + [_vp]
        lib.drgnn_step_gradients.argtypes = ([ctypes.POINTER(NetDesc), _vp, _c_i64] + [ctypes.POINTER(ConvGrads)] * 2 +
                                             [_vp, _vp] + [_c_i32] * 3 + [_vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_c_i64), _c_i32,
                                                                       _vp, _c_i32, _vp])
        lib.drgnn_optim_norm_words.argtypes = [_c_i64]
        lib.drgnn_optim_norm_words.restype = _c_i64
        lib.drgnn_adam_step_opt.argtypes = [_vp] * 5 + [_c_i64, ctypes.POINTER(Optim), _vp]
        lib.drgnn_train_update_opt.argtypes = ([ctypes.POINTER(NetDesc), _vp, _c_i64] +
                                               [ctypes.POINTER(ConvGrads)] * 2 + [_vp, _c_i64] + [_c_i32] * 3 +
                                               [_c_i64] + [_vp] * 4 + [_c_i64] + [_vp] * 2 +
                                               [ctypes.POINTER(Optim), _c_i32, _vp])
        lib.drgnn_step_update_opt.argtypes = ([ctypes.POINTER(NetDesc), _vp, _c_i64] +
                                              [ctypes.POINTER(ConvGrads)] * 2 + [_vp, _vp] + [_c_i32] * 3 +
                                              [_c_i64] + [_vp] * 4 + [_c_i64] + [_vp] * 2 +
                                              [ctypes.POINTER(Optim), _c_i32, _c_i32, _vp])
        lib.drgnn_cohort_update_opt.argtypes = ([ctypes.POINTER(NetDesc), _vp, _vp, _c_i32, _vp] + [ctypes.POINTER(ConvGrads)] * 2 +
                                                [_c_i32] * 3 + [_c_i64, _c_i64, _vp, _c_i32, _c_i32, _vp])
        lib.drgnn_train_epoch_opt.argtypes = [ctypes.POINTER(EpochPlan), ctypes.POINTER(Optim), _vp, _c_i64, _vp, _vp, _vp]
        lib.drgnn_iface_workspace_bytes.argtypes = [_c_i64] * 4
        lib.drgnn_iface_workspace_bytes.restype = _c_i64
        lib.drgnn_iface_fill.argtypes = [ctypes.POINTER(IfaceRequest)] + [_c_i64] * 3 + [_vp] * 9
        lib.drgnn_depth_workspace.argtypes = [_c_i64, _c_i64, _c_i32, ctypes.POINTER(_c_i64)]
        lib.drgnn_depth_workspace.restype = _c_i64
        lib.drgnn_rmsd_workspace.argtypes = [_c_i64] * 4 + [ctypes.POINTER(_c_i64)]
        lib.drgnn_rmsd_workspace.restype = _c_i64
        for _, symbol, record in REQUEST_CALLS + REQUEST_CALLS_2:
            getattr(lib, symbol).argtypes = [ctypes.POINTER(record), _vp]
        for name in CAPACITY_CALLS:
            getattr(lib, "drgnn_" + name).argtypes, getattr(lib, "drgnn_" + name).restype = [_c_i32], _c_i32
        if lib.drgnn_abi_version() != 5:
            raise DrgnnError("ABI mismatch in %s" % path)

    # -- topology ---------------------------------------------------------------
    def topology_layout(self, n_nodes, n_edges, n_graphs):
        oi = (_c_i64 * (TI_COUNT + 1))()
        of = (_c_i64 * (TF_COUNT + 1))()
        _check(self.lib.drgnn_topology_layout(n_nodes, n_edges, n_graphs, oi, of), "drgnn_topology_layout")
        return list(oi), list(of)

    def topology_scratch_elems(self, n_nodes, n_edges, n_graphs):
        return int(self.lib.drgnn_topology_scratch_elems(n_nodes, n_edges, n_graphs))

    def topology_lds_bytes(self, max_nodes, max_edges):
        return int(self.lib.drgnn_topology_lds_bytes(max_nodes, max_edges))

    def topology_build(self, edge_index, edge_attr, batch, cluster0, cluster1, node_ptr, edge_ptr,
                       c1_ptr, n_nodes, n_edges, len_c1, n_graphs, max_nodes, max_edges, ws_i32,
                       ws_f32, scratch, stream):
        _check(self.lib.drgnn_topology_build(
            _ptr(edge_index), _ptr(edge_attr), _ptr(batch), _ptr(cluster0), _ptr(cluster1),
            _ptr(node_ptr), _ptr(edge_ptr), _ptr(c1_ptr), n_nodes, n_edges, len_c1, n_graphs,
            max_nodes, max_edges, _ptr(ws_i32), _ptr(ws_f32), _ptr(scratch), stream),
            "drgnn_topology_build")

    def topology_finalize(self, ws_i32, n_nodes, n_edges, n_graphs, stream):
        _check(self.lib.drgnn_topology_finalize(_ptr(ws_i32), n_nodes, n_edges, n_graphs, stream),
               "drgnn_topology_finalize")

    def topology_status(self, ws_i32, n_nodes, n_edges, n_graphs, stream):
        st = (_c_i32 * 4)()
        _check(self.lib.drgnn_topology_status(_ptr(ws_i32), n_nodes, n_edges, n_graphs, st, stream),
               "drgnn_topology_status")
        return list(st)

    # -- fused net --------------------------------------------------------------
    def net_lds_bytes(self, kind, n_feat, max_nodes, max_edges, max_c0, backward):
        return int(self.lib.drgnn_net_lds_bytes(kind, n_feat, max_nodes, max_edges, max_c0, int(backward)))

    def net_partial_elems(self, kind, n_feat):
        return int(self.lib.drgnn_net_partial_elems(kind, n_feat))

    def net_scratch_elems(self, kind, n_feat, n_nodes, n_edges, n_graphs):
        return int(self.lib.drgnn_net_scratch_elems(kind, n_feat, n_nodes, n_edges, n_graphs))

    def net_forward(self, desc, x, ws_i32, ws_f32, n_nodes, n_edges, n_graphs, max_nodes, max_edges,
                    max_c0, xp, arg0, arg1, readout, scratch, stream, step_inc=None):
        _check(self.lib.drgnn_net_forward(
            ctypes.byref(desc), _ptr(x), _ptr(ws_i32), _ptr(ws_f32), n_nodes, n_edges, n_graphs,
            max_nodes, max_edges, max_c0, _ptr(xp), _ptr(arg0), _ptr(arg1), _ptr(readout), _ptr(scratch),
            _ptr(step_inc), stream), "drgnn_net_forward")

    def net_backward_fused_head(self, desc, head, x, readout, target, step, ws_i32, ws_f32, n_nodes, n_edges,
                                n_graphs, max_nodes, max_edges, max_c0, xp, arg0, arg1, pred, head_partials,
                                grad_x, partials, scratch, stream, next_topology=None):
        _check(self.lib.drgnn_net_backward_fused_head(
            ctypes.byref(desc), ctypes.byref(head), _ptr(x), _ptr(readout), _ptr(target), _ptr(step),
            _ptr(ws_i32), _ptr(ws_f32), n_nodes, n_edges, n_graphs, max_nodes, max_edges, max_c0, _ptr(xp),
            _ptr(arg0), _ptr(arg1), _ptr(pred), _ptr(head_partials), _ptr(grad_x), _ptr(partials),
            _ptr(scratch), None if next_topology is None else ctypes.byref(next_topology), stream),
            "drgnn_net_backward_fused_head")

    def net_backward(self, desc, x, grad_readout, ws_i32, ws_f32, n_nodes, n_edges, n_graphs,
                     max_nodes, max_edges, max_c0, xp, arg0, arg1, grad_x, partials, scratch, stream,
                     step_inc=None):
        _check(self.lib.drgnn_net_backward(
            ctypes.byref(desc), _ptr(x), _ptr(grad_readout), _ptr(ws_i32), _ptr(ws_f32), n_nodes,
            n_edges, n_graphs, max_nodes, max_edges, max_c0, _ptr(xp), _ptr(arg0), _ptr(arg1),
            _ptr(grad_x), _ptr(partials), _ptr(scratch), _ptr(step_inc), stream), "drgnn_net_backward")

    def train_update(self, desc, conv_partials, n_graphs, g1, g2, head_partials, R, H, O, head_offset,
                     flat_p, flat_g, exp_avg, exp_avg_sq, step, loss, lr, beta1, beta2, eps, stream,
                     apply_adam=True, optim=None):
        """``optim`` (an Optim record): drgnn_train_update_opt, Adam's scalars and the options from the record"""
        args = (ctypes.byref(desc), _ptr(conv_partials), n_graphs, g1, g2, _ptr(head_partials), head_partials.size(0), R, H, O,
                head_offset, _ptr(flat_p), _ptr(flat_g), _ptr(exp_avg), _ptr(exp_avg_sq), flat_p.numel(), _ptr(step), _ptr(loss))
        if optim is None:
            _check(self.lib.drgnn_train_update(*(args + (lr, beta1, beta2, eps, 1 if apply_adam else 0, stream))),
                   "drgnn_train_update")
        else:
            _check(self.lib.drgnn_train_update_opt(*(args + (ctypes.byref(optim), 1 if apply_adam else 0, stream))),
                   "drgnn_train_update_opt")

    # -- fused training step ------------------------------------------------------
    def step_plan(self, kind, n_feat, max_nodes, max_edges, max_c0, R, H, O, n_graphs, co_built_graphs=0, train=True,
                  topo_flags=0, overrides=None):
        """The launch plan (StepPlan, ``out`` members filled) of a fused step of ``n_graphs`` graphs with these bounds on a
        workspace built with ``topo_flags``, the same launch building the topology of ``co_built_graphs`` graphs.
        ``overrides``: dict over StepPlan.OVERRIDES (tests, A/B runs).  ``family == 0``: outside the fused kernels."""
        p = _plan_inputs(kind, n_feat, max_nodes, max_edges, max_c0, R, H, O, n_graphs, topo_flags)
        p.co_built_graphs, p.train = int(co_built_graphs), int(bool(train))
        for k, v in (overrides or {}).items():
            if k not in StepPlan.OVERRIDES:
                raise KeyError("unknown step-plan override %r" % (k,))
            setattr(p, k, int(v))
        self.lib.drgnn_net_step_plan(ctypes.byref(p))
        return p

    def net_step_plan(self, kind, n_feat, max_nodes, max_edges, max_c0, R, H, O, n_graphs, co_built_graphs=0, train=True,
                      topo_flags=TOPO_HIER | TOPO_TILES, overrides=None):
        """(workgroups per graph, LDS bytes per workgroup) of ``step_plan`` -- by default for a training launch on a workspace
        with the hierarchical order and aggregation tiles (what the trainers build); (0, 0): outside the fused kernels."""
        p = self.step_plan(kind, n_feat, max_nodes, max_edges, max_c0, R, H, O, n_graphs, co_built_graphs, train, topo_flags,
                           overrides)
        return int(p.wgs_per_graph), int(p.lds_bytes)

    def net_step_lds_bytes(self, kind, n_feat, max_nodes, max_edges, max_c0, R, H, O):
        return int(self.lib.drgnn_net_step_lds_bytes(kind, n_feat, max_nodes, max_edges, max_c0, R, H, O))

    def step_is_specialised(self, kind, x, n_feat, max_nodes, max_edges, max_c0, H, O):
        """Padded feature width of the width-specialised fused step kernel these bounds launch (0: generic)."""
        return int(self.lib.drgnn_net_step_variant(kind, _ptr(x), n_feat, max_nodes, max_edges, max_c0, H, O))

    def head_compact_elems(self, R, H, O):
        return int(self.lib.drgnn_head_compact_elems(R, H, O))

    def net_train_step(self, desc, head, x, target, step2, ws_i32, ws_f32, n_nodes, n_edges, n_graphs,
                       max_nodes, max_edges, max_c0, pred, readout, head_partials, partials, xchg, stream,
                       next_topology=None, hints=None):
        _check(self.lib.drgnn_net_train_step(
            ctypes.byref(desc), ctypes.byref(head), _ptr(x), _ptr(target), _ptr(step2), _ptr(ws_i32),
            _ptr(ws_f32), n_nodes, n_edges, n_graphs, max_nodes, max_edges, max_c0, _ptr(pred), _ptr(readout),
            _ptr(head_partials), _ptr(partials), _ptr(xchg),
            None if next_topology is None else ctypes.byref(next_topology),
            None if hints is None else ctypes.byref(hints), stream), "drgnn_net_train_step")

    def net_train_step_cached(self, desc, head, cache, ids, n_graphs, max_nodes, max_edges, max_c0, step2, pred,
                              readout, head_partials, partials, xchg, stream, hints=None):
        _check(self.lib.drgnn_net_train_step_cached(
            ctypes.byref(desc), ctypes.byref(head), ctypes.byref(cache), _ptr(ids), n_graphs, max_nodes, max_edges,
            max_c0, _ptr(step2), _ptr(pred), _ptr(readout), _ptr(head_partials), _ptr(partials), _ptr(xchg),
            None if hints is None else ctypes.byref(hints), stream),
            "drgnn_net_train_step_cached")


    def ens_step_plan(self, K, kind, n_feat, max_nodes, max_edges, max_c0, R, H, O, n_graphs, topo_flags=0):
        """The plan (StepPlan) of an ensemble launch of K models; ``family == 0``: no fused ensemble launch takes it."""
        p = _plan_inputs(kind, n_feat, max_nodes, max_edges, max_c0, R, H, O, n_graphs, topo_flags)
        self.lib.drgnn_ens_step_plan(ctypes.byref(p), int(K))
        return p

    def ens_predict_cached(self, desc, head, members, K, cache, ids, n_graphs, max_nodes, max_edges, max_c0, step2, pred,
                           readout, stream, hints):
        _check(self.lib.drgnn_ens_predict_cached(
            ctypes.byref(desc), ctypes.byref(head), _ptr(members), int(K), ctypes.byref(cache), _ptr(ids), n_graphs,
            max_nodes, max_edges, max_c0, _ptr(step2), _ptr(pred), _ptr(readout), ctypes.byref(hints), stream),
            "drgnn_ens_predict_cached")

    def cohort_step_plan(self, K, kind, n_feat, max_nodes, max_edges, max_c0, R, H, O, n_graphs, topo_flags=0):
        """The plan (StepPlan) of a cohort's fused step launch of K members; ``family == 0``: the members are stepped one by one."""
        p = _plan_inputs(kind, n_feat, max_nodes, max_edges, max_c0, R, H, O, n_graphs, topo_flags)
        self.lib.drgnn_cohort_step_plan(ctypes.byref(p), int(K))
        return p

    def cohort_train_step_cached(self, desc, head, members, K, cache, ids, counts, ids_stride, n_graphs, max_nodes, max_edges,
                                 max_c0, stream, hints):
        """``ids`` / ``counts``: raw device addresses (this step's rows of the epoch's tables)"""
        _check(self.lib.drgnn_cohort_train_step_cached(
            ctypes.byref(desc), ctypes.byref(head), _ptr(members), int(K), ctypes.byref(cache), ids, counts, int(ids_stride),
            int(n_graphs), max_nodes, max_edges, max_c0, ctypes.byref(hints), stream), "drgnn_cohort_train_step_cached")

    def cohort_update(self, desc, members, K, counts, g1, g2, R, H, O, head_offset, n_param, stream, losses=None, apply_adam=True,
                      optims=None, any_clip=False):
        """``counts`` / ``losses``: raw device addresses (this step's rows of the epoch's tables; ``losses`` may be None);
        ``optims``: the device table of the members' Optim records (drgnn_cohort_update_opt)"""
        head = (ctypes.byref(desc), _ptr(members))
        tail = (int(K), counts, g1, g2, R, H, O, int(head_offset), int(n_param), losses, 1 if apply_adam else 0)
        if optims is None:
            _check(self.lib.drgnn_cohort_update(*(head + tail + (stream,))), "drgnn_cohort_update")
        else:
            _check(self.lib.drgnn_cohort_update_opt(*(head + (_ptr(optims),) + tail + (1 if any_clip else 0, stream))),
                   "drgnn_cohort_update_opt")

    def step_update(self, desc, conv_partials, n_graphs, g1, g2, head_partials, readout, R, H, O, head_offset,
                    flat_p, flat_g, exp_avg, exp_avg_sq, step2, loss, lr, beta1, beta2, eps, stream,
                    apply_adam=True, slabs_per_graph=0, optim=None):
        """``optim`` (an Optim record): drgnn_step_update_opt, Adam's scalars and the options from the record"""
        args = (ctypes.byref(desc), _ptr(conv_partials), n_graphs, g1, g2, _ptr(head_partials), _ptr(readout), R, H, O,
                head_offset, _ptr(flat_p), _ptr(flat_g), _ptr(exp_avg), _ptr(exp_avg_sq), flat_p.numel(), _ptr(step2), _ptr(loss))
        tail = (1 if apply_adam else 0, int(slabs_per_graph), stream)
        if optim is None:
            _check(self.lib.drgnn_step_update(*(args + (lr, beta1, beta2, eps) + tail)), "drgnn_step_update")
        else:
            _check(self.lib.drgnn_step_update_opt(*(args + (ctypes.byref(optim),) + tail)), "drgnn_step_update_opt")

    def step_gradients(self, desc, conv_partials, n_graphs, g1, g2, head_partials, readout, R, H, O, head_grad,
                       graph_weight, zero_ptr, zero_len, n_zero, step2, slabs_per_graph, stream):
        """drgnn_step_gradients: the slabs of a fused step summed into the gradient tensors (each graph's slab times
        ``graph_weight[g]`` when given); ``zero_ptr`` / ``zero_len``: ctypes arrays of the ranges to clear."""
        _check(self.lib.drgnn_step_gradients(
            ctypes.byref(desc), _ptr(conv_partials), n_graphs, g1, g2, _ptr(head_partials), _ptr(readout), R, H, O,
            head_grad, _ptr(graph_weight), zero_ptr, zero_len, int(n_zero), _ptr(step2), int(slabs_per_graph), stream),
            "drgnn_step_gradients")

    def net_step_xchg_elems(self, kind, max_nodes, max_c0, H):
        return int(self.lib.drgnn_net_step_xchg_elems(kind, max_nodes, max_c0, H))

    def net_reduce_grads(self, desc, partials, n_nodes, n_graphs, g1, g2, grad_x, stream):
        _check(self.lib.drgnn_net_reduce_grads(ctypes.byref(desc), _ptr(partials), n_nodes, n_graphs,
                                               g1, g2, _ptr(grad_x), stream), "drgnn_net_reduce_grads")


    # -- stand-alone layers / pooling functions ----------------------------------
    def conv_layer_slabs(self, n_nodes):
        return int(self.lib.drgnn_conv_layer_slabs(n_nodes))

    def conv_layer_partial_elems(self, kind, F, H):
        return int(self.lib.drgnn_conv_layer_partial_elems(kind, F, H))

    def conv_layer_forward(self, kind, x, F, H, cp, ws_i32, ws_f32, n_edges, u, out, stream):
        _check(self.lib.drgnn_conv_layer_forward(kind, _ptr(x), x.size(0), F, H, ctypes.byref(cp), _ptr(ws_i32),
                                                 _ptr(ws_f32), n_edges, _ptr(u), _ptr(out), stream),
               "drgnn_conv_layer_forward")

    def conv_layer_backward(self, kind, x, F, H, cp, ws_i32, ws_f32, n_edges, grad_out, du, partials, cg,
                            grad_x, stream):
        _check(self.lib.drgnn_conv_layer_backward(kind, _ptr(x), x.size(0), F, H, ctypes.byref(cp), _ptr(ws_i32),
                                                  _ptr(ws_f32), n_edges, _ptr(grad_out), _ptr(du),
                                                  _ptr(partials), ctypes.byref(cg), _ptr(grad_x), stream),
               "drgnn_conv_layer_backward")

    def segpool_forward(self, ws_i32, n_nodes, n_edges, n_graphs, x, H, op, out, arg, stream):
        _check(self.lib.drgnn_segpool_forward(_ptr(ws_i32), n_nodes, n_edges, n_graphs, _ptr(x), H, op,
                                              _ptr(out), _ptr(arg), stream), "drgnn_segpool_forward")

    def segmax_backward(self, grad_out, arg, n_clusters, H, n_nodes, grad_x, stream):
        _check(self.lib.drgnn_segmax_backward(_ptr(grad_out), _ptr(arg), n_clusters, H, n_nodes, _ptr(grad_x),
                                              stream), "drgnn_segmax_backward")

    def pooled_edges_export(self, ws_i32, ws_f32, n_nodes, n_edges, n_graphs, e1_total, edge_index, edge_attr,
                            stream):
        _check(self.lib.drgnn_pooled_edges_export(_ptr(ws_i32), _ptr(ws_f32), n_nodes, n_edges, n_graphs,
                                                  e1_total, _ptr(edge_index), _ptr(edge_attr), stream),
               "drgnn_pooled_edges_export")

    def cluster_offset(self, cluster, node_ptr, n_graphs, scratch, stream):
        _check(self.lib.drgnn_cluster_offset(_ptr(cluster), _ptr(node_ptr), n_graphs, _ptr(scratch), stream),
               "drgnn_cluster_offset")

    def graclus(self, ws_i32, n_nodes, n_edges, n_graphs, max_nodes, max_edges, weight, perm, cluster, stream):
        _check(self.lib.drgnn_graclus(_ptr(ws_i32), n_nodes, n_edges, n_graphs, max_nodes, max_edges, _ptr(weight),
                                      _ptr(perm), _ptr(cluster), stream), "drgnn_graclus")

    def mcl(self, edge_index, n_edges, node_ptr, edge_ptr, mat_ptr, n_graphs, mat_scratch, int_scratch, labels,
            info, stream):
        _check(self.lib.drgnn_mcl(_ptr(edge_index), n_edges, _ptr(node_ptr), _ptr(edge_ptr), _ptr(mat_ptr), n_graphs,
                                  _ptr(mat_scratch), _ptr(int_scratch), _ptr(labels), _ptr(info), stream), "drgnn_mcl")

    def louvain(self, edge_index, n_edges, node_ptr, edge_ptr, n_graphs, max_nodes, max_edges, labels, info,
                modularity, stream):
        _check(self.lib.drgnn_louvain(_ptr(edge_index), n_edges, _ptr(node_ptr), _ptr(edge_ptr), n_graphs, max_nodes,
                                      max_edges, _ptr(labels), _ptr(info), _ptr(modularity), stream), "drgnn_louvain")

    def metrics_workspace_bytes(self, n):
        return int(self.lib.drgnn_metrics_workspace_bytes(n))

    def metrics(self, pred, y, n, what, direction, threshold, label_lo, n_labels, workspace, counts, scores, order, hits,
                stream):
        _check(self.lib.drgnn_metrics(_ptr(pred), _ptr(y), n, what, direction, float(threshold), label_lo, n_labels,
                                      _ptr(workspace), workspace.numel() * workspace.element_size(), _ptr(counts),
                                      _ptr(scores), _ptr(order), _ptr(hits), stream), "drgnn_metrics")

    def iface_workspace_bytes(self, n_complexes, max_res_a, max_res_b, n_residues):
        return int(self.lib.drgnn_iface_workspace_bytes(int(n_complexes), int(max_res_a), int(max_res_b), int(n_residues)))

    def rmsd_workspace(self, n_a, n_b, n_fit, n_rms):
        """(bytes, offsets [3]) of drgnn_rmsd_workspace; DrgnnError for counts the call refuses"""
        off = (_c_i64 * 3)()
        n = int(self.lib.drgnn_rmsd_workspace(int(n_a), int(n_b), int(n_fit), int(n_rms), off))
        if n < 0:
            _check(-2, "drgnn_rmsd_workspace")
        return n, list(off)

    def depth_workspace(self, n_atoms, n_complexes, n_dots):
        """(bytes, offsets [10]) of drgnn_depth_workspace; DrgnnError for counts the call refuses"""
        off = (_c_i64 * 10)()
        n = int(self.lib.drgnn_depth_workspace(int(n_atoms), int(n_complexes), int(n_dots), off))
        if n < 0:
            _check(-2, "drgnn_depth_workspace")
        return n, [int(v) for v in off]

    def iface_fill(self, request, n_nodes, n_edges, n_iedges, node_residue, pos, chain, type_, edge_index, dist,
                   internal_edge_index, internal_dist, stream):
        _check(self.lib.drgnn_iface_fill(ctypes.byref(request), int(n_nodes), int(n_edges), int(n_iedges), _ptr(node_residue),
                                         _ptr(pos), _ptr(chain), _ptr(type_), _ptr(edge_index), _ptr(dist),
                                         _ptr(internal_edge_index), _ptr(internal_dist), stream), "drgnn_iface_fill")

    def collate(self, gset, ids, n_graphs, n_nodes, n_edges, x, edge_index, edge_attr, batch, cluster0, cluster1,
                y, node_ptr, edge_ptr, c1_ptr, stream):
        _check(self.lib.drgnn_collate(ctypes.byref(gset), _ptr(ids), n_graphs, n_nodes, n_edges, _ptr(x),
                                      _ptr(edge_index), _ptr(edge_attr), _ptr(batch), _ptr(cluster0),
                                      _ptr(cluster1), _ptr(y), _ptr(node_ptr), _ptr(edge_ptr), _ptr(c1_ptr),
                                      stream), "drgnn_collate")

    def topology_tiles(self, ws_i32, ws_f32, n_nodes, n_edges, n_graphs, x, n_feat, use_weights, tiles, stream):
        """Aggregation tiles of an already built workspace (a second flavour for a shared cached topology)."""
        _check(self.lib.drgnn_topology_tiles(_ptr(ws_i32), _ptr(ws_f32), int(n_nodes), int(n_edges), int(n_graphs), _ptr(x),
                                             int(n_feat), int(bool(use_weights)), _ptr(tiles), stream), "drgnn_topology_tiles")

    def topology_tiles_elems(self, n_nodes, n_feat):
        return int(self.lib.drgnn_topology_tiles_elems(int(n_nodes), int(n_feat)))

    def topology_tiles_ok(self, max_nodes, max_edges, n_feat):
        """True when the builder can form the level-0 aggregation tiles (TOPO_TILES) for graphs of these bounds."""
        return bool(self.lib.drgnn_topology_tiles_ok(int(max_nodes), int(max_edges), int(n_feat)))

    def topology_build_request(self, request, stream):
        _check(self.lib.drgnn_topology_build_request(ctypes.byref(request), stream), "drgnn_topology_build_request")

    def batch_offsets(self, gset, ids, n_ids, batch_size, ptrs, stream):
        _check(self.lib.drgnn_batch_offsets(ctypes.byref(gset), _ptr(ids), n_ids, batch_size, _ptr(ptrs), stream),
               "drgnn_batch_offsets")

    # -- one-shot all-reduce over peer-mapped exchange buffers -------------------------
    def p2p_bytes(self, n_floats):
        return int(self.lib.drgnn_p2p_bytes(n_floats))

    def p2p_alloc(self, nbytes):
        """(device pointer, 64-byte IPC handle) of a zero-filled fine-grained exchange buffer."""
        ptr = _vp()
        handle = ctypes.create_string_buffer(64)
        _check(self.lib.drgnn_p2p_alloc(nbytes, ctypes.byref(ptr), handle), "drgnn_p2p_alloc")
        return ptr.value, handle.raw

    def p2p_open(self, handle):
        ptr = _vp()
        buf = ctypes.create_string_buffer(bytes(handle), 64)
        _check(self.lib.drgnn_p2p_open(buf, ctypes.byref(ptr)), "drgnn_p2p_open")
        return ptr.value

    def p2p_close(self, ptr):
        _check(self.lib.drgnn_p2p_close(ptr), "drgnn_p2p_close")

    def p2p_free(self, ptr):
        _check(self.lib.drgnn_p2p_free(ptr), "drgnn_p2p_free")

    def allreduce_oneshot(self, grad, n, peers, world, rank, weight, seq, status, stream, part=0):
        arr = (_vp * world)(*peers)
        _check(self.lib.drgnn_allreduce_oneshot(_ptr(grad), n, arr, world, rank, float(weight), _ptr(seq), _ptr(status),
                                                part, stream), "drgnn_allreduce_oneshot")

    def train_epoch_scratch_bytes(self, plan):
        """Bytes of device scratch for the plan; None when a graph does not fit the fused kernels."""
        n = int(self.lib.drgnn_train_epoch_scratch_bytes(ctypes.byref(plan)))
        if n == -2:
            return None
        if n < 0:
            _check(n, "drgnn_train_epoch_scratch_bytes")
        return n

    def train_epoch(self, plan, scratch, pred, losses, stream):
        _check(self.lib.drgnn_train_epoch(ctypes.byref(plan), _ptr(scratch), scratch.numel() * scratch.element_size(),
                                          _ptr(pred), _ptr(losses), stream), "drgnn_train_epoch")

    def train_epoch_opt(self, plan, optim, scratch, pred, losses, stream):
        _check(self.lib.drgnn_train_epoch_opt(ctypes.byref(plan), ctypes.byref(optim), _ptr(scratch),
                                              scratch.numel() * scratch.element_size(), _ptr(pred), _ptr(losses), stream),
               "drgnn_train_epoch_opt")

    # -- head / loss / optimiser ------------------------------------------------
    def head_partial_elems(self, R, H, O):
        return int(self.lib.drgnn_head_partial_elems(R, H, O))

    def head_num_slabs(self, n_graphs):
        return int(self.lib.drgnn_head_num_slabs(n_graphs))

    def head_pass_units(self, R, H, O, n_graphs):
        """Hidden units an inference head_step of ``n_graphs`` keeps in LDS at a time (H: the head whole, in one pass)."""
        return int(self.lib.drgnn_head_pass_units(R, H, O, n_graphs))

    def net_head_stage_bytes(self, R, H, O):
        """LDS bytes the backward launch needs on top of net_lds_bytes to keep the head's weights in LDS."""
        return int(self.lib.drgnn_net_head_stage_bytes(R, H, O))

    def head_step(self, desc, readout, target, n_graphs, step, pred, grad_readout, partials, stream):
        _check(self.lib.drgnn_head_step(ctypes.byref(desc), _ptr(readout), _ptr(target), n_graphs,
                                        _ptr(step), _ptr(pred), _ptr(grad_readout), _ptr(partials),
                                        stream), "drgnn_head_step")

    def head_reduce(self, partials, n_graphs, R, H, O, grad_block_ptr, loss, step, stream):
        _check(self.lib.drgnn_head_reduce(_ptr(partials), n_graphs, R, H, O, grad_block_ptr, _ptr(loss),
                                          _ptr(step), stream), "drgnn_head_reduce")

    def adam_step(self, param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay,
                  stream):
        _check(self.lib.drgnn_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
                                        _ptr(step), param.numel(), lr, beta1, beta2, eps, weight_decay,
                                        stream), "drgnn_adam_step")


    def optim_norm_words(self, n_param):
        """doubles of ``Optim.norm_words`` scratch a clipping step over ``n_param`` parameters needs"""
        return int(self.lib.drgnn_optim_norm_words(int(n_param)))

    def adam_step_opt(self, param, grad, exp_avg, exp_avg_sq, step, optim, stream):
        _check(self.lib.drgnn_adam_step_opt(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(step),
                                            param.numel(), ctypes.byref(optim), stream), "drgnn_adam_step_opt")


def _request_call(name, symbol):
    def call(self, request, stream):
        _check(getattr(self.lib, symbol)(ctypes.byref(request), stream), symbol)
    call.__name__ = name
    return call


def _capacity_call(name):
    def call(self, what):
        return int(getattr(self.lib, "drgnn_" + name)(int(what)))
    call.__name__ = name
    return call


for _name, _symbol, _ in REQUEST_CALLS + REQUEST_CALLS_2:
    setattr(Api, _name, _request_call(_name, _symbol))
for _name in CAPACITY_CALLS:
    setattr(Api, _name, _capacity_call(_name))

_API = None


def get():
    """The product library.  Raises if it has not been built: no CPU fallback."""
    global _API
    if _API is None:
        if not os.path.exists(LIB_PATH):
            raise DrgnnError(
                "HIP library %s not found. Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C deeprank-gnn_amd/csrc` (hipcc, gfx950)." % LIB_PATH)
        _API = Api(LIB_PATH)
    return _API


def require_device(*tensors):
    """The kernels run on the GPU only; refuse anything else loudly."""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise DrgnnError("deeprank_gnn_amd kernels need CUDA/HIP tensors (MI355X); got a %s "
                             "tensor. There is no CPU path." % t.device.type)


def current_stream(ref):
    """Raw hipStream_t of torch's current stream on the device of ``ref``."""
    if ref.is_cuda:
        return torch.cuda.current_stream(ref.device).cuda_stream
    return None


def step_hints(node_ptr=None, edge_ptr=None, set_node_ptr=None, set_edge_ptr=None, ids=None, topo_flags=0, tiles=None, plan=None,
               next_ids=None):
    """(StepHints, keep-alive tuple) from numpy arrays: int32 per-mini-batch tables, or int64 set tables + int32 ids;
    ``plan``: the StepPlan the caller sized its buffers from."""
    import numpy as np
    h = StepHints()
    keep = []

    def pin(a, dtype):
        if a is None:
            return None
        a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
        keep.append(a)
        return a.ctypes.data
    h.host_node_ptr, h.host_edge_ptr = pin(node_ptr, np.int32), pin(edge_ptr, np.int32)
    h.set_node_ptr, h.set_edge_ptr, h.host_ids = pin(set_node_ptr, np.int64), pin(set_edge_ptr, np.int64), pin(ids, np.int32)
    h.topo_flags = int(topo_flags)
    h.tiles = _ptr(tiles)
    if tiles is not None:
        keep.append(tiles)
    if plan is not None:
        h.plan = ctypes.addressof(plan)
        keep.append(plan)
    if next_ids is not None and next_ids.numel() > 0:      # (device int32 tensor: the next mini-batch's graph numbers)
        h.next_ids, h.n_next = next_ids.data_ptr(), int(next_ids.numel())
        keep.append(next_ids)
    return h, tuple(keep)
