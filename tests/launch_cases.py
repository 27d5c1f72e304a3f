"""Inputs and checks shared by tests/test_launch_form.py (host emulation) and tests/test_gpu_launch_form.py (the device):
the two things every feature entry point leaves to the launch form of csrc/drgnn_launch.h.

1 A grid without blocks is skipped while the rest of the call runs: requests of 0, 1 or 2 items in which one launch of an
  entry point has nothing to do and the others have.  Every case returns 0 and gives the values in EXPECT, which were
  recorded from the emulation build of the commit before the launch form (whose emulation looped and whose device side
  guarded each launch by hand).  What the other suites already hold is not repeated here: drgnn_pose_consensus_bits without
  chain A (consensus_cases.check_groups), drgnn_iface_count without complexes or contacts (iface_cases.check_empty_complexes),
  the calls without targets or poses (the check_empty_* of every *_cases.py).  The stand-alone layers refuse a request
  without nodes (a null x), so no valid request leaves one of their grids empty.
2 A kernel that asks for more than 64 KiB of dynamic LDS has its limit raised first.  k_graclus and k_louvain have their
  cases (graclus_check.check_graclus_large: 72 004 bytes; test_gpu_louvain.test_graph_near_the_carve_limit: ~153 KiB) and
  k_bsa_residues asks for more in every call; the builder's k_iface_pairs gets its case here.

The training path's launches took the form one commit later; their cases (1b) were recorded in the same way from the emulation
build before it: a launch pair and a fused step of zero graphs that still carry the next mini-batch's topology request, the
builder's offsets prologue on 2 and on 0 nodes, and a backward launch that shares its grid with the builder.  Beyond 64 KiB of
dynamic LDS those kernels are launched by the suites that own them: k_topo<true> by test_gpu_topology_paths (cases C127 - C129
and N1024 / N1025: 72 928 - 152 480 bytes), k_net<.., true> by test_gpu_launch_pair's regime (ii) widths (backward launches of
156 000 - 161 664 bytes), k_net_co_topo by its co-built case (103 968 bytes + 34 628 of the staged head) and k_head by its
HEAD_STEP_CASES that go in passes (the largest chunk of hidden units that fits 160 KiB)."""
import numpy as np

from bsa_cases import same_bits

FILL = -7.0
FILL_I32 = -7
# chain B of the LDS case: 21 residues of 260 atoms, staged as one tile (iface_pairs_lds_bytes, csrc/drgnn_iface.h)
LDS_RES, LDS_ATOMS = 21, 260


def iface_pairs_lds_bytes(tile_atoms, residues_per_block=16):
    """iface_pairs_lds_bytes (csrc/drgnn_iface.h): three floats per staged atom and one per residue of the block (IF_AB)"""
    return 4 * (3 * tile_atoms + residues_per_block)


# ---- 1 partly empty calls ----------------------------------------------------------------------------------------------
def iface_without_chain_a(api, device):
    """two complexes of one and two residues, all of chain B: no chain-A block for the pairs kernel, while the spheres, the
    rows, the scan and the offsets run"""
    from deeprank_gnn_amd.interface import build_ragged
    xyz = np.array([[0, 0, 0], [0, 0, 0], [2, 0, 0]], dtype=np.float32)
    return build_ragged(api, xyz, np.array([0, 1, 2, 3]), np.array([0, 1, 3]), np.array([0, 1]), np.zeros(3, dtype=np.int32),
                        device=device)


def _words(device, M, n_a, n_b):
    import torch
    return torch.full((M, n_a, (n_b + 63) // 64), 3, dtype=torch.int64, device=device)


def counts_without_listed_poses(api, device):
    """two groups that list no pose: the outputs are cleared, cs_count has no list entry to take"""
    from deeprank_gnn_amd.interface import contact_counts_raw
    counts, residues = contact_counts_raw(api, _words(device, 2, 1, 2), 2, np.zeros(0, dtype=np.int64), np.zeros(3, dtype=np.int64))
    return {"counts": counts.cpu().numpy(), "residues": residues.cpu().numpy()}


def counts_without_residues(api, device):
    """n_chain_a + n_chain_b == 0 with one group of two listed poses: nothing to clear and nothing to count"""
    from deeprank_gnn_amd.interface import contact_counts_raw
    counts, residues = contact_counts_raw(api, _words(device, 2, 0, 0), 0, np.arange(2), np.array([0, 2]))
    return {"counts": counts.cpu().numpy(), "residues": residues.cpu().numpy()}


def segmax_without_clusters(api, device):
    """drgnn_segmax_backward of zero clusters: grad_x keeps what it held"""
    import torch
    from deeprank_gnn_amd import _lib
    grad_out = torch.ones((1, 2), dtype=torch.float32, device=device)
    arg = torch.zeros((1, 2), dtype=torch.int64, device=device)
    gx = torch.full((2, 2), FILL, dtype=torch.float32, device=device)
    api.segmax_backward(grad_out, arg, 0, 2, 2, gx, _lib.current_stream(gx))
    return {"grad_x": gx.cpu().numpy()}


def depth_by_phase(api, device):
    """two residues of one complex, both targets, n_dots 8: the whole call, then the three launches one call each on a
    workspace of their own (phases 1, 2, 4).  Returns the depths of the whole call and what `out` held after each phase"""
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.residue_features import _residue_request, depth_dots, depth_link
    xyz, rad, n_dots = np.array([[0, 0, 0], [3, 0, 0], [3, 1, 0]], dtype=np.float64), np.array([1.9, 1.7, 1.5]), 8
    n_bytes, _ = api.depth_workspace(3, 1, n_dots)
    got = {}
    for name, sequence in (("whole", (0,)), ("phase", (1, 2, 4))):
        r, out, status = _residue_request(_lib.DepthRequest, device, xyz, [0, 1, 3], [0, 2], None, [0, 1], [0, 0], ())
        r.input("radii", rad, torch.float64)
        r.input("dots", depth_dots(n_dots), torch.float64)
        r.output("workspace", max(1, n_bytes // 8), torch.int64, zeros=True)
        r.set(n_radii=3, probe=1.5, link=depth_link(n_dots), n_dots=n_dots, components=0, workspace_bytes=n_bytes)
        out.fill_(FILL)
        for phases in sequence:
            r.set(phases=phases)
            r.run(api, "depth_residues")
            got["%s %d" % (name, phases)] = out.cpu().numpy().copy()
        assert int(status.cpu()[0]) == 0
    return got


def rmsd_by_phase(api, device):
    """two poses of two atoms, the second the first moved by (3, 4, 0), no superposition: the whole call, then the records
    (phases 1) and the pairs (phases 2) one call each"""
    import torch
    from deeprank_gnn_amd.interface import pose_rmsd_raw
    xyz = torch.tensor([[[0, 0, 0], [1, 0, 0]], [[3, 4, 0], [4, 4, 0]]], dtype=torch.float32, device=device)
    idx = np.arange(2, dtype=np.int32)
    got = {"whole 0": pose_rmsd_raw(api, xyz, xyz, idx).cpu().numpy()}
    work = torch.zeros(max(api.rmsd_workspace(2, 2, 0, 2)[0] // 8, 1), dtype=torch.float64, device=device)
    d = torch.full((2, 2), FILL, dtype=torch.float64, device=device)
    for phases in (1, 2):
        pose_rmsd_raw(api, xyz, xyz, idx, phases=phases, workspace=work, out=d)
        got["phase %d" % phases] = d.cpu().numpy().copy()
    return got


# ---- 1b the training path: the launch pair, the fused step and the builder's offsets prologue ----------------------------
PAIR_FEAT = 4
REFUSALS = {"bad argument": -1, "workspace/capacity": -2, "unsupported width": -3}      # (_lib._check)


def return_code(call):
    """0, or the DRGNN_E_* code the call was refused with"""
    from deeprank_gnn_amd import _lib
    try:
        call()
    except _lib.DrgnnError as e:
        return np.int32(REFUSALS[str(e).rsplit(": ", 1)[1]])
    return np.int32(0)


def tiny_graph(nodes, edges, y=0.5):
    """`nodes` nodes, each a depth-0 cluster of its own, all in one depth-1 cluster; features on a grid of quarters"""
    import torch
    from deeprank_gnn_amd.data import Data
    g = Data(x=(torch.arange(nodes * PAIR_FEAT, dtype=torch.float32).reshape(nodes, PAIR_FEAT) % 5 - 2) / 4,
             edge_index=torch.tensor(edges, dtype=torch.int64).reshape(-1, 2).t().contiguous(),
             edge_attr=torch.ones(len(edges), 1), y=torch.tensor([y]), pos=torch.zeros(nodes, 3))
    g.cluster0, g.cluster1 = torch.arange(nodes), torch.zeros(nodes, dtype=torch.int64)
    return g


def unbuilt(api, device, graph):
    """an allocated workspace for a batch of this one graph (offset tables from the collation), every word FILL_I32"""
    from deeprank_gnn_amd.data import Batch
    from deeprank_gnn_amd.topology import Topology
    topo = Topology.from_batch(Batch.from_data_list([graph]).to(device), api=api, need_weights=False, build=False, with_tiles=False)
    topo.ws_i32.fill_(FILL_I32)
    return topo


def built_alone(api, device, graph):
    """... built by drgnn_topology_build_request alone"""
    from deeprank_gnn_amd import _lib
    topo = unbuilt(api, device, graph)
    api.topology_build_request(topo.request(_lib.TOPO_HIER), _lib.current_stream(topo.ws_i32))
    return topo


def workspace(topo, prefix="next "):
    """the status words, the offsets and every promised array (topo_cases.segments) of a one-graph workspace"""
    from topo_cases import segments
    out = {prefix + name: per_graph[0].copy() for name, per_graph in segments(topo, False).items()}
    out[prefix + "NPTR"], out[prefix + "EPTR"] = topo.array("NPTR").cpu().numpy()[:2], topo.array("EPTR").cpu().numpy()[:2]
    out[prefix + "status"] = np.array(topo.status(), dtype=np.int32)
    return out


def pair_trainer(api, device):
    """a GINet of PAIR_FEAT features behind a trainer that takes the launch pair (drgnn_net_forward +
    drgnn_net_backward_fused_head) whatever the shape"""
    import pair_check as pc
    from deeprank_gnn_amd.trainer import FusedTrainer
    tr = FusedTrainer(pc.build_net("GINet", pc.make_params("GINet", PAIR_FEAT), device), lr=0.01, task="reg", api=api)
    tr.fused_step = False
    return tr


NEXT_GRAPH = (2, [(0, 1), (1, 0)])
GRAD_SAMPLE = np.arange(4, 44, 4)      # ten elements of the flat gradient (conv1 of the first branch)


def empty_launch_with_next(api, device, fused):
    """a launch of ZERO graphs that carries the request for the next mini-batch's topology (one graph of 2 nodes, the edge in
    both directions): nothing to share a launch with, so the request is built by launches of its own.  fused: the call is
    drgnn_net_train_step, else drgnn_net_backward_fused_head.  The return code, the next workspace, and whether every word
    of it is what drgnn_topology_build_request alone leaves"""
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.functional import H1, H2, _describe
    tr = pair_trainer(api, device)
    nxt, alone = unbuilt(api, device, tiny_graph(*NEXT_GRAPH)), built_alone(api, device, tiny_graph(*NEXT_GRAPH))
    new = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=device)
    x, y, ws, pred, readout = new((4, PAIR_FEAT)), new(1), new(64, torch.int32), new((1, tr.O)), new((1, tr.R))
    partials = new((2, api.net_partial_elems(tr.kind, PAIR_FEAT)))
    desc, head, stream = _describe(tr.kind, PAIR_FEAT, tr.live, tr.n_branch), tr._head_desc(True), _lib.current_stream(x)
    request = nxt.request(_lib.TOPO_HIER)
    if fused:
        hints = _lib.StepHints()      # (what the device's plan asks of a workspace: the order and 16-byte aligned tiles)
        tiles = new(64)
        hints.topo_flags, hints.tiles = _lib.TOPO_HIER | _lib.TOPO_TILES, tiles.data_ptr()
        rc = return_code(lambda: api.net_train_step(
            desc, head, x, y, tr.step2, ws, None, 0, 0, 0, 1, 0, 1, pred, readout, new((1, api.head_compact_elems(tr.R, tr.H, tr.O))),
            partials, new(2 * max(tr.H, H2), torch.int64), stream, next_topology=request, hints=hints))
    else:
        rc = return_code(lambda: api.net_backward_fused_head(
            desc, head, x, readout, y, tr.step, ws, None, 0, 0, 0, 1, 0, 1, new((2, 4, H1)), new((2, 4, H1), torch.int32),
            new((2, 4, H2), torch.int32), pred, new((1, api.head_partial_elems(tr.R, tr.H, tr.O))), None, partials, None, stream,
            next_topology=request))
    got = workspace(nxt)
    got["rc"], got["next equals the build alone"] = np.array(rc), np.array(torch.equal(nxt.ws_i32, alone.ws_i32))
    return got


def topology_build_without_tables(api, device):
    """drgnn_topology_build without offset tables -- the prologue that clears the status words and derives NPTR / EPTR from
    the batch vector -- on one graph of 2 nodes and no edge (the items of the prologue span the nodes), then on one graph of
    0 nodes (one item, nothing to span; no LDS bound, so the builder works out of global scratch)"""
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.topology import Topology
    got = {}
    for n_nodes in (2, 0):
        topo = Topology(api, n_nodes, 0, 1, device, False)
        topo.ws_i32.fill_(FILL_I32)
        edge_index, batch = torch.zeros((2, 1), dtype=torch.int64, device=device), torch.zeros(2, dtype=torch.int64, device=device)
        cluster0, cluster1 = torch.arange(2, device=device), torch.zeros(2, dtype=torch.int64, device=device)
        scratch = torch.zeros(api.topology_scratch_elems(n_nodes, 0, 1), dtype=torch.int32, device=device)
        rc = return_code(lambda: api.topology_build(edge_index, None, batch, cluster0, cluster1, None, None, None, n_nodes, 0,
                                                    n_nodes, 1, n_nodes, 0, topo.ws_i32, None, scratch, _lib.current_stream(batch)))
        got.update({"%d nodes rc" % n_nodes: np.array(rc), "%d nodes NPTR" % n_nodes: topo.array("NPTR").cpu().numpy()[:2],
                    "%d nodes EPTR" % n_nodes: topo.array("EPTR").cpu().numpy()[:2],
                    "%d nodes status" % n_nodes: np.array(topo.status(), dtype=np.int32)})
    return got


def co_built_pair(api, device):
    """drgnn_net_backward_fused_head on one 3-node graph, alone and with the request for the next topology, whose offset tables
    let it share the launch: the same gradients, loss and predictions bit for bit, and a next workspace that is word for
    word the one drgnn_topology_build_request builds alone"""
    import torch
    from deeprank_gnn_amd.data import Batch
    from deeprank_gnn_amd.topology import Topology
    batch = Batch.from_data_list([tiny_graph(3, [(0, 1), (1, 0), (1, 2), (2, 1)])]).to(device)
    runs = {}
    for name in ("alone", "shared"):
        tr = pair_trainer(api, device)
        topo = Topology.from_batch(batch, api=api, need_weights=False)
        nxt = unbuilt(api, device, tiny_graph(*NEXT_GRAPH)) if name == "shared" else None
        # (what makes the backward launch take the request along: net_launch's co_ok, csrc/drgnn_capi.hip)
        assert nxt is None or (nxt._inputs[5] is not None and nxt._inputs[6] is not None and nxt._inputs[7] is not None)
        loss = tr.compute_gradients(batch, topo=topo, next_topo=nxt)
        runs[name] = (tr.flat_g.cpu().numpy().copy(), tr.last_pred.cpu().numpy().copy(), np.array(float(loss), dtype=np.float32), nxt)
    alone, shared = runs["alone"], runs["shared"]
    got = workspace(shared[3])
    got["next equals the build alone"] = np.array(torch.equal(shared[3].ws_i32, built_alone(api, device, tiny_graph(*NEXT_GRAPH)).ws_i32))
    got["gradients equal the launch alone"] = np.array(all(same_bits(a, b) for a, b in zip(alone[:3], shared[:3])))
    assert np.isfinite(shared[0]).all()
    got["gradient sample"], got["pred"], got["loss"] = shared[0][GRAD_SAMPLE], shared[1], shared[2]
    return got


_I32, _I64, _F32 = np.int32, np.int64, np.float32
_DEPTH = np.array([float.fromhex("0x1.e666666666666p+0"), float.fromhex("0x1.9999999999998p+0")])      # 1.9, 1.6 - 2 ulp
_UNTOUCHED = np.full(2, FILL)
_RMSD = np.array([[0.0, 5.0], [5.0, 0.0]])
CASES = {
    "iface_count without chain A": iface_without_chain_a,
    "contact_counts without listed poses": counts_without_listed_poses,
    "contact_counts without residues": counts_without_residues,
    "segmax_backward without clusters": segmax_without_clusters,
    "depth_residues phase by phase": depth_by_phase,
    "pose_rmsd phase by phase": rmsd_by_phase,
    "net_backward_fused_head without graphs, with the next topology": lambda api, device: empty_launch_with_next(api, device, False),
    "net_train_step without graphs, with the next topology": lambda api, device: empty_launch_with_next(api, device, True),
    "topology_build without offset tables": topology_build_without_tables,
    "net_backward_fused_head sharing its launch with the next topology": co_built_pair,
}
EXPECT = {
    "iface_count without chain A": {
        "node_ptr": np.zeros(3, _I32), "edge_ptr": np.zeros(3, _I32), "iedge_ptr": np.zeros(3, _I32),
        "node_residue": np.zeros(0, _I32), "pos": np.zeros((0, 3), _F32), "chain": np.zeros(0, _I32), "type": np.zeros(0, _I32),
        "edge_index": np.zeros((0, 2), _I64), "dist": np.zeros(0, _F32), "internal_edge_index": np.zeros((0, 2), _I64),
        "internal_dist": np.zeros(0, _F32)},
    "contact_counts without listed poses": {"counts": np.zeros((2, 1, 2), _I32), "residues": np.zeros((2, 3), _I32)},
    "contact_counts without residues": {"counts": np.zeros((1, 0, 0), _I32), "residues": np.zeros((1, 0), _I32)},
    "segmax_backward without clusters": {"grad_x": np.full((2, 2), FILL, _F32)},
    "depth_residues phase by phase": {"whole 0": _DEPTH, "phase 1": _UNTOUCHED, "phase 2": _UNTOUCHED, "phase 4": _DEPTH},
    "pose_rmsd phase by phase": {"whole 0": _RMSD, "phase 1": np.full((2, 2), FILL), "phase 2": _RMSD},
}


def _i32(*values):
    return np.array(values, _I32)


# The training-path cases, recorded from the emulation build of the commit before the launch form reached the training path.
# The workspace of the 2-node graph with its edge in both directions: status "no fault, no faulty graph" and every promised array
_NEXT = {"next status": _i32(0, -1, 0, 0), "next NPTR": _i32(0, 2), "next EPTR": _i32(0, 2), "next ROWPTR0": _i32(0, 1, 2),
         "next COL0": _i32(1, 0), "next EID0": _i32(0, 1), "next CL0": _i32(0, 1), "next NC0": _i32(2), "next ROWPTR1": _i32(0, 1, 2),
         "next COL1": _i32(1, 0), "next NE1": _i32(2), "next COLPTR1": _i32(0, 1, 2), "next ROWIDX1": _i32(1, 0), "next CL1": _i32(0, 0),
         "next NC1": _i32(1), "next MPTR1": _i32(0, 2), "next MEM1": _i32(0, 1), "next HORD": _i32(0, 1), "next HMP0": _i32(0, 1, 2),
         "next HSPLIT": _i32(0, 0, 0, 1), "next equals the build alone": np.array(True)}
_EMPTY_WITH_NEXT = dict(_NEXT, rc=np.array(0, _I32))
_SAMPLE = ["-0x1.562c1ep-9", "0x1.1313f8p-5", "0x1.4bdae6p-6", "-0x1.4e8558p-8", "-0x1.263a66p-13", "0x1.868a6cp-7", "0x0.0p+0",
           "-0x1.ac5498p-6", "0x1.39c34p-7", "-0x1.f57fd2p-7"]
EXPECT.update({
    "net_backward_fused_head without graphs, with the next topology": _EMPTY_WITH_NEXT,
    "net_train_step without graphs, with the next topology": _EMPTY_WITH_NEXT,
    "topology_build without offset tables": {
        "2 nodes rc": np.array(0, _I32), "2 nodes NPTR": _i32(0, 2), "2 nodes EPTR": _i32(0, 0), "2 nodes status": _i32(0, -1, 0, 0),
        "0 nodes rc": np.array(0, _I32), "0 nodes NPTR": _i32(0, 0), "0 nodes EPTR": _i32(0, 0), "0 nodes status": _i32(0, -1, 0, 0)},
    "net_backward_fused_head sharing its launch with the next topology": dict(
        _NEXT, **{"gradients equal the launch alone": np.array(True),
                  "gradient sample": np.array([float.fromhex(h) for h in _SAMPLE], _F32),
                  "pred": np.array([[float.fromhex("-0x1.18807ep-3")]], _F32), "loss": np.array(float.fromhex("0x1.9f75d6p-2"), _F32)}),
})
# What the device's floats may differ by from the emulation's recorded ones: |got - want| <= tol + rtol |want| with tol from
# DEVICE_TOL and rtol from DEVICE_RTOL.  depth: depth_cases.TOL; the RMSD case is exact in fp64; the launch pair: the element-wise
# rule of its own suite (elementwise.TOL, tests/pair_check.py).  Integers and flags are compared bit for bit on both builds.
DEVICE_TOL = {"depth_residues phase by phase": 1e-12, "net_backward_fused_head sharing its launch with the next topology": 1e-4}
DEVICE_RTOL = {"net_backward_fused_head sharing its launch with the next topology": 1e-4}


def check_case(name, api, device):
    got, want = CASES[name](api, device), EXPECT[name]
    assert sorted(got) == sorted(want), name
    tol, rtol = (DEVICE_TOL.get(name, 0.0), DEVICE_RTOL.get(name, 0.0)) if device != "cpu" else (0.0, 0.0)
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (name, key, got[key])
        if tol and want[key].dtype.kind == "f":
            assert bool((np.abs(got[key] - want[key]) <= tol + rtol * np.abs(want[key])).all()), (name, key, got[key])
        else:
            assert same_bits(got[key], want[key]), (name, key, got[key])
    if "phase 4" in got:                                               # (one build, one workspace content: the same bits)
        assert same_bits(got["phase 4"], got["whole 0"]), name


# ---- 2 dynamic LDS beyond 64 KiB ---------------------------------------------------------------------------------------
def iface_large_tile(api, device, tile_atoms):
    """one complex: a chain A of one atom next to a chain B of LDS_RES residues of LDS_ATOMS atoms on a 1/8 A grid, chain B
    staged in tiles of ``tile_atoms``"""
    from deeprank_gnn_amd.interface import build_ragged
    rng = np.random.default_rng(64)
    n_b = LDS_RES * LDS_ATOMS
    centre = np.repeat(np.stack((np.full(LDS_RES, 6.0), 4.0 * np.arange(LDS_RES), np.zeros(LDS_RES)), axis=1), LDS_ATOMS, axis=0)
    b = np.round((centre + rng.uniform(-1.5, 1.5, (n_b, 3))) * 8) / 8
    xyz = np.concatenate(([[0.0, 0.0, 0.0]], b)).astype(np.float32)
    atom_ptr = np.concatenate(([0], 1 + LDS_ATOMS * np.arange(LDS_RES + 1)))
    return build_ragged(api, xyz, atom_ptr, np.array([0, LDS_RES + 1]), np.array([1]), np.arange(LDS_RES + 1, dtype=np.int32) % 20,
                        device=device, tile_atoms=tile_atoms)


def check_iface_beyond_64k(api, device):
    """chain B in one tile of 5 460 atoms (65 584 bytes of dynamic LDS) against the default tile of 4 096 (49 216 bytes):
    the same bits, and edges to find.  Returns the large-tile result"""
    n_b = LDS_RES * LDS_ATOMS
    assert iface_pairs_lds_bytes(n_b) == 65584 > 64 * 1024 > iface_pairs_lds_bytes(4096)
    large, default = iface_large_tile(api, device, n_b), iface_large_tile(api, device, 0)
    assert sorted(large) == sorted(default) and all(same_bits(large[k], default[k]) for k in large)
    assert large["edge_ptr"].tolist()[1] >= 2 and large["iedge_ptr"].tolist()[1] >= 1
    return large
