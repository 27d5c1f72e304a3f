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
  k_bsa_residues asks for more in every call; the builder's k_iface_pairs gets its case here."""
import numpy as np

from bsa_cases import same_bits

FILL = -7.0
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
# what the device may differ by from the emulation's recorded floats (depth_cases.TOL; the RMSD case is exact in fp64)
DEVICE_TOL = {"depth_residues phase by phase": 1e-12}


def check_case(name, api, device):
    got, want = CASES[name](api, device), EXPECT[name]
    assert sorted(got) == sorted(want), name
    tol = DEVICE_TOL.get(name, 0.0) if device != "cpu" else 0.0
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (name, key, got[key])
        if tol:
            assert float(np.abs(got[key] - want[key]).max()) <= tol, (name, key, got[key])
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
