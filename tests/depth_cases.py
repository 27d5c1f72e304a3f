"""Inputs and checks shared by tests/test_depth.py (host emulation) and tests/test_gpu_depth.py (the device): the residue
depth of deeprank_gnn_amd.interface (drgnn_depth_residues, csrc/drgnn_depth.h) against the float64 statement of the rule
in tests/depth_ref.py, which sees the float32 coordinates the kernel sees.

The accessible dots, the component labels and the component kept are integers and are held to equality; TOL, the one
tolerance of the depth (absolute, A), is the issue's 1e-12: kernel and rule do the same fp64 operations in the same order,
so equal bits are expected, and 1e-12 is a few thousand units in the last place of a depth of a few A."""
import os

import numpy as np

import depth_ref as R
from bsa_cases import atn, same_bits
from helpers import GOLDEN

TOL = 1e-12
_SURF = {}


def rounded(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ---- 1ATN ------------------------------------------------------------------------------------------------------------
def atn_x(m):
    a = atn()
    return rounded(a["xyz"][m][a["table"].order])


def atn_surface(m, n_dots=R.N_DOTS):
    """depth_ref's surface ("outer") of pose m on the float32 coordinates, computed once per request and left unchanged"""
    if (m, n_dots) not in _SURF:
        t = atn()["table"]
        _SURF[(m, n_dots)] = R.surface(atn_x(m), R.radii_of(t.atom_name), n_dots=n_dots)
    return _SURF[(m, n_dots)]


def all_of(surf):
    """the same surface under components="all\""""
    return dict(surf, keep=np.ones_like(surf["keep"]), outer=-1)


def recorded():
    """per pose the fixture's node_data/depth, in the order of atn()["nodes"]"""
    a = atn()
    with np.load(os.path.join(GOLDEN, "fixture_1ATN.npz")) as f:
        return [f[mol + "/node_data/depth"].reshape(-1).copy() for mol in a["mols"]]


def figures(got, rec):
    e = got - rec
    return {"rms": float(np.sqrt((e * e).mean())), "mean": float(e.mean()), "r": float(np.corrcoef(got, rec)[0, 1]),
            "share": float((np.abs(e) <= 0.5).mean()), "worst": float(np.abs(e).max())}


def check_ref_against_recorded():
    """issue check 1: the rule at its defaults against the 496 recorded values; measured here: rms 0.152 A, mean
    -0.027 A, r 0.990, share within 0.5 A 0.994, worst 1.72 A; with every component kept: rms 0.378 A, r 0.938"""
    a = atn()
    t = a["table"]
    rad = R.radii_of(t.atom_name)
    rec = recorded()
    assert sum(len(r) for r in rec) == 496
    outer, every = [], []
    for m in range(4):
        surf = atn_surface(m)
        outer.append(R.residue_depth(atn_x(m), t.atom_ptr, rad, a["nodes"][m], surf=surf)[0])
        every.append(R.residue_depth(atn_x(m), t.atom_ptr, rad, a["nodes"][m], surf=all_of(surf))[0])
    f, g = figures(np.concatenate(outer), np.concatenate(rec)), figures(np.concatenate(every), np.concatenate(rec))
    print("outer component: rms %(rms).3f A, mean %(mean).3f A, r %(r).4f, within 0.5 A %(share).4f, worst %(worst).2f A" % f)
    print("all components:  rms %(rms).3f A, mean %(mean).3f A, r %(r).4f, within 0.5 A %(share).4f, worst %(worst).2f A" % g)
    assert f["rms"] <= 0.19 and abs(f["mean"]) <= 0.06 and f["r"] >= 0.985 and f["share"] >= 0.985
    assert g["r"] < 0.96


def run_raw(api, device, x, atom_ptr, rad, targets=None, **opt):
    """(depth [K], the surface the call left) of one complex through depth_raw"""
    from deeprank_gnn_amd.interface import depth_raw
    n = len(atom_ptr) - 1
    targets = np.arange(n) if targets is None else np.asarray(targets, dtype=np.int64)
    out, status, surf = depth_raw(api, x, atom_ptr, [0, n], rad, targets, np.zeros(len(targets), dtype=np.int64), device=device,
                                  parts=True, **opt)
    assert status == 0
    return out, surf[0]


def equal_depth(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (what, got, want)
    dev = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    assert dev <= TOL, (what, dev)
    return dev


def equal_to_rule(api, device, x, atom_ptr, rad, targets=None, what="", ref=None, **opt):
    """issue check 2 for one complex: masks, labels, the component kept and the depths.  Returns (got, want, ref surface)"""
    got, surf = run_raw(api, device, x, atom_ptr, rad, targets, **opt)
    which = opt.pop("components", "outer")
    if ref is None:
        ref = R.surface(rounded(x), np.asarray(rad, dtype=np.float64), which=which, **opt)
    want = R.residue_depth(rounded(x), atom_ptr, rad, targets, probe=opt.get("probe", R.PROBE), surf=ref)[0]
    assert np.array_equal(surf["mask"], ref["mask"]), (what, "accessible dots")
    assert np.array_equal(surf["ids"], ref["ids"]), (what, "dot ids")
    assert np.array_equal(surf["label"], ref["label"]), (what, "component labels")
    assert surf["outer"] == ref["outer"], (what, "component kept", surf["outer"], ref["outer"])
    dev = equal_depth(got, want, what)
    print("%s: %d accessible dots, %d components, kept %d, largest |depth - depth_ref| = %.3g A"
          % (what, len(ref["ids"]), len(np.unique(ref["label"])), ref["outer"], dev))
    return got, want, ref


def emu_subset():
    """twelve nodes of pose 1w, the deepest and the shallowest recorded among them"""
    a = atn()
    nodes, rec = a["nodes"][0], recorded()[0]
    order = np.argsort(rec)
    pick = [int(order[0]), int(order[-1])] + [int(i) for i in order[5:-5:len(order) // 10][:10]]
    assert len(set(pick)) == 12
    return np.array(sorted(int(nodes[i]) for i in pick))


def check_atn(api, device, m, n_dots=R.N_DOTS, subset=None):
    """one pose: the node residues (or `subset`) against the rule"""
    a = atn()
    t = a["table"]
    targets = np.sort(a["nodes"][m]) if subset is None else subset
    x = a["xyz"][m][t.order]
    return equal_to_rule(api, device, x, t.atom_ptr, R.radii_of(t.atom_name), targets, a["mols"][m], ref=atn_surface(m, n_dots),
                         n_dots=n_dots)


def cutout(n_a=12, n_b=12):
    """(table, xyz [4, T', 3]): the first residues of both chains of 1ATN as a complex of its own, the four poses"""
    from deeprank_gnn_amd.interface import AtomTable
    a = atn()
    t = a["table"]
    res = np.concatenate((np.arange(n_a), t.split + np.arange(n_b)))
    grouped = np.concatenate([np.arange(t.atom_ptr[r], t.atom_ptr[r + 1]) for r in res])
    idx = np.sort(t.order[grouped])
    chain, seq, name, atom = (np.asarray(v)[idx] for v in a["per_atom"])
    xyz = a["xyz"][:, idx]
    return AtomTable(chain, seq, name, xyz[0], atom_name=atom), xyz


# ---- hand-made atoms -------------------------------------------------------------------------------------------------
def spiral(n, radius):
    return R.unit_dots(n) * radius


def hand(residues):
    """(x, atom_ptr, rad) of residues [[(xyz, radius), ...], ...]"""
    x = np.array([p for atoms in residues for p, _ in atoms], dtype=np.float64).reshape(-1, 3)
    rad = np.array([r for atoms in residues for _, r in atoms], dtype=np.float64)
    atom_ptr = np.concatenate(([0], np.cumsum([len(atoms) for atoms in residues])))
    return x, atom_ptr, rad


SHELL_RADIUS = 8.0                     # a closed shell of 400 atoms: its inner surface (4.6 A) leaves the probe room
AXES = [(1.5, 0, 0), (-1.5, 0, 0), (0, 1.5, 0), (0, -1.5, 0), (0, 0, 1.5), (0, 0, -1.5)]


def check_hand_case(name, api, device):
    kw = {"what": name}
    if name == "one_atom":                                             # every dot is accessible: depth = the radius
        x, ap, rad = hand([[((1.0, 2.0, 3.0), 1.9)]])
        got, want, ref = equal_to_rule(api, device, x, ap, rad, **kw)
        assert ref["mask"].all() and abs(got[0] - 1.9) <= 1e-12
    elif name == "two_far_atoms":                                      # two equal components: the first is kept
        x, ap, rad = hand([[((0.0, 0.0, 0.0), 1.9)], [((20.0, 0.0, 0.0), 1.7)]])
        got, want, ref = equal_to_rule(api, device, x, ap, rad, **kw)
        assert ref["mask"].all() and ref["outer"] == 0 and sorted(set(ref["label"].tolist())) == [0, 192]
        gap = 20.0 - 3.4 - 1.5                                         # to the first atom's surface, within a dot spacing
        assert abs(got[0] - 1.9) <= 1e-12 and gap <= got[1] <= gap + 0.5
    elif name == "hollow_shell":                                       # the cavity's component is dropped, or kept
        shell = [[(tuple(p), 1.9)] for p in spiral(400, SHELL_RADIUS)]
        x, ap, rad = hand([[((0.0, 0.0, 0.0), 1.9)]] + shell)
        outer, _, ref = equal_to_rule(api, device, x, ap, rad, targets=[0], n_dots=64, **kw)
        every, _, _ = equal_to_rule(api, device, x, ap, rad, targets=[0], n_dots=64, components="all", **kw)
        assert len(np.unique(ref["label"])) == 2 and ref["mask"][0].all() and ref["outer"] != ref["label"][0]
        spacing = R.default_link(64) / 1.5
        assert abs(every[0] - 1.9) <= 1e-12                            # its own dots
        assert abs((outer[0] - every[0]) - SHELL_RADIUS) <= spacing, (outer, every)   # (8 + 3.4 - 1.5) - 1.9
    elif name == "buried_atom":                                        # six neighbours at 1.5 A cover every dot
        x, ap, rad = hand([[((0.0, 0.0, 0.0), 1.9)]] + [[(p, 1.9)] for p in AXES])
        got, want, ref = equal_to_rule(api, device, x, ap, rad, **kw)
        assert not ref["mask"][0].any() and ref["mask"][1:].any(axis=1).all() and np.isfinite(got).all() and got[0] > 1.9
    elif name == "same_place":
        x, ap, rad = hand([[((0.5, 0.25, 0.0), 1.9), ((0.5, 0.25, 0.0), 1.9)], [((2.0, 0.25, 0.0), 1.5)]])
        equal_to_rule(api, device, x, ap, rad, **kw)
        x, ap, rad = hand([[((0.5, 0.25, 0.0), 1.9), ((0.5, 0.25, 0.0), 1.5)]])
        got, _, ref = equal_to_rule(api, device, x, ap, rad, **kw)
        assert ref["mask"][0].all() and not ref["mask"][1].any()
    elif name == "hydrogens_only":                                     # radius 0: no dots, a depth all the same
        x, ap, rad = hand([[((0.0, 0.0, 0.0), 1.9), ((1.5, 0.0, 0.0), 1.7)], [((0.5, 1.0, 0.0), 0.0), ((4.0, 0.0, 0.0), 0.0)]])
        got, want, ref = equal_to_rule(api, device, x, ap, rad, **kw)
        assert not ref["mask"][2:].any() and np.isfinite(got).all() and got[1] != got[0]
        x, ap, rad = hand([[((0.0, 0.0, 0.0), 0.0)]])                  # nothing but hydrogens: no surface at all
        got, _, ref = equal_to_rule(api, device, x, ap, rad, **kw)
        assert got[0] == np.inf and ref["outer"] == -1
    elif name == "singletons":                                         # a link below the dot spacing
        x, ap, rad = hand([[((1.0, 2.0, 3.0), 1.9)]])
        got, want, ref = equal_to_rule(api, device, x, ap, rad, link=0.01, n_dots=65, **kw)
        assert np.array_equal(ref["label"], np.arange(65)) and ref["outer"] == 0
        none, _, _ = equal_to_rule(api, device, x, ap, rad, link=0.0, n_dots=65, **kw)
        assert same_bits(none, got)
    else:
        raise KeyError(name)


HAND_CASES = ("one_atom", "two_far_atoms", "hollow_shell", "buried_atom", "same_place", "hydrogens_only", "singletons")
DOT_COUNTS = (1, 63, 64, 65, 192)


def check_dot_count(api, device, n_dots):
    """a cut-out of 1ATN at `n_dots` dots per atom"""
    t, xyz = cutout()
    equal_to_rule(api, device, xyz[0][t.order], t.atom_ptr, R.radii_of(t.atom_name), what="n_dots %d" % n_dots, n_dots=n_dots)


# ---- independence (issue check 3) ------------------------------------------------------------------------------------
def check_independence(api, device, n_dots=64):
    """batch, chunk, the place in the target list and the run change no bit.  Returns the batch's result [3, R]"""
    from deeprank_gnn_amd.interface import AtomTable, depth_radii, depth_raw, residue_depth
    t, xyz = cutout()
    kw = {"api": api, "device": device, "n_dots": n_dots}
    poses = AtomTable.poses(t, xyz[:3])
    full = residue_depth(poses, **kw)
    assert full.shape == (3, t.n_residues) and np.isfinite(full).all()
    for m in range(3):
        assert same_bits(full[m], residue_depth(AtomTable.poses(t, xyz[m:m + 1]), **kw)[0]), m      # alone
    assert same_bits(full, residue_depth(poses, chunk=1, **kw)) and same_bits(full, residue_depth(poses, chunk=2, **kw))
    assert same_bits(full[::-1], residue_depth(AtomTable.poses(t, xyz[:3][::-1]), **kw))             # another place
    for _ in range(3):
        assert same_bits(full, residue_depth(poses, **kw))
    r, rad = 5, depth_radii(t)
    others = [k for k in range(t.n_residues) if k != r]
    for order in ([r] + others, others + [r], [r]):                    # first, last and alone in the target list
        out, status = depth_raw(api, xyz[1][t.order], t.atom_ptr, [0, t.n_residues], rad, order, np.zeros(len(order), int),
                                n_dots=n_dots, device=device)
        assert status == 0 and same_bits(out[order.index(r)], full[1, r])
    part = residue_depth(poses, residues=[r, 2], **kw)
    assert same_bits(part[:, [r, 2]], full[:, [r, 2]]) and np.isnan(part).sum() == 3 * (t.n_residues - 2)
    want = R.residue_depth(rounded(xyz[1][t.order]), t.atom_ptr, R.radii_of(t.atom_name), n_dots=n_dots)[0]
    equal_depth(full[1], want, "the batch against the rule")
    return full


def device_equals_emulation(api, full):
    """issue check 4: the batch of check 3 and three hand cases, the device against the host emulation"""
    from emu_api import emu
    host = check_independence(emu(), "cpu")
    equal_depth(full, host, "device against emulation")
    cases = [hand([[((0.0, 0.0, 0.0), 1.9)]] + [[(p, 1.9)] for p in AXES]),
             hand([[((0.0, 0.0, 0.0), 1.9)], [((20.0, 0.0, 0.0), 1.7)]]),
             hand([[((0.5, 0.25, 0.0), 1.9), ((0.5, 0.25, 0.0), 1.9)], [((2.0, 0.25, 0.0), 1.5)]])]
    for x, ap, rad in cases:
        d, sd = run_raw(api, "cuda", x, ap, rad, n_dots=65)
        h, sh = run_raw(emu(), "cpu", x, ap, rad, n_dots=65)
        assert np.array_equal(sd["mask"], sh["mask"]) and np.array_equal(sd["label"], sh["label"]) and sd["outer"] == sh["outer"]
        equal_depth(d, h, "hand case, device against emulation")


# ---- refusals (issue check 5) ----------------------------------------------------------------------------------------
def check_value_errors():
    """the Python side refuses before anything is uploaded (api=object() would fail at the first call)"""
    import pytest
    from deeprank_gnn_amd.interface import AtomTable, depth_radii, interface_graphs, interface_resident_set, residue_depth
    t, xyz = cutout(3, 3)
    a = atn()
    kw = {"api": object(), "device": "cpu"}
    n = t.n_input_atoms
    bare = AtomTable(["A"] * n, np.arange(n), ["ALA"] * n, np.zeros((n, 3)))
    odd = AtomTable(["A", "B"], [1, 2], ["ALA", "ALA"], np.zeros((2, 3)), atom_name=["CA", "1"])
    for call in (lambda: depth_radii(bare), lambda: residue_depth(bare, **kw),
                 lambda: interface_graphs([bare], ["x"], depth=True, **kw)):
        with pytest.raises(ValueError, match="atom_name"):
            call()
    with pytest.raises(ValueError, match="no radius"):
        residue_depth(odd, **kw)
    with pytest.raises(ValueError, match="n_dots"):
        residue_depth(t, n_dots=0, **kw)
    with pytest.raises(ValueError, match="probe"):
        residue_depth(t, probe=0.0, **kw)
    with pytest.raises(ValueError, match="probe"):
        residue_depth(t, probe=-1.5, **kw)
    with pytest.raises(ValueError, match="components"):
        residue_depth(t, components="inner", **kw)
    with pytest.raises(ValueError, match="components"):
        interface_graphs([t], ["x"], depth={"components": "largest"}, **kw)
    with pytest.raises(ValueError, match="link"):
        residue_depth(t, link=-1.0, **kw)
    with pytest.raises(ValueError, match="radi"):
        residue_depth(t, radii=np.ones(3), **kw)
    with pytest.raises(ValueError, match="residue index"):
        residue_depth(t, residues=[t.n_residues], **kw)
    with pytest.raises(ValueError, match="built-in"):
        interface_resident_set([t], ["x"], node_feature=["type", "depth"], residue_features={"depth": np.zeros(t.n_residues)}, **kw)
    with pytest.raises(ValueError, match="depth"):
        interface_resident_set([t], ["x"], node_feature=["type", "depth"], depth=False, **kw)
    rad = np.full(n, 1.5)
    assert np.array_equal(depth_radii(t, rad), rad) and depth_radii(t).dtype == np.float64


def check_capacity(api, device):
    """a complex beyond the documented capacity is refused, never a number; the complex next to it keeps its value"""
    import pytest
    from deeprank_gnn_amd._lib import DrgnnError
    from deeprank_gnn_amd.interface import AtomTable, depth_raw, residue_depth
    dots, per_complex = api.depth_capacity(0), api.depth_capacity(1)
    assert dots == 4096 and per_complex == 4194304 and api.depth_capacity(9) == -1
    n = per_complex // dots + 1
    big = np.stack((4.0 * np.arange(n), np.zeros(n), np.zeros(n)), axis=1)
    small = np.array([[0.0, 50.0, 0.0]])
    x = np.concatenate((big, small))
    out, status = depth_raw(api, x, np.arange(n + 2), [0, n, n + 1], np.full(n + 1, 1.9), [0, n - 1, n], [0, 0, 1], n_dots=dots,
                            device=device)
    assert status & 1 and np.isnan(out[:2]).all()
    alone, status = depth_raw(api, small, [0, 1], [0, 1], [1.9], [0], [0], n_dots=dots, device=device)
    assert status == 0 and same_bits(out[2], alone[0]) and abs(alone[0] - 1.9) <= 1e-12
    table = AtomTable(["A"] * n, np.arange(n), ["ALA"] * n, big, atom_name=["C"] * n)
    with pytest.raises(DrgnnError, match="capacity"):
        residue_depth(table, residues=[0], n_dots=dots, api=api, device=device)
    with pytest.raises(DrgnnError, match="capacity"):                  # more dots per atom than the kernels take
        depth_raw(api, small, [0, 1], [0, 1], [1.9], [0], [0], n_dots=dots + 1, device=device)


def check_empty_targets(api, device):
    from deeprank_gnn_amd.interface import depth_raw, residue_depth
    t, xyz = cutout(3, 3)
    out, status = depth_raw(api, t.xyz, t.atom_ptr, [0, t.n_residues], R.radii_of(t.atom_name), [], [], device=device)
    assert out.shape == (0,) and status == 0
    got = residue_depth(t, residues=[], api=api, device=device)
    assert got.shape == (t.n_residues,) and np.isnan(got).all()
    assert residue_depth([], api=api, device=device) == []


REFUSALS = {"null xyz": {"xyz": None}, "null radii": {"radii": None}, "null dots": {"dots": None}, "null out": {"out": None},
            "null status": {"status": None}, "null workspace": {"workspace": None}, "null host_atom_ptr": {"host_atom_ptr": None},
            "null target_res": {"target_res": None}, "n_dots 0": {"n_dots": 0}, "probe 0": {"probe": 0.0},
            "probe NaN": {"probe": float("nan")}, "link negative": {"link": -1.0}, "components 2": {"components": 2}, "phases 8": {"phases": 8},
            "n_radii does not divide": {"n_radii": 4}, "n_targets negative": {"n_targets": -1},
            "small workspace": {"workspace_bytes": 64}}


def check_refusal(api, device, name):
    """one malformed field: refused before a launch (out keeps its fill); the good request runs"""
    import pytest
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._lib import DrgnnError
    from deeprank_gnn_amd.interface import depth_dots
    dev = torch.device(device)
    x, ap, rad = hand([[((0.0, 0.0, 0.0), 1.9), ((1.5, 0.0, 0.0), 1.7)], [((0.5, 1.0, 0.0), 0.0)], [((8.0, 0.0, 0.0), 1.5)]])
    host = {"atom_ptr": ap.astype(np.int32), "res_ptr": np.array([0, 3], np.int32), "target_res": np.arange(3, dtype=np.int32),
            "target_complex": np.zeros(3, np.int32)}
    if name == "target past its complex":
        host["target_res"] = np.array([0, 1, 3], np.int32)
    if name == "atom_ptr decreases":
        host["atom_ptr"] = np.array([0, 3, 2, 4], np.int32)
    d = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    d.update(xyz=torch.from_numpy(x.astype(np.float32)).to(dev), radii=torch.from_numpy(rad).to(dev),
             dots=torch.from_numpy(depth_dots(32)).to(dev))
    n_bytes, _ = api.depth_workspace(4, 1, 32)
    work = torch.empty(n_bytes // 8, dtype=torch.int64, device=dev)
    out = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def request(tables, **over):
        q = _lib.DepthRequest()
        for k in ("xyz", "radii", "dots", "atom_ptr", "res_ptr", "target_res", "target_complex"):
            setattr(q, k, d[k].data_ptr())
        for k, v in tables.items():
            setattr(q, "host_" + k, v.ctypes.data)
        q.n_atoms, q.n_residues, q.n_complexes, q.n_targets, q.n_radii = 4, 3, 1, 3, 4
        q.probe, q.link, q.n_dots, q.components = 1.5, 1.0, 32, 0
        q.workspace, q.workspace_bytes, q.out, q.status = work.data_ptr(), n_bytes, out.data_ptr(), status.data_ptr()
        for k, v in over.items():
            setattr(q, k, v)
        return q

    stream = _lib.current_stream(d["xyz"])
    over = dict(REFUSALS.get(name, {}))
    if name == "n_radii does not divide":
        over = {"n_radii": 3}
    with pytest.raises(DrgnnError, match="capacity" if name == "small workspace" else "bad argument"):
        api.depth_residues(request(host, **over), stream)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((out == -7).all()) and int(status.cpu()[0]) == 0      # nothing was launched
    good = {"atom_ptr": ap.astype(np.int32), "res_ptr": host["res_ptr"], "target_res": np.arange(3, dtype=np.int32),
            "target_complex": host["target_complex"]}
    d.update({k: torch.from_numpy(v).to(dev) for k, v in good.items()})
    api.depth_residues(request(good), stream)
    want = R.residue_depth(x, ap, rad, n_dots=32, link=1.0)[0]
    equal_depth(out.cpu().numpy(), want, "the good request")
    assert int(status.cpu()[0]) == 0


def refusal_names():
    return sorted(REFUSALS) + ["target past its complex", "atom_ptr decreases"]


# ---- through the layers (issue check 6) ------------------------------------------------------------------------------
TREG_MEASURED = 0.0        # |prediction from atoms - prediction with the recorded depth|, see check_graphs


def check_graphs(api, device, outdir, poses=(0,), nn_kw=None, **opt):
    """interface_graphs(depth=...) writes node_data/depth = residue_depth on the nodes and leaves every other key as it
    is; GraphDataSet loads the reference's feature list with it; pretrained_treg's prediction from these graphs against
    the same graphs with the fixture's recorded depth.

    The shipped checkpoint lists type, polarity, bsa, charge, cons, ic, pssm: it does not read `depth`, so the difference
    measured on the emulation build is exactly 0 (TREG_MEASURED) and the bound, 1.5 x that, is 0 as well.  It is not the
    1e-4 parity bound because the two depths are different quantities (a dot surface against MSMS, 0.15 A rms apart); a
    GraphDataSet over the reference's full feature list shows the column a net that reads depth would see."""
    import torch
    from iface_cases import match_by_pos
    from helpers import NODE_FEATURES, golden, params_of
    from deeprank_gnn_amd.clustering import PreCluster
    from deeprank_gnn_amd.dataset import GraphDataSet, GraphStore
    from deeprank_gnn_amd.ginet import GINet
    from deeprank_gnn_amd.interface import AtomTable, interface_graphs, residue_depth
    from deeprank_gnn_amd.NeuralNet import NeuralNet
    a = atn()
    t = a["table"]
    mols = [a["mols"][m] for m in poses]
    batch = AtomTable.poses(t, a["xyz"][list(poses)])
    built = interface_graphs(batch, mols, api=api, device=device, depth=(opt or True), bsa=True)
    plain = interface_graphs(batch, mols, api=api, device=device, bsa=True)
    direct = residue_depth(batch, api=api, device=device, residues=[built.get(mol, "node_data/residue") for mol in mols], **opt)
    fixture = GraphStore(os.path.join(GOLDEN, "fixture_1ATN.npz"))
    mine, theirs = [], []
    for k, mol in enumerate(mols):
        assert sorted(built._mols[mol]) == sorted(list(plain._mols[mol]) + ["node_data/depth"])
        for key in plain._mols[mol]:
            assert same_bits(built.get(mol, key), plain.get(mol, key)), (mol, key)
        depth = built.get(mol, "node_data/depth")
        nodes = built.get(mol, "node_data/residue")
        assert depth.dtype == np.float64 and depth.shape == (len(nodes),) and same_bits(depth, direct[k][nodes])
        perm = match_by_pos(built.get(mol, "node_data/pos"), fixture.get(mol, "node_data/pos"))
        rec = fixture.get(mol, "node_data/depth")
        print("%s: node_data/depth against the fixture: %s" % (mol, figures(depth[perm], rec.reshape(-1))))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        tree = {key: (v[perm] if key.startswith("node_data/") or key == "nodes" else v) for key, v in built._mols[mol].items()}
        tree["edge_index"] = inv[built.get(mol, "edge_index")]
        tree["internal_edge_index"] = inv[built.get(mol, "internal_edge_index")]
        for key, v in fixture._mols[mol].items():                     # hse, cons, ic, pssm and the scores: recorded
            if (key.startswith("node_data/") and key not in tree) or key.startswith("score/"):
                tree[key] = v
        other = dict(tree)
        other["node_data/depth"] = rec
        mine.append(tree)
        theirs.append(other)
    stores = [GraphStore.from_trees(mols, mine), GraphStore.from_trees(mols, theirs)]
    sets = [GraphDataSet(st, node_feature=list(NODE_FEATURES), edge_feature=["dist"], target="irmsd") for st in stores]
    at = 20 + 4 + 1                                                    # type, polarity, bsa come before depth
    assert sets[0][0].x.shape == (len(mine[0]["nodes"]), 20 + 4 + 1 + 1 + 3 + 1 + 20)
    assert np.array_equal(sets[0][0].x[:, at].numpy(), mine[0]["node_data/depth"].astype(np.float32))
    for ds in sets:
        PreCluster(ds, method="mcl", api=api, device=device)
    g = golden("pretrained_treg.npz")
    feats = [str(f) for f in g["node_feature"]]
    ck = os.path.join(str(outdir), "pretrained_treg.pth.tar")
    torch.save({'model': params_of(g), 'optimizer': {'state': {}, 'param_groups': [{'lr': 0.001, 'betas': (0.9, 0.999),
                                                                                  'eps': 1e-08, 'weight_decay': 0}]},
                'node': feats, 'edge': ['dist'], 'target': str(g["target_name"]), 'task': "reg", 'classes': [0, 1],
                'class_weight': None, 'batch_size': 64, 'percent': [1.0, 0.0], 'lr': 0.001, 'index': None, 'shuffle': False,
                'threshold': 0.3, 'cluster_nodes': 'mcl', 'transform_sigmoid': False}, ck)
    outs = []
    for st in stores:
        model = NeuralNet(st, GINet, pretrained_model=ck, outdir=str(outdir), **(nn_kw or {}))
        model.test(hdf5=None)
        outs.append(np.asarray(model.test_out, dtype=np.float64).reshape(len(mols), -1))
    diff = float(np.abs(outs[0] - outs[1]).max())
    print("pretrained_treg (features %s): from atoms %s, with the recorded depth %s, difference %.3g (bound %.3g)"
          % (feats, outs[0].ravel(), outs[1].ravel(), diff, 1.5 * TREG_MEASURED))
    assert np.isfinite(outs[0]).all() and diff <= 1.5 * TREG_MEASURED


def check_resident_set(api, device, poses=(0, 1), **opt):
    """interface_resident_set(node_feature=[..., "depth"]) equals the path through the store bit for bit"""
    import pack_cases as P
    import score_cases as SC
    from deeprank_gnn_amd.clustering import PreCluster
    from deeprank_gnn_amd.dataset import GraphDataSet, GraphStore
    from deeprank_gnn_amd.interface import AtomTable, interface_graphs, interface_resident_set
    from deeprank_gnn_amd.resident import ResidentGraphSet
    case, record = SC.atn()
    mols = [record["mols"][m] for m in poses]
    batch = AtomTable.poses(case.table, np.stack([case.poses[m] for m in poses]))
    features = ["type", "depth", "pos", "hse", "charge"]
    depth = opt or True
    store = interface_graphs(batch, mols, api=api, device=device, reference=case.sref, hse=True, depth=depth)
    ds = GraphDataSet(store, node_feature=features, edge_feature=["dist"], target="irmsd", clustering_method="mcl")
    PreCluster(ds, method="mcl", api=api, device=device)
    want = ResidentGraphSet(ds, device, api=api)
    for chunk in (None, 1):
        got = interface_resident_set(batch, mols, node_feature=features, reference=case.sref, target="irmsd", depth=depth,
                                     chunk=chunk, api=api, device=device)
        assert got.n_feat == want.n_feat == 28
        P.assert_sets_equal(got, want, "1ATN with depth, chunk %s" % chunk, attr="default")
    x = got.x.cpu().numpy()
    assert np.array_equal(x[:got.node_ptr[1], 20], store.get(mols[0], "node_data/depth").astype(np.float32))
    twice = interface_resident_set(batch, mols, node_feature=["depth", "type", "depth"], depth=depth, api=api, device=device)
    x = twice.x.cpu().numpy()
    assert twice.mols == mols and twice.n_feat == 22
    for g, mol in enumerate(mols):                                     # listed twice: two equal columns, the store's values
        rows = x[twice.node_ptr[g]:twice.node_ptr[g + 1]]
        for col in (0, 21):
            assert same_bits(rows[:, col].copy(), store.get(mol, "node_data/depth").astype(np.float32)), (mol, col)
