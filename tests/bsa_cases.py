"""Inputs and checks shared by tests/test_bsa.py (host emulation) and tests/test_gpu_bsa.py (the device): the buried
surface area of deeprank_gnn_amd.interface (drgnn_bsa_residues, csrc/drgnn_bsa.h) against the float64 statement of the
rule in tests/bsa_ref.py, which sees the float32 coordinates the kernel sees.

Hand-made atoms live on the 1/8 A grid, so that grid translations and quarter turns keep the inputs exact in fp32.

TOL, the one tolerance (absolute, A^2) between the kernel and bsa_ref: 4 x the largest deviation measured on an MI355X
over all 496 nodes of the four 1ATN poses (profiles/bsa_ab.txt: MEASURED below, for bsa, sasa_unbound and sasa_complex
alike).  The kernel's arc arithmetic is fp32; the margin covers poses outside the fixture and acos near +-1."""
import os

import numpy as np

import bsa_ref as R
from helpers import GOLDEN

MEASURED = 1.14e-4         # A^2: sasa_complex 1.14e-4, bsa 1.04e-4, sasa_unbound 3.3e-5 (profiles/bsa_ab.txt)
TOL = 4 * MEASURED         # 4.56e-4 A^2
assert TOL <= 1e-2
PROBE = 1.4
RZ = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


# ---- 1ATN ------------------------------------------------------------------------------------------------------------
_ATN = None
_ATN_REF = {}


def atn():
    """dict: table (AtomTable of pose 1w with atom names), xyz float64 [4, T, 3] in the file's atom order, mols, and per
    pose `nodes` (the residue of every fixture node, matched by node_data/pos) and `recorded` (its node_data/bsa)"""
    global _ATN
    if _ATN is None:
        from deeprank_gnn_amd.interface import AtomTable
        with np.load(os.path.join(GOLDEN, "atoms_1ATN.npz")) as z, np.load(os.path.join(GOLDEN, "scores_1ATN.npz")) as s, \
                np.load(os.path.join(GOLDEN, "fixture_1ATN.npz")) as f:
            n = np.diff(z["atom_ptr"])
            chain = np.repeat(np.array(["A", "B"])[z["res_chain"]], n)
            seq = np.repeat(z["res_seq"], n)
            res = np.repeat(z["res_names"][z["res_name_index"]], n)
            names = s["atom_names"][s["pose_name_index"]]
            xyz = z["xyz_milli"] / 1000.0
            mols = [str(m) for m in z["mols"]]
            table = AtomTable(chain, seq, res, xyz[0], atom_name=names)
            nodes, recorded = [], []
            for m, mol in enumerate(mols):
                x = xyz[m][table.order]
                centre = np.add.reduceat(x, table.atom_ptr[:-1], axis=0) / np.diff(table.atom_ptr)[:, None]
                d = np.abs(f[mol + "/node_data/pos"][:, None, :] - centre[None]).max(axis=2)
                assert d.min(axis=1).max() < 1e-4 and len(set(d.argmin(axis=1).tolist())) == d.shape[0]
                nodes.append(d.argmin(axis=1))
                recorded.append(f[mol + "/node_data/bsa"][:, 0].copy())
        _ATN = {"table": table, "xyz": xyz, "mols": mols, "nodes": nodes, "recorded": recorded,
                "per_atom": (chain, seq, res, names)}
    return _ATN


def atn_ref(m, residues, rounded=True):
    """bsa_ref's (sasa_unbound, sasa_complex, bsa) of `residues` of pose m, computed once per request; rounded: on the
    float32 coordinates the kernel sees, else on the file's"""
    a = atn()
    key = (m, tuple(int(r) for r in residues), rounded)
    if key not in _ATN_REF:
        t = a["table"]
        cr, ur = R.radii_of(np.repeat(t.res_name, np.diff(t.atom_ptr)), t.atom_name)
        x = a["xyz"][m][t.order]
        if rounded:
            x = x.astype(np.float32).astype(np.float64)
        _ATN_REF[key] = R.residue_bsa(x, t.atom_ptr, t.split, cr, ur, list(residues), PROBE, 20)
    return _ATN_REF[key]


def emu_subset():
    """12 node residues of pose 1w over both chains: the most negative and the largest recorded values among them"""
    a = atn()
    nodes, rec = a["nodes"][0], a["recorded"][0]
    order = np.argsort(rec)
    pick = list(order[:3]) + list(order[-3:])
    rest = [i for i in range(len(nodes)) if i not in pick]
    pick += rest[::max(1, len(rest) // 6)][:6]
    sub = np.array(sorted(int(nodes[i]) for i in pick))
    t = a["table"]
    assert len(sub) == 12 and (sub < t.split).any() and (sub >= t.split).any() and rec[order[0]] < 0
    return sub


def deviation(got, want):
    """largest |got - want| over (bsa, sasa_unbound, sasa_complex); got as residue_bsa(parts=True) restricted, want as
    bsa_ref's (unbound, complex, bsa)"""
    return max(np.abs(got[0] - want[2]).max(), np.abs(got[1] - want[0]).max(), np.abs(got[2] - want[1]).max())


def check_atn(api, device, poses, subset=None):
    """issue check 2 on 1ATN: the kernel against bsa_ref on the same float32 coordinates.  Returns the deviation"""
    from deeprank_gnn_amd.interface import AtomTable, residue_bsa
    a = atn()
    t = a["table"]
    batch = AtomTable.poses(t, a["xyz"][list(poses)])
    res = [np.asarray(subset if subset is not None else np.sort(a["nodes"][m])) for m in poses]
    got = residue_bsa(batch, residues=res, api=api, device=device, parts=True)
    worst = 0.0
    for k, m in enumerate(poses):
        want = atn_ref(m, res[k])
        assert np.isnan(got[0][k]).sum() == t.n_residues - len(res[k])
        d = deviation([g[k][res[k]] for g in got], want)
        print("pose %s: %d residues, largest |kernel - bsa_ref| = %.3g A^2" % (a["mols"][m], len(res[k]), d))
        worst = max(worst, d)
    print("largest deviation %.3g A^2 (TOL %.3g)" % (worst, TOL))
    assert worst <= TOL
    return worst


# ---- hand-made atoms -------------------------------------------------------------------------------------------------
class Atoms(object):
    """residues [(chain, [(xyz, complex_r, unbound_r), ...]), ...], chain A first; explicit radii"""

    def __init__(self, residues):
        self.xyz = np.array([p for _, atoms in residues for p, _, _ in atoms], dtype=np.float64).reshape(-1, 3)
        self.cr = np.array([c for _, atoms in residues for _, c, _ in atoms], dtype=np.float64)
        self.ur = np.array([u for _, atoms in residues for _, _, u in atoms], dtype=np.float64)
        self.atom_ptr = np.concatenate(([0], np.cumsum([len(atoms) for _, atoms in residues]))).astype(np.int64)
        self.split = sum(1 for c, _ in residues if c == "A")
        assert [c for c, _ in residues] == ["A"] * self.split + ["B"] * (len(residues) - self.split)
        self.n_res = len(residues)

    def run(self, api, device, targets=None, xyz=None, n_slices=20):
        """(out [K,3] sasa_unbound, sasa_complex, bsa; status) of the kernel"""
        from deeprank_gnn_amd.interface import bsa_raw
        targets = np.arange(self.n_res) if targets is None else np.asarray(targets, dtype=np.int64)
        return bsa_raw(api, self.xyz if xyz is None else xyz, self.atom_ptr, [0, self.n_res], [self.split], self.cr, self.ur,
                       targets, np.zeros(len(targets), dtype=np.int64), PROBE, n_slices, device)

    def want(self, targets=None, xyz=None, n_slices=20):
        targets = np.arange(self.n_res) if targets is None else targets
        x = (self.xyz if xyz is None else xyz).astype(np.float32).astype(np.float64)
        cr, ur = self.cr.astype(np.float32).astype(np.float64), self.ur.astype(np.float32).astype(np.float64)
        return np.stack(R.residue_bsa(x, self.atom_ptr, self.split, cr, ur, list(targets), PROBE, n_slices), axis=1)


def one(p, r, chain="A"):
    return (chain, [(p, r, r)])


def sphere(r):
    """4 pi R^2 of an isolated atom (the radius as the float32 the kernel is given)"""
    return 4.0 * np.pi * (float(np.float32(r)) + PROBE) ** 2


def ring(n, radius=3.5, r=0.5):
    ang = 2.0 * np.pi * np.arange(n) / n
    return [((radius * np.cos(a), radius * np.sin(a), 0.0), r, r) for a in ang]


def crowd(seed=5):
    """a chain of one residue (A) facing four residues of chain B, one of them with 70 atoms; atoms on the grid, some
    absent from the complex (radius 0 there, as the hydrogens are)"""
    rng = np.random.default_rng(seed)

    def res(centre, n):
        pts = set()
        while len(pts) < n:
            pts.add(tuple((np.round((np.asarray(centre) + rng.uniform(-3.0, 3.0, 3)) * 8) / 8).tolist()))
        return [(p, float(rng.choice([0.0, 1.42, 1.64, 1.88])), float(rng.choice([1.1, 1.61, 1.8]))) for p in sorted(pts)]

    return Atoms([("A", res((0.0, 0.0, 0.0), 9)), ("B", res((5.0, 0.0, 0.0), 70)), ("B", res((4.0, 4.0, 1.0), 6)),
                  ("B", res((2.0, -4.0, -1.0), 1)), ("B", res((30.0, 0.0, 0.0), 4))])


GRAZE = tuple(float(np.float32(v)) for v in (1.6444417, -3.1301105, -4.7323689))


GRAZE_IN = [tuple(float(np.float32(v)) for v in p) for p in ((0.7982006072998047, -1.4433780908584595, -2.9124019145965576),
                                                             (-2.162132740020752, -1.75696861743927, 2.087636947631836))]


def hand_cases():
    """name -> (Atoms, targets or None, closed forms {(target row, column): value} or None)"""
    big, small = 2.0, 1.0
    cases = {
        "isolated": (Atoms([one((1.0, 2.0, 3.0), 1.6)]), None, {(0, 0): sphere(1.6), (0, 1): sphere(1.6), (0, 2): 0.0}),
        # R = 3.0 and 3.25: the spheres touch at distance 6.25, along x and along z
        "touching_x": (Atoms([one((0.0, 0.0, 0.0), 1.6), one((6.25, 0.0, 0.0), 1.85)]), None,
                       {(0, 0): sphere(1.6), (1, 0): sphere(1.85)}),
        "touching_z": (Atoms([one((0.0, 0.0, 0.0), 1.6), one((0.0, 0.0, 6.25), 1.85)]), None,
                       {(0, 0): sphere(1.6), (1, 0): sphere(1.85)}),
        "half_angstrom": (Atoms([one((0.0, 0.0, 0.0), 1.6), one((0.5, 0.0, 0.0), 1.85)]), None, None),
        "inside": (Atoms([one((0.0, 0.0, 0.0), big), one((0.25, 0.125, 0.0), small)]), None, {(1, 0): 0.0, (1, 1): 0.0}),
        "above_on_z": (Atoms([one((0.0, 0.0, 0.0), 1.6), one((0.0, 0.0, 2.5), 1.85)]), None, None),
        "mirror_pair": (Atoms([one((0.0, 0.0, 0.0), 1.6), one((2.0, 0.0, 1.0), 1.85), one((2.0, 0.0, -1.0), 1.85)]), None, None),
        "same_place": (Atoms([one((0.0, 0.0, 0.0), 1.6), one((2.0, 0.5, 1.0), 1.85), one((2.0, 0.5, 1.0), 1.85),
                              one((2.0, 0.5, 1.0), 1.85)]), None, None),
        "through_pi": (Atoms([one((0.0, 0.0, 0.0), 1.6), one((-2.0, 0.125, 0.0), 1.85), one((-2.0, -0.125, 0.5), 1.2)]), None, None),
        # the neighbour's circle grazes the centre's in one slice: in fp32 the tests of the rule still see an overlap and
        # the cosine rounds to 1, an arc of length 0.  It buries nothing (and must not read as a full turn)
        "grazing": (Atoms([one((0.0, 0.0, 0.0), 1.6), one(GRAZE, 1.85)]), None, None),
        "grazing_third": (Atoms([one((0.0, 0.0, 0.0), 1.6), one(GRAZE, 1.85), one((2.0, 1.0, 0.5), 1.2)]), None, None),
        # the same from inside: the neighbour's circle nearly swallows the centre's, the cosine rounds to -1 in fp32
        "grazing_inside": (Atoms([one((0.0, 0.0, 0.0), 1.6), one(GRAZE_IN[0], 1.85)]), None, None),
        "grazing_inside_2": (Atoms([one((0.0, 0.0, 0.0), 1.6), one(GRAZE_IN[1], 2.4), one((4.0, 1.0, 0.5), 1.2)]), None, None),
        "ring_200": (Atoms([one((0.0, 0.0, 0.0), 1.6), ("A", ring(200))]), [0], None),
        "across_chains": (Atoms([one((0.0, 0.0, 0.0), 1.6), one((2.0, 0.0, 0.0), 1.85, "B")]), None,
                          {(0, 0): sphere(1.6), (1, 0): sphere(1.85)}),
        "crowd": (crowd(), None, None),
    }
    return cases


def check_hand_case(name, api, device):
    atoms, targets, closed = hand_cases()[name]
    out, status = atoms.run(api, device, targets)
    want = atoms.want(targets)
    d = np.abs(out - want).max()
    print("%s: largest |kernel - bsa_ref| = %.3g A^2" % (name, d))
    assert status == 0 and out.shape == want.shape
    assert d <= TOL, (name, out, want)
    for (row, col), v in (closed or {}).items():
        assert abs(out[row, col] - v) <= TOL and abs(want[row, col] - v) <= 1e-9, (name, row, col, out[row, col], v)
    if name == "inside":
        assert out[1, 0] == 0.0 and out[1, 1] == 0.0
    if name == "ring_200":
        assert 0.0 < out[0, 0] < 0.8 * sphere(1.6)
    if name == "across_chains":                                   # the other chain buries in the complex only
        assert out[0, 2] > 1.0 and out[1, 2] > 1.0


def check_capacity(api, device):
    """a centre atom ringed by more neighbours than the documented capacity: refused, never a number"""
    import pytest
    from deeprank_gnn_amd._lib import DrgnnError
    from deeprank_gnn_amd.interface import AtomTable, residue_bsa
    cap = api.bsa_capacity(0)
    assert cap >= 256 and api.bsa_capacity(1) >= cap and api.bsa_capacity(7) == -1
    assert api.bsa_capacity(3) * 1024 < 2 ** 32
    fits = Atoms([one((0.0, 0.0, 0.0), 1.6), ("A", ring(cap))])
    out, status = fits.run(api, device, [0])
    assert status == 0 and abs(out[0, 0] - fits.want([0])[0, 0]) <= TOL
    over = Atoms([one((0.0, 0.0, 0.0), 1.6), ("A", ring(cap + 1)), one((40.0, 0.0, 0.0), 1.6, "B")])
    out, status = over.run(api, device, [0, 2])
    assert status & 1 and np.isnan(out[0]).all()
    assert abs(out[1, 0] - sphere(1.6)) <= TOL                      # the residue that fits keeps its value
    n = over.xyz.shape[0]
    table = AtomTable(np.array(["A"] * (n - 1) + ["B"]), np.array([1] + [2] * (cap + 1) + [3]), np.array(["ALA"] * n), over.xyz)
    with pytest.raises(DrgnnError, match="capacity"):
        residue_bsa(table, residues=[0], radii=(over.cr, over.ur), api=api, device=device)


def check_empty_targets(api, device):
    from deeprank_gnn_amd.interface import AtomTable, residue_bsa
    atoms = hand_cases()["mirror_pair"][0]
    out, status = atoms.run(api, device, [])
    assert out.shape == (0, 3) and status == 0
    n = atoms.xyz.shape[0]
    table = AtomTable(np.array(["A"] * n), np.arange(n), np.array(["ALA"] * n), atoms.xyz)
    got = residue_bsa(table, residues=[], radii=(atoms.cr, atoms.ur), api=api, device=device)
    assert got.shape == (n,) and np.isnan(got).all()
    assert residue_bsa([], api=api, device=device) == []


def check_other_slices(api, device):
    """n_slices is a parameter: 1, 7 and 33 (more than one pass of the kernel's slice chunks)"""
    atoms = hand_cases()["through_pi"][0]
    for n in (1, 7, 33):
        out, status = atoms.run(api, device, n_slices=n)
        assert status == 0 and np.abs(out - atoms.want(n_slices=n)).max() <= TOL, n


# ---- rigid motions (issue check 4) -----------------------------------------------------------------------------------
def check_rigid_motion(api, device):
    atoms = crowd(seed=8)
    base, status = atoms.run(api, device)
    assert status == 0 and np.abs(base - atoms.want()).max() <= TOL
    for moved in (atoms.xyz + (3.0, -2.5, 8.0), atoms.xyz @ RZ.T, atoms.xyz @ (RZ @ RZ).T + (0.0, 16.0, -7.125)):
        out, status = atoms.run(api, device, xyz=moved)             # exact in fp32: translation, quarter turns about z
        assert status == 0 and np.abs(out - base).max() <= TOL
    c, s = np.cos(0.7), np.sin(0.7)
    turned = atoms.xyz @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]).T      # any angle about z
    out, _ = atoms.run(api, device, xyz=turned)
    assert np.abs(out - atoms.want(xyz=turned)).max() <= TOL and np.abs(out - base).max() <= TOL
    # a general rotation is no invariant of a slice method: the kernel and bsa_ref move together
    rot = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    tilted = atoms.xyz @ rot.T
    out, _ = atoms.run(api, device, xyz=tilted)
    want = atoms.want(xyz=tilted)
    assert np.abs(out - want).max() <= TOL
    print("general rotation moves bsa_ref by %.3g A^2" % np.abs(want - atoms.want()).max())


# ---- independence (issue check 5) ------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_independence(api, device, subset, poses=(0, 1, 2)):
    """batch, chunk, pose position and target list change no bit"""
    from deeprank_gnn_amd.interface import AtomTable, residue_bsa
    a = atn()
    t = a["table"]
    sub = np.asarray(subset)
    kw = {"api": api, "device": device, "parts": True}
    full = residue_bsa(AtomTable.poses(t, a["xyz"][list(poses)]), residues=sub, **kw)
    for chunk in (1, 2):
        again = residue_bsa(AtomTable.poses(t, a["xyz"][list(poses)]), residues=sub, chunk=chunk, **kw)
        assert all(same_bits(x[:, sub], y[:, sub]) for x, y in zip(full, again)), chunk
    back = residue_bsa(AtomTable.poses(t, a["xyz"][list(poses)[::-1]]), residues=sub, **kw)
    assert all(same_bits(x[:, sub], y[::-1][:, sub]) for x, y in zip(full, back))
    alone = residue_bsa(AtomTable.poses(t, a["xyz"][[poses[1]]]), residues=sub[3:4], **kw)      # one residue of one pose
    assert all(same_bits(x[1:2, sub[3:4]], y[:, sub[3:4]]) for x, y in zip(full, alone))
    assert np.isnan(alone[0]).sum() == t.n_residues - 1
    # as tables of their own in a ragged batch (per-complex radius tables), each with a target list of its own
    from deeprank_gnn_amd.interface import AtomTable as T
    tables = [T(*a["per_atom"][:3], a["xyz"][m], atom_name=a["per_atom"][3]) for m in poses[:2]]
    ragged = residue_bsa(tables, residues=[sub[:5], sub[2:]], **kw)
    assert all(same_bits(full[j][0][sub[:5]], ragged[0][j][sub[:5]]) and same_bits(full[j][1][sub[2:]], ragged[1][j][sub[2:]])
               for j in range(3))
    return full


def assert_device_equals_emulation(dev, host, sub):
    for x, y in zip(dev, host):
        assert np.abs(x[:, sub] - y[:, sub]).max() <= TOL


# ---- refusals (issue check 6) ----------------------------------------------------------------------------------------
def check_value_errors():
    """the Python side refuses before anything is uploaded (api=object() would fail at the first call)"""
    import pytest
    from deeprank_gnn_amd.interface import AtomTable, interface_graphs, residue_bsa
    chain, seq = np.array(["A", "A", "A", "B", "B"]), np.array([1, 1, 1, 2, 2])
    res, xyz = np.array(["SER"] * 3 + ["GLY"] * 2), np.arange(15, dtype=np.float64).reshape(5, 3)
    names = np.array(["N", "CA", "OG", "N", "HA2"])
    kw = {"api": object(), "device": "cpu"}
    good = AtomTable(chain, seq, res, xyz, atom_name=names)
    with pytest.raises(ValueError, match="atom_name"):
        residue_bsa(AtomTable(chain, seq, res, xyz), **kw)
    with pytest.raises(ValueError, match="atom_name"):
        interface_graphs([AtomTable(chain, seq, res, xyz)], ["x"], bsa=True, **kw)
    with pytest.raises(ValueError, match="CG.*SER"):                 # a heavy atom outside the table
        residue_bsa(AtomTable(chain, seq, res, xyz, atom_name=np.array(["N", "CA", "CG", "N", "HA2"])), **kw)
    with pytest.raises(ValueError, match="starts with 'X'"):        # an unknown first letter (the unbound table)
        residue_bsa(AtomTable(chain, seq, res, xyz, atom_name=np.array(["N", "CA", "OG", "N", "XE"])), **kw)
    with pytest.raises(ValueError, match="non-standard residue HOH"):
        residue_bsa(AtomTable(chain, seq, np.array(["SER"] * 3 + ["HOH"] * 2), xyz, atom_name=names), **kw)
    with pytest.raises(ValueError, match="5 entries"):
        residue_bsa(good, radii=(np.ones(4), np.ones(5)), **kw)
    with pytest.raises(ValueError, match="5 entries"):
        residue_bsa(good, radii=(np.ones(5), np.ones((5, 1))), **kw)
    with pytest.raises(ValueError, match=">= 0"):
        residue_bsa(good, radii=(np.ones(5), np.array([1.0, 1.0, -0.5, 1.0, 1.0])), **kw)
    with pytest.raises(ValueError, match=">= 0"):
        residue_bsa(good, radii=(np.array([1.0, np.nan, 1.0, 1.0, 1.0]), np.ones(5)), **kw)
    with pytest.raises(ValueError, match="n_slices"):
        residue_bsa(good, n_slices=0, **kw)
    with pytest.raises(ValueError, match="probe"):
        residue_bsa(good, probe=-1.0, **kw)
    with pytest.raises(ValueError, match="radii must be"):
        residue_bsa(good, radii="bondi", **kw)
    with pytest.raises(ValueError, match="residue index"):
        residue_bsa(good, residues=[2], **kw)


def check_refusals(api, device):
    """every DRGNN_E_ARG condition of drgnn_bsa_residues is met on the host tables, before a launch: out keeps its fill"""
    import pytest
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._lib import DrgnnError
    atoms = crowd()
    dev = torch.device(device)
    T, Rn = atoms.xyz.shape[0], atoms.n_res
    host = {"atom_ptr": atoms.atom_ptr.astype(np.int32), "res_ptr": np.array([0, Rn], np.int32),
            "res_split": np.array([atoms.split], np.int32), "target_res": np.arange(Rn, dtype=np.int32),
            "target_complex": np.zeros(Rn, np.int32)}
    d = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    d["xyz"] = torch.from_numpy(atoms.xyz.astype(np.float32)).to(dev)
    d["rad_complex"] = torch.from_numpy(atoms.cr.astype(np.float32)).to(dev)
    d["rad_unbound"] = torch.from_numpy(atoms.ur.astype(np.float32)).to(dev)
    out = torch.full((Rn, 3), -7.0, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def request(**over):
        q = _lib.BsaRequest()
        for k in ("xyz", "atom_ptr", "res_ptr", "res_split", "rad_complex", "rad_unbound", "target_res", "target_complex"):
            setattr(q, k, d[k].data_ptr())
        h = {k: np.ascontiguousarray(over.pop("tab_" + k, v), dtype=np.int32) for k, v in host.items()}
        for k in host:
            setattr(q, "host_" + k, h[k].ctypes.data)
        q.n_atoms, q.n_residues, q.n_complexes, q.n_targets, q.n_radii = T, Rn, 1, Rn, T
        q.probe, q.n_slices = PROBE, 20
        q.out, q.status = out.data_ptr(), status.data_ptr()
        for k, v in over.items():
            setattr(q, k, v)
        return q, h

    def put(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    stream = _lib.current_stream(d["xyz"])
    bad = [{k: None} for k in ("xyz", "atom_ptr", "res_ptr", "res_split", "rad_complex", "rad_unbound", "target_res",
                               "target_complex", "host_atom_ptr", "host_res_ptr", "host_res_split", "host_target_res",
                               "host_target_complex", "out", "status")]
    ap = host["atom_ptr"]
    bad += [{"tab_atom_ptr": put(ap, 0, 1)}, {"tab_atom_ptr": put(ap, 2, ap[1] - 1)}, {"tab_atom_ptr": put(ap, Rn, T + 1)},
            {"tab_res_ptr": np.array([1, Rn])}, {"tab_res_ptr": np.array([0, Rn - 1])}, {"tab_res_split": np.array([Rn + 1])},
            {"tab_res_split": np.array([-1])}, {"tab_target_res": put(host["target_res"], 1, Rn)},
            {"tab_target_res": put(host["target_res"], 0, -1)}, {"tab_target_complex": put(host["target_complex"], 2, 1)},
            {"tab_target_complex": put(host["target_complex"], 2, -1)},
            {"n_slices": 0}, {"n_slices": -4}, {"probe": -0.5}, {"probe": float("nan")}, {"n_radii": T - 1}, {"n_radii": 0},
            {"n_targets": -1}, {"n_atoms": -1}]
    for over in bad:
        q, keep = request(**over)
        with pytest.raises(DrgnnError, match="bad argument"):
            api.bsa_residues(q, stream)
    for over in ({"n_slices": api.bsa_capacity(2) + 1}, {"n_targets": api.bsa_capacity(3) + 1}):
        q, keep = request(**over)
        with pytest.raises(DrgnnError, match="capacity"):
            api.bsa_residues(q, stream)
    with pytest.raises(DrgnnError, match="bad argument"):
        _lib._check(api.lib.drgnn_bsa_residues(None, stream), "drgnn_bsa_residues")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((out == -7).all()) and int(status.cpu()[0]) == 0                 # nothing was launched
    q, keep = request()
    api.bsa_residues(q, stream)                                                  # and the good request runs
    assert np.abs(out.cpu().numpy() - atoms.want()).max() <= TOL and int(status.cpu()[0]) == 0


# ---- interface_graphs(bsa=True) (issue check 7) ----------------------------------------------------------------------
def check_graphs(api, device, outdir, nn_kw=None, poses=(0, 1, 2, 3)):
    """node_data/bsa of the graphs built from atoms against the fixture's, node for node; the store without the argument
    is today's; and the way from atoms through PreCluster and the two shipped checkpoints, against the same graphs
    carrying the fixture's recorded bsa (1e-4, the repository's parity bound)."""
    import torch
    from iface_cases import match_by_pos
    from helpers import golden, params_of
    from deeprank_gnn_amd.clustering import PreCluster
    from deeprank_gnn_amd.dataset import GraphDataSet, GraphStore
    from deeprank_gnn_amd.ginet import GINet
    from deeprank_gnn_amd.interface import AtomTable, interface_graphs
    from deeprank_gnn_amd.NeuralNet import NeuralNet
    a = atn()
    t = a["table"]
    mols = [a["mols"][m] for m in poses]
    batch = AtomTable.poses(t, a["xyz"][list(poses)])
    built = interface_graphs(batch, mols, api=api, device=device, bsa=True)
    plain = interface_graphs(batch, mols, api=api, device=device)
    fixture = GraphStore(os.path.join(GOLDEN, "fixture_1ATN.npz"))
    mine, theirs, worst = [], [], 0.0
    for mol in mols:
        assert sorted(built._mols[mol]) == sorted(list(plain._mols[mol]) + ["node_data/bsa"])
        for k in plain._mols[mol]:                                    # without `bsa`: what it is today
            x, y = built.get(mol, k), plain.get(mol, k)
            assert same_bits(x, y), (mol, k)
        bsa = built.get(mol, "node_data/bsa")
        perm = match_by_pos(built.get(mol, "node_data/pos"), fixture.get(mol, "node_data/pos"))
        assert bsa.dtype == np.float64 and bsa.shape == (len(perm), 1) and np.isfinite(bsa).all()
        worst = max(worst, np.abs(bsa[perm] - fixture.get(mol, "node_data/bsa")).max())
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        tree = {k: (v[perm] if k.startswith("node_data/") or k == "nodes" else v) for k, v in built._mols[mol].items()}
        tree["edge_index"] = inv[built.get(mol, "edge_index")]
        tree["internal_edge_index"] = inv[built.get(mol, "internal_edge_index")]
        for k, v in fixture._mols[mol].items():                       # cons, ic, pssm (PSSM files) and the scores
            if (k.startswith("node_data/") and k not in tree) or k.startswith("score/"):
                tree[k] = v
        other = dict(tree)
        other["node_data/bsa"] = fixture.get(mol, "node_data/bsa")
        mine.append(tree)
        theirs.append(other)
    print("largest |node_data/bsa - fixture| = %.3g A^2 (TOL %.3g)" % (worst, TOL))
    assert worst <= TOL
    stores = [GraphStore.from_trees(mols, mine), GraphStore.from_trees(mols, theirs)]
    atoms_only = GraphDataSet(stores[0], node_feature=["type", "polarity", "bsa"], edge_feature=["dist"], target="irmsd")
    PreCluster(atoms_only, method="mcl", api=api, device=device)
    assert atoms_only[0].x.shape == (len(mine[0]["nodes"]), 25)
    assert np.array_equal(atoms_only[0].x[:, 24].numpy(), mine[0]["node_data/bsa"][:, 0].astype(np.float32))
    PreCluster(GraphDataSet(stores[1], node_feature=["type", "polarity", "bsa"], edge_feature=["dist"], target="irmsd"),
               method="mcl", api=api, device=device)
    # the shipped weights fix their own inputs: pretrained_treg reads type, polarity, bsa, charge (from atoms here) and
    # cons, ic, pssm (from the fixture: PSSM files); pretrained_class reads pssm alone
    for name, task, target in (("pretrained_treg.npz", "reg", None), ("pretrained_class.npz", "class", "binclass")):
        g = golden(name)
        feats = [str(f) for f in g["node_feature"]]
        target = target or str(g["target_name"])
        ck = os.path.join(str(outdir), name + ".pth.tar")
        torch.save({'model': params_of(g), 'optimizer': {'state': {}, 'param_groups': [{'lr': 0.001, 'betas': (0.9, 0.999),
                                                                                      'eps': 1e-08, 'weight_decay': 0}]},
                    'node': feats, 'edge': ['dist'], 'target': target, 'task': task, 'classes': [0, 1], 'class_weight': None,
                    'batch_size': 64, 'percent': [1.0, 0.0], 'lr': 0.001, 'index': None, 'shuffle': False,
                    'threshold': 1 if task == 'class' else 0.3, 'cluster_nodes': 'mcl', 'transform_sigmoid': False}, ck)
        outs = []
        for st in stores:
            model = NeuralNet(st, GINet, pretrained_model=ck, outdir=str(outdir), **(nn_kw or {}))
            model.test(hdf5=None)
            outs.append(np.asarray(model.test_out, dtype=np.float64).reshape(len(mols), -1))
        print(name, "from atoms", outs[0].ravel(), "with the recorded bsa", outs[1].ravel())
        assert np.isfinite(outs[0]).all() and np.abs(outs[0] - outs[1]).max() <= 1e-4
