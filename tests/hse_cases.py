"""Inputs and checks shared by tests/test_hse.py (host emulation) and tests/test_gpu_hse.py (the device): the half-sphere
exposure of deeprank_gnn_amd.interface (drgnn_hse_residues, csrc/drgnn_hse.h) against the float64 statement of the rule
in tests/hse_ref.py, which sees the float32 coordinates the kernel sees.

Counts and NaN rows are held to exact equality: every decision of the kernel is fp64 on fp32 coordinates, and the
1ATN inputs are asserted to stay MIN_MARGIN away from any tie.  Hand-made atoms live on the 1/8 A grid with CA - CA
steps of 3.75 A, so that fp32 and fp64 agree exactly and grid translations and quarter turns keep the inputs exact.

TOL, the one tolerance (absolute, rad) of the angle between the kernel and hse_ref: 4 x the largest deviation measured
on an MI355X over all 2508 residues of the four 1ATN poses (profiles/hse_ab.txt: MEASURED below)."""
import os

import numpy as np

import hse_ref as R
from bsa_cases import atn, same_bits
from helpers import GOLDEN

MEASURED = 2.22e-16        # rad: one unit in the last place of an angle in [1, 2) (profiles/hse_ab.txt)
TOL = 4 * MEASURED
assert TOL <= 1e-6
MIN_MARGIN = 1e-6          # A: hse_ref's smallest margin over the 1ATN inputs must stay above this (measured: 2.8e-5, pose 2w)
RZ = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
RX = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])


# ---- 1ATN ------------------------------------------------------------------------------------------------------------
_REF = {}


def atn_bb():
    t = atn()["table"]
    return R.table_of(t.res_name, t.res_chain, t.atom_ptr, t.atom_name)


def atn_ref(m, rounded=True, **opt):
    """hse_ref's (rows [627,3], margin [627]) of pose m, computed once per request; rounded: on the float32 coordinates
    the kernel sees, else on the file's"""
    key = (m, rounded, tuple(sorted(opt.items())))
    if key not in _REF:
        a = atn()
        t = a["table"]
        x = a["xyz"][m][t.order]
        if rounded:
            x = x.astype(np.float32).astype(np.float64)
        _REF[key] = R.residue_hse(x, t.atom_ptr, atn_bb(), **opt)
    return _REF[key]


def recorded():
    """per pose the fixture's node_data/hse, rows in the order of atn()["nodes"]"""
    a = atn()
    with np.load(os.path.join(GOLDEN, "fixture_1ATN.npz")) as f:
        return [f[mol + "/node_data/hse"].copy() for mol in a["mols"]]


def check_ref_against_recorded(connect):
    """issue check 1: hse_ref on the float32-rounded coordinates against the 496 recorded rows"""
    a = atn()
    t = a["table"]
    rec = recorded()
    assert sum(len(r) for r in rec) == 496
    worst = 0.0
    for m, mol in enumerate(a["mols"]):
        nodes = a["nodes"][m]
        rows = atn_ref(m, connect=connect)[0][nodes]
        rows = np.where(np.isnan(rows[:, :1]), 0.0, rows)              # the reference writes (0, 0, 0) for no value
        assert np.array_equal(rows[:, :2], rec[m][:, :2]), mol
        err = np.abs(rows[:, 2] - rec[m][:, 2]).max()
        zero = sorted((int(t.res_chain[r]), int(t.res_seq[r])) for r in nodes[(rec[m] == 0.0).all(axis=1)])
        print("%s (%s): %d nodes, counts equal, max |angle - recorded| = %.3g rad, zero rows %s" % (mol, connect, len(nodes), err, zero))
        assert zero == ([(1, 1), (1, 260)] if m < 3 else [(1, 260)])   # B1 in 1w - 3w, B260 in all four
        worst = max(worst, err)
    assert worst <= 1e-9


def equal_rows(got, want, what=""):
    """NaN rows and counts exactly, the angle within TOL (a NaN angle: in both).  Returns the largest angle deviation"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.flatnonzero(np.isnan(got).any(1) != np.isnan(want).any(1)))
    has = ~np.isnan(want[:, 0])
    assert np.array_equal(got[has, :2], want[has, :2]), (what, np.flatnonzero((got[:, :2] != want[:, :2]).any(axis=1) & has))
    fin = ~np.isnan(want[:, 2])
    dev = float(np.abs(got[fin, 2] - want[fin, 2]).max()) if fin.any() else 0.0
    assert dev <= TOL, (what, dev)
    return dev


def check_atn(api, device, poses=(0, 1, 2, 3), **opt):
    """issue check 2: the kernel against hse_ref on all 627 residues of the poses, no residue left out"""
    from deeprank_gnn_amd.interface import AtomTable, residue_hse
    a = atn()
    t = a["table"]
    got = residue_hse(AtomTable.poses(t, a["xyz"][list(poses)]), api=api, device=device, **opt)
    assert got.shape == (len(poses), 627, 3) and got.dtype == np.float64
    worst, margin = 0.0, np.inf
    for k, m in enumerate(poses):
        want, mar = atn_ref(m, **opt)
        margin = min(margin, mar.min())
        dev = equal_rows(got[k], want, a["mols"][m])
        print("pose %s %s: %d of 627 residues with a value, counts equal, largest |angle - hse_ref| = %.3g rad, margin %.3g A"
              % (a["mols"][m], opt, (~np.isnan(want[:, 0])).sum(), dev, mar.min()))
        worst = max(worst, dev)
    print("largest angle deviation %.3g rad (TOL %.3g), smallest margin %.3g A" % (worst, TOL, margin))
    assert margin >= MIN_MARGIN
    return worst


# ---- hand-made atoms -------------------------------------------------------------------------------------------------
OFF = {"N": (-0.5, 0.25, 0.125), "C": (0.5, 0.25, -0.125), "CB": (0.0, 0.75, 0.5)}      # about the CA; C(r) - N(r+1) > 1.8 A
V = [(2.25, -3.0, 0.0), (0.0, 0.0, 0.0), (-2.25, -3.0, 0.0)]                            # b of the middle one: exactly (0, 1, 0)


def res(ca, chain="A", name="ALA", without=(), **off):
    """one residue: its CA, then N, C, CB at OFF (or the offsets given as N=, C=, CB=) unless left out"""
    ca = np.asarray(ca, dtype=np.float64)
    atoms = [("CA", ca)] + [(k, ca + np.asarray(off.get(k, OFF[k]))) for k in ("N", "C", "CB")
                            if k not in without and not (name == "GLY" and k == "CB" and "CB" not in off)]
    return (chain, name, atoms)


def zigzag(n, x0=0.0, chain="A", **kw):
    """n residues with CA - CA steps of exactly 3.75 A"""
    return [res((x0 + 2.25 * i, 3.0 * (i % 2), 0.0), chain, **kw) for i in range(n)]


class Chains(object):
    """residues [(chain, res_name, [(atom name, xyz), ...]), ...], chain A first"""

    def __init__(self, residues):
        self.n_res = len(residues)
        self.chain = np.array([c for c, _, atoms in residues for _ in atoms])
        self.seq = np.array([i + 1 for i, (_, _, atoms) in enumerate(residues) for _ in atoms])
        self.res_name = np.array([n for _, n, atoms in residues for _ in atoms])
        self.atom_name = np.array([a for _, _, atoms in residues for a, _ in atoms])
        self.xyz = np.array([p for _, _, atoms in residues for _, p in atoms], dtype=np.float64).reshape(-1, 3)
        assert np.array_equal(self.xyz * 8, np.round(self.xyz * 8))                 # on the 1/8 A grid

    def table(self, xyz=None):
        from deeprank_gnn_amd.interface import AtomTable
        return AtomTable(self.chain, self.seq, self.res_name, self.xyz if xyz is None else xyz, atom_name=self.atom_name)

    def run(self, api, device, xyz=None, residues=None, **opt):
        from deeprank_gnn_amd.interface import residue_hse
        return residue_hse(self.table(xyz), residues=residues, api=api, device=device, **opt)

    def want(self, xyz=None, **opt):
        t = self.table(xyz)
        bb = R.table_of(t.res_name, t.res_chain, t.atom_ptr, t.atom_name)
        return R.residue_hse(t.xyz.astype(np.float64), t.atom_ptr, bb, **opt)[0]


ANGLE_CB = float(np.arccos(0.75 / np.sqrt(0.75 * 0.75 + 0.5 * 0.5)))                    # between OFF["CB"] and (0, 1, 0)
NAN = float("nan")


def hand_cases():
    """name -> (Chains, options, {residue: row or None (no value)}): the rows the rule gives by hand"""
    a3 = [res(p) for p in V]
    pair = [res((3.75, 0.0, 0.0), "B"), res((3.75, 0.125, 0.0), "B")]
    turn = [res((0.0, 4.0, 0.0), "B"), res((0.0, 4.0, 3.75), "B")]
    cases = {
        # a 3-residue peptide opposite a 2-residue chain: only the middle residue has a value; the two of the chain have
        # none but are counted, the one at d.b = 0 down, the one 1/8 A above the plane up
        "three_opposite_two": (Chains(a3 + pair), {}, {0: None, 1: (1, 3, ANGLE_CB), 2: None, 3: None, 4: None}),
        # a residue with no link on either side (5 A from the centre, the last of chain A): no value, counted by nobody
        "unlinked_is_invisible": (Chains(a3 + [res((0.0, 5.0, 0.0))] + pair), {}, {1: (1, 3, ANGLE_CB), 3: None}),
        # a gap of 4.5 A after the third residue: both sides have no value and are still counted
        "gap_in_mid_chain": (Chains(zigzag(3) + zigzag(3, x0=9.0)), {},
                             {0: None, 1: (0, 5, ANGLE_CB), 2: None, 3: None, 4: (0, 5, ANGLE_CB), 5: None}),
        # exactly 12.0 A away: not counted; 11.875 A: counted
        "radius_edge": (Chains(a3 + [res((0.0, 12.0, 0.0), "B"), res((0.0, 11.875, 0.0), "B")]), {}, {1: (1, 2, ANGLE_CB)}),
        # a CA at the centre's own position goes down
        "same_place": (Chains(a3 + [res((0.0, 0.0, 0.0), "B"), res((0.0, 0.125, 0.0), "B")]), {}, {1: (1, 3, ANGLE_CB)}),
        # three collinear CAs: b is the zero vector, everything goes down and the angle is undefined
        "collinear": (Chains([res((-3.75, 0.0, 0.0)), res((0.0, 0.0, 0.0)), res((3.75, 0.0, 0.0))] + turn), {},
                      {0: None, 1: (0, 4, NAN), 2: None}),
        "gly_with_n_and_c": (Chains([res(V[0]), res(V[1], name="GLY"), res(V[2])] + turn), {}, {}),
        "gly_without_n": (Chains([res(V[0]), res(V[1], name="GLY", without=("N",)), res(V[2])] + turn), {}, {1: (2, 2, 0.0)}),
        "no_cb": (Chains([res(V[0]), res(V[1], without=("CB",)), res(V[2])] + turn), {}, {1: (2, 2, 0.0)}),
        # a residue name outside the 20 in mid-chain breaks the peptide and is not counted
        "nonstandard_breaks": (Chains(zigzag(3) + [res((6.75, 3.0, 0.0), name="MSE")] + zigzag(3, x0=9.0)), {},
                               {0: None, 2: None, 3: None, 4: None, 6: None}),
        "offset_1": (Chains(a3 + pair), {"offset": 1}, {1: (1, 1, ANGLE_CB)}),
        "offset_1_radius_8": (Chains(zigzag(9) + zigzag(4, x0=1.0, chain="B", CB=(0.0, -0.75, 0.5))), {"offset": 1, "radius": 8.0}, {}),
        "offset_3_radius_8": (Chains(zigzag(9) + zigzag(4, x0=1.0, chain="B")), {"offset": 3, "radius": 8.0}, {}),
        # CA - CA 3.75 A but C - N 2.76 A: one peptide by CA, no link at all by C - N
        "cn_unlinked": (Chains(a3 + pair), {"connect": "CN"}, {k: None for k in range(5)}),
        # C - N 1.25 A along the trace: linked both ways
        "cn_linked": (Chains([res((3.75 * i, 0.0, 0.0) if i != 2 else (7.5, 0.125, 0.0), N=(-1.25, 0.0, 0.0), C=(1.25, 0.0, 0.0))
                              for i in range(5)] + turn), {"connect": "CN"}, {0: None, 4: None}),
        # HSExposureCB: every member with a CB has a value, the first residue of a peptide too; the angle is 0
        "cb_direction": (Chains(a3 + pair), {"direction": "CB"},
                         {0: (3, 1, 0.0), 1: (1, 3, 0.0), 2: (3, 1, 0.0), 3: (1, 3, 0.0), 4: (0, 4, 0.0)}),
        "cb_direction_gly": (Chains([res(V[0]), res(V[1], name="GLY"), res(V[2], without=("CB",))] + turn), {"direction": "CB"},
                             {2: None}),
    }
    return cases


def check_hand_case(name, api, device):
    atoms, opt, rows = hand_cases()[name]
    got, want = atoms.run(api, device, **opt), atoms.want(**opt)
    print(name, "\n", got)
    equal_rows(got, want, name)
    for r, row in rows.items():
        if row is None:
            assert np.isnan(want[r]).all() and np.isnan(got[r]).all(), (name, r)
        else:
            assert np.array_equal(want[r, :2], row[:2]) and np.array_equal(got[r, :2], row[:2]), (name, r, got[r], row)
            if np.isnan(row[2]):
                assert np.isnan(want[r, 2]) and np.isnan(got[r, 2])
            else:
                assert abs(want[r, 2] - row[2]) <= 1e-15 and abs(got[r, 2] - row[2]) <= TOL, (name, r, got[r], row)
    if name == "gly_with_n_and_c":
        assert np.array_equal(got[1, :2], (2, 2)) and 0.1 < got[1, 2] < 3.0
    if name == "cb_direction_gly":
        assert not np.isnan(got[1]).any() and got[1, 2] == 0.0
    if name == "cn_linked":
        assert not np.isnan(got[1:4]).any() and np.isnan(atoms.run(api, device, connect="CN", residues=[0])[0]).all()
    if name == "cn_unlinked":
        assert not np.isnan(atoms.run(api, device)[1]).any()


# ---- rigid motions (issue check 4) -----------------------------------------------------------------------------------
def check_rigid_motion(api, device):
    atoms = Chains(zigzag(9) + zigzag(4, x0=1.0, chain="B") + [res((5.0, 6.0, 1.0), "B", name="GLY")])
    for opt in ({}, {"direction": "CB"}, {"offset": 1, "radius": 8.0}):
        base = atoms.run(api, device, **opt)
        equal_rows(base, atoms.want(**opt), "base")
        assert (~np.isnan(base[:, 0])).sum() >= 9
        for moved in (atoms.xyz + (3.0, -2.5, 8.0), atoms.xyz @ RZ.T, atoms.xyz @ (RX @ RZ).T + (0.0, 16.0, -7.125),
                      atoms.xyz @ (RZ @ RZ @ RX).T - (100.0, 0.125, 64.0)):
            out = atoms.run(api, device, xyz=moved, **opt)          # exact in fp32: grid translations, quarter turns
            equal_rows(out, base, "moved")


# ---- independence (issue check 5) ------------------------------------------------------------------------------------
def check_independence(api, device, poses=(0, 1, 2)):
    """batch, chunk, tile, pose position and target list change no bit.  Returns the batch's result"""
    from deeprank_gnn_amd.interface import AtomTable, hse_raw, hse_table, residue_hse, _ragged
    a = atn()
    t = a["table"]
    kw = {"api": api, "device": device}
    xyz = a["xyz"][list(poses)]
    full = residue_hse(AtomTable.poses(t, xyz), **kw)
    for m in range(len(poses)):
        assert same_bits(full[m], residue_hse(AtomTable.poses(t, xyz[m:m + 1]), **kw)[0]), m      # each pose alone
    assert same_bits(full, residue_hse(AtomTable.poses(t, xyz), chunk=1, **kw))
    assert same_bits(full, residue_hse(AtomTable.poses(t, xyz), chunk=2, **kw))
    back = residue_hse(AtomTable.poses(t, xyz[::-1]), **kw)                                     # another batch position
    assert same_bits(full, back[::-1])
    rng = np.random.default_rng(3)
    sub = np.sort(rng.choice(t.n_residues, 40, replace=False))
    part = residue_hse(AtomTable.poses(t, xyz), residues=sub, **kw)                             # a subset of the targets
    assert same_bits(full[:, sub], part[:, sub]) and np.isnan(part).all(axis=2).sum() == len(poses) * (t.n_residues - 40)
    # one call with the targets of all poses shuffled together, and with other tile sizes
    part_list = [(t, x) for x in AtomTable.poses(t, xyz).xyz]
    x, atom_ptr, res_ptr = _ragged(part_list)[:3]
    tgt = rng.permutation(len(poses) * t.n_residues)
    for tile in (None, 1, 7, 64, 1000):
        out, status = hse_raw(api, x, atom_ptr, res_ptr, hse_table(t), tgt, tgt // t.n_residues, device=device, tile=tile)
        assert status == 0 and same_bits(full.reshape(-1, 3)[tgt], out), tile
    # as tables of their own in a ragged batch, each with a target list of its own
    tables = [AtomTable(*a["per_atom"][:3], a["xyz"][m], atom_name=a["per_atom"][3]) for m in poses[:2]]
    ragged = residue_hse(tables, residues=[sub[:5], sub[2:]], **kw)
    assert same_bits(full[0][sub[:5]], ragged[0][sub[:5]]) and same_bits(full[1][sub[2:]], ragged[1][sub[2:]])
    return full


def assert_device_equals_emulation(dev, host):
    for x, y in zip(dev, host):
        equal_rows(x, y, "device against emulation")


# ---- empty target list (issue check 6) -------------------------------------------------------------------------------
def check_empty_targets(api, device):
    from deeprank_gnn_amd.interface import hse_raw, hse_table, residue_hse
    atoms = hand_cases()["three_opposite_two"][0]
    t = atoms.table()
    out, status = hse_raw(api, t.xyz, t.atom_ptr, [0, t.n_residues], hse_table(t), [], [], device=device)
    assert out.shape == (0, 3) and status == 0
    got = atoms.run(api, device, residues=[])
    assert got.shape == (5, 3) and np.isnan(got).all()
    assert residue_hse([], api=api, device=device) == []


# ---- capacity (issue check 7) ----------------------------------------------------------------------------------------
def line_table(n, chains=("A",)):
    """n CA-only ALA residues on a zigzag with steps of 3.75 A"""
    from deeprank_gnn_amd.interface import AtomTable
    i = np.arange(n)
    xyz = np.stack((2.25 * i, 3.0 * (i % 2), np.zeros(n)), axis=1)
    return AtomTable(np.array(["A"] * n), i + 1, np.array(["ALA"] * n), xyz, atom_name=np.array(["CA"] * n))


def check_capacity(api, device):
    """a complex one residue beyond the documented capacity is refused, never a number; at the capacity it is served"""
    import pytest
    from deeprank_gnn_amd._lib import DrgnnError
    from deeprank_gnn_amd.interface import hse_raw, hse_table, residue_hse, _ragged
    cap = api.hse_capacity(0)
    assert cap >= 4096 and api.hse_capacity(1) * 1024 < 2 ** 32 and api.hse_capacity(7) == -1
    fits, over = line_table(cap), line_table(cap + 1)
    got = residue_hse(fits, api=api, device=device)
    want = R.residue_hse(fits.xyz.astype(np.float64), fits.atom_ptr, hse_table(fits))[0]
    equal_rows(got, want, "at the capacity")
    assert (~np.isnan(got[:, 0])).sum() == cap - 2 and got[cap // 2, 0] + got[cap // 2, 1] == 10
    with pytest.raises(DrgnnError, match="capacity"):
        residue_hse(over, api=api, device=device)
    with pytest.raises(DrgnnError, match="capacity"):
        residue_hse(over, residues=[5], api=api, device=device)
    # in one batch with a complex that fits: NaN rows for the one refused, the other keeps its values
    x, atom_ptr, res_ptr = _ragged([(over, over.xyz), (fits, fits.xyz)])[:3]
    tgt = np.array([0, 7, cap, cap + 1 + 7, cap + 1 + 8, 8])
    cx = np.array([0, 0, 0, 1, 1, 0])
    out, status = hse_raw(api, x, atom_ptr, res_ptr, np.concatenate([hse_table(over), hse_table(fits)]), tgt, cx, device=device)
    assert status & 1 and np.isnan(out[[0, 1, 2, 5]]).all()
    assert same_bits(out[3:5], got[7:9])


# ---- refusals (issue check 8) ----------------------------------------------------------------------------------------
def check_value_errors():
    """the Python side refuses before anything is uploaded (api=object() would fail at the first call)"""
    import pytest
    from deeprank_gnn_amd.interface import AtomTable, hse_table, interface_graphs, residue_hse
    atoms = hand_cases()["three_opposite_two"][0]
    kw = {"api": object(), "device": "cpu"}
    good = atoms.table()
    bare = AtomTable(atoms.chain, atoms.seq, atoms.res_name, atoms.xyz)
    with pytest.raises(ValueError, match="atom_name"):
        hse_table(bare)
    with pytest.raises(ValueError, match="atom_name"):
        residue_hse(bare, **kw)
    with pytest.raises(ValueError, match="atom_name"):
        interface_graphs([bare], ["x"], hse=True, **kw)
    with pytest.raises(ValueError, match="connect"):
        residue_hse(good, connect="CC", **kw)
    with pytest.raises(ValueError, match="direction"):
        residue_hse(good, direction="N", **kw)
    with pytest.raises(ValueError, match="direction"):
        interface_graphs([good], ["x"], hse={"direction": "up"}, **kw)
    with pytest.raises(ValueError, match="residue index"):
        residue_hse(good, residues=[5], **kw)
    with pytest.raises(ValueError, match="residue index"):
        residue_hse(good, residues=[-1], **kw)
    with pytest.raises(ValueError, match="radius"):
        residue_hse(good, radius=0.0, **kw)
    with pytest.raises(ValueError, match="radius"):
        residue_hse(good, radius=float("nan"), **kw)
    with pytest.raises(ValueError, match="offset"):
        residue_hse(good, offset=-1, **kw)
    with pytest.raises(ValueError, match="offset"):
        residue_hse(good, offset=0.5, **kw)


REQUEST_TABLES = ("atom_ptr", "res_ptr", "bb", "target_res", "target_complex", "tile_ptr")


def refusal_cases():
    """name -> what to change in a good request over the case "offset_1_radius_8" (13 residues, two tiles)"""
    atoms = hand_cases()["offset_1_radius_8"][0]
    t = atoms.table()
    Rn, T = t.n_residues, t.n_atoms
    ap = t.atom_ptr.astype(np.int32)
    bb = R.table_of(t.res_name, t.res_chain, t.atom_ptr, t.atom_name)
    tgt = np.arange(Rn, dtype=np.int32)

    def put(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    cases = {"null " + k: {k: None} for k in ("xyz",) + REQUEST_TABLES + tuple("host_" + k for k in REQUEST_TABLES) + ("out", "status")}
    cases.update({
        "atom_ptr starts at 1": {"tab_atom_ptr": put(ap, 0, 1)}, "atom_ptr decreases": {"tab_atom_ptr": put(ap, 2, ap[1] - 1)},
        "atom_ptr ends past the atoms": {"tab_atom_ptr": put(ap, Rn, T + 1)},
        "res_ptr starts at 1": {"tab_res_ptr": np.array([1, Rn])}, "res_ptr ends early": {"tab_res_ptr": np.array([0, Rn - 1])},
        "target past its complex": {"tab_target_res": put(tgt, 1, Rn)}, "target below its complex": {"tab_target_res": put(tgt, 0, -1)},
        "target complex past the batch": {"tab_target_complex": put(np.zeros(Rn, np.int32), 2, 1)},
        "target complex negative": {"tab_target_complex": put(np.zeros(Rn, np.int32), 2, -1)},
        "tile_ptr starts at 1": {"tab_tile_ptr": np.array([1, 8, Rn])}, "tile_ptr decreases": {"tab_tile_ptr": np.array([0, 14, Rn])},
        "tile_ptr ends early": {"tab_tile_ptr": np.array([0, 8, Rn - 1])},
        "bb offset past its residue": {"tab_bb": put(bb, (3, 1), 4)}, "bb offset below -1": {"tab_bb": put(bb, (0, 3), -2)},
        "radius 0": {"radius": 0.0}, "radius negative": {"radius": -12.0}, "radius NaN": {"radius": float("nan")},
        "offset negative": {"offset": -1}, "cutoff 0": {"connect_cutoff": 0.0},
        "connect column 4": {"connect_a": 4}, "connect column -1": {"connect_b": -1}, "connect column flags": {"connect_b": 5},
        "direction 2": {"direction": 2}, "direction -1": {"direction": -1},
        "n_rows 0": {"n_rows": 0}, "n_rows does not divide": {"n_rows": Rn - 1}, "n_targets negative": {"n_targets": -1},
        "n_atoms negative": {"n_atoms": -1}, "n_tiles 0": {"n_tiles": 0}, "n_tiles negative": {"n_tiles": -1},
    })
    return atoms, cases


def check_refusal(api, device, name):
    """one malformed field: refused on the host tables, before a launch (out keeps its fill); the good request runs.
    `name`: a key of refusal_cases(), "two complexes in a tile", "capacity" or "null request\""""
    import pytest
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._lib import DrgnnError
    atoms, cases = refusal_cases()
    t = atoms.table()
    dev = torch.device(device)
    two = name == "two complexes in a tile"
    M = 2 if two else 1
    Rn, T = t.n_residues * M, t.n_atoms * M
    bb = R.table_of(t.res_name, t.res_chain, t.atom_ptr, t.atom_name)
    host = {"atom_ptr": np.concatenate([t.atom_ptr[:-1] + m * t.n_atoms for m in range(M)] + [[T]]).astype(np.int32),
            "res_ptr": (t.n_residues * np.arange(M + 1)).astype(np.int32), "bb": bb,
            "target_res": np.arange(Rn, dtype=np.int32), "target_complex": np.repeat(np.arange(M), t.n_residues).astype(np.int32),
            "tile_ptr": np.array([0, 8, Rn], np.int32)}
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host.items()}
    d["xyz"] = torch.from_numpy(np.tile(t.xyz, (M, 1))).to(dev)
    out = torch.full((Rn, 3), -7.0, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def request(**over):
        q = _lib.HseRequest()
        for k in ("xyz",) + REQUEST_TABLES:
            setattr(q, k, d[k].data_ptr())
        h = {k: np.ascontiguousarray(over.pop("tab_" + k, v), dtype=np.int32) for k, v in host.items()}
        for k in host:
            setattr(q, "host_" + k, h[k].ctypes.data)
        q.n_atoms, q.n_residues, q.n_complexes, q.n_targets, q.n_tiles, q.n_rows = T, Rn, M, Rn, 2, t.n_residues
        q.radius, q.offset, q.connect_a, q.connect_b, q.connect_cutoff, q.direction = 8.0, 1, 1, 1, 4.3, 0
        q.out, q.status = out.data_ptr(), status.data_ptr()
        for k, v in over.items():
            setattr(q, k, v)
        return q, h

    stream = _lib.current_stream(d["xyz"])
    if name == "capacity":
        q, keep = request(n_tiles=api.hse_capacity(1) + 1)
        with pytest.raises(DrgnnError, match="capacity"):
            api.hse_residues(q, stream)
    elif name == "null request":
        with pytest.raises(DrgnnError, match="bad argument"):
            _lib._check(api.lib.drgnn_hse_residues(None, stream), "drgnn_hse_residues")
    else:
        q, keep = request(**({} if two else dict(cases[name])))       # two complexes: the first tile ends inside the first
        with pytest.raises(DrgnnError, match="bad argument"):         # complex, the second runs over both
            api.hse_residues(q, stream)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((out == -7).all()) and int(status.cpu()[0]) == 0                 # nothing was launched
    if two:
        host["tile_ptr"] = np.array([0, t.n_residues, Rn], np.int32)
        d["tile_ptr"] = torch.from_numpy(host["tile_ptr"]).to(dev)
    q, keep = request()
    api.hse_residues(q, stream)                                                  # and the good request runs
    want = atoms.want(offset=1, radius=8.0)
    equal_rows(out.cpu().numpy(), np.tile(want, (M, 1)), "the good request")
    assert int(status.cpu()[0]) == 0


def refusal_names():
    return sorted(refusal_cases()[1]) + ["two complexes in a tile", "capacity", "null request"]


# ---- interface_graphs(hse=True) (issue check 9) ----------------------------------------------------------------------
def check_graphs(api, device, poses=(0, 1, 2, 3)):
    """node_data/hse of the graphs built from atoms against the fixture's, node for node; every other key is what the
    store without the argument holds; with bsa=True too both are there; GraphDataSet stacks the three columns"""
    from iface_cases import match_by_pos
    from deeprank_gnn_amd.dataset import GraphDataSet, GraphStore
    from deeprank_gnn_amd.interface import AtomTable, interface_graphs
    a = atn()
    t = a["table"]
    mols = [a["mols"][m] for m in poses]
    batch = AtomTable.poses(t, a["xyz"][list(poses)])
    built = interface_graphs(batch, mols, api=api, device=device, hse=True)
    plain = interface_graphs(batch, mols, api=api, device=device)
    both = interface_graphs(AtomTable.poses(t, a["xyz"][[poses[0]]]), mols[:1], api=api, device=device, bsa=True,
                            hse={"radius": 12.0, "connect": "CA"})
    only_bsa = interface_graphs(AtomTable.poses(t, a["xyz"][[poses[0]]]), mols[:1], api=api, device=device, bsa=True)
    fixture = GraphStore(os.path.join(GOLDEN, "fixture_1ATN.npz"))
    worst = 0.0
    for mol in mols:
        assert sorted(built._mols[mol]) == sorted(list(plain._mols[mol]) + ["node_data/hse"])
        for k in plain._mols[mol]:                                    # without `hse`: what it is today
            assert same_bits(built.get(mol, k), plain.get(mol, k)), (mol, k)
        hse = built.get(mol, "node_data/hse")
        perm = match_by_pos(built.get(mol, "node_data/pos"), fixture.get(mol, "node_data/pos"))
        want = fixture.get(mol, "node_data/hse")
        assert hse.dtype == np.float64 and hse.shape == (len(perm), 3) and np.isfinite(hse).all()
        assert np.array_equal(hse[perm][:, :2], want[:, :2]), mol
        worst = max(worst, np.abs(hse[perm][:, 2] - want[:, 2]).max())
    print("largest |angle of node_data/hse - fixture| = %.3g rad (bound 1e-5)" % worst)
    assert worst <= 1e-5
    mol = mols[0]
    assert sorted(both._mols[mol]) == sorted(list(plain._mols[mol]) + ["node_data/bsa", "node_data/hse"])
    assert same_bits(both.get(mol, "node_data/hse"), built.get(mol, "node_data/hse"))
    assert same_bits(both.get(mol, "node_data/bsa"), only_bsa.get(mol, "node_data/bsa"))
    ds = GraphDataSet(both, node_feature=["type", "polarity", "bsa", "hse"], edge_feature=["dist"])
    x = ds[0].x.numpy()
    assert x.shape == (both.get(mol, "node_data/pos").shape[0], 28)
    assert np.array_equal(x[:, 25:], both.get(mol, "node_data/hse").astype(np.float32))
