"""Inputs and checks shared by tests/test_lddt.py (host emulation) and tests/test_gpu_lddt.py (the device): the lDDT of
deeprank_gnn_amd.interface (LddtReference, lddt_scores, drgnn_pose_lddt) against the numpy rule of tests/lddt_ref.py.

Everything the kernel gives is an integer and every score one fp64 division, so every check is an equality.  Hand-made
complexes live on the 1/8 A grid (score_cases.py): fp32 holds every coordinate and fp64 every difference, square and sum
exactly, collinear pairs have exact distances, so a pair whose pose distance differs from d_ref by exactly a threshold is a
true tie, and the 90-degree rotations, grid translations and the mirror image keep every d2 bit for bit.

The kernel's shape (csrc/drgnn_lddt.h): a workgroup takes WG_RESIDUES residues, its 16 waves one residue after another, 64
lanes across a residue's entries, 4 entries per lane at a time: a wave's stride is 256 entries, the workgroup's WG_ENTRIES.
Every matched pair is two entries, so an entry total is even: the totals "one below, at and one above" a multiple of
WG_ENTRIES are WG_ENTRIES - 2, WG_ENTRIES and WG_ENTRIES + 2; the lane cases also hold residues of 255, 256, 257 entries."""
import os

import numpy as np

import lddt_ref as R
import score_cases as S
from score_cases import MIRROR, RX, RZ, atoms_of, grid

THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
WG_RESIDUES = 64
WG_ENTRIES = 16 * 4 * 64


class Case(object):
    """A decoy topology with its poses and a reference structure; the package's and the rule's objects, made once"""

    def __init__(self, name, decoy, reference, poses, thresholds=THRESHOLDS):
        self.name, self.thresholds = name, tuple(thresholds)
        self.chain, self.seq, self.res_name, self.atom, base = atoms_of(decoy) if isinstance(decoy, list) else decoy
        self.ref_atoms = atoms_of(reference) if isinstance(reference, list) else reference
        self.poses = [np.asarray(p, dtype=np.float64) for p in poses] if poses is not None else [base]
        self._table = self._lref = self._ref = self._want = None

    @property
    def table(self):
        if self._table is None:
            from deeprank_gnn_amd.interface import AtomTable
            self._table = AtomTable(self.chain, self.seq, self.res_name, self.poses[0], atom_name=self.atom)
        return self._table

    @property
    def lref(self):
        if self._lref is None:
            from deeprank_gnn_amd.interface import LddtReference
            c, s, _, n, x = self.ref_atoms
            self._lref = LddtReference(self.table, c, s, n, x, thresholds=self.thresholds)
        return self._lref

    @property
    def ref(self):
        if self._ref is None:
            c, s, _, n, x = self.ref_atoms
            self._ref = R.Reference(("A", "B"), c, s, n, x, thresholds=self.thresholds)
        return self._ref

    def want(self):
        """lddt_ref's result for every pose, computed once"""
        if self._want is None:
            self._want = [self.ref.score(self.chain, self.seq, self.atom, p.astype(np.float32)) for p in self.poses]
        return self._want

    def keys(self):
        t = self.table
        return [(t.chains[c], int(q)) for c, q in zip(t.res_chain, t.res_seq)]

    def residue(self, chain, seq):
        return self.keys().index((chain, seq))

    def run(self, api, device, poses=None, chunk=None, per_residue=True):
        from deeprank_gnn_amd.interface import AtomTable, lddt_scores
        xyz = np.stack(self.poses if poses is None else poses)
        return lddt_scores(AtomTable.poses(self.table, xyz), self.lref, per_residue=per_residue, device=device, api=api, chunk=chunk)


def assert_reference_equals_rule(case):
    """the once-per-complex half: the denominators and the matching of LddtReference against lddt_ref"""
    L, ref, w = case.lref, case.ref, case.want()[0]
    assert (L.n_pairs, L.n_inter_pairs) == (ref.n_pairs, ref.n_inter_pairs), (L.n_pairs, L.n_inter_pairs, ref.n_pairs, ref.n_inter_pairs)
    assert (L.n_ref_atoms, L.n_matched_atoms, L.n_matched_pairs) == (len(ref.keys), w["n_matched_atoms"], w["n_matched_pairs"])
    assert L.n_pairs_of_residue.tolist() == [ref.residue_pairs.get(k, 0) for k in case.keys()]
    assert L.n_inter_pairs_of_residue.tolist() == [ref.residue_inter_pairs.get(k, 0) for k in case.keys()]
    assert len(L.self_atom) == len(L.other_atom) == len(L.d_ref) == 2 * L.n_matched_pairs == L.entry_ptr[-1]


def assert_equals_rule(case, got, want=None):
    """every count equals lddt_ref's and every score is the fp64 quotient"""
    want = case.want() if want is None else want
    keys, K = case.keys(), len(case.thresholds)
    zero = np.zeros(K, dtype=np.int64)
    M, NR = len(want), len(keys)
    assert got["preserved"].shape == (M, 2, K) and got["preserved"].dtype == np.int64
    assert got["residue_preserved"].shape == (M, NR, 2, K) and got["lddt"].shape == got["ilddt"].shape == (M,)
    pairs = np.array([case.ref.residue_pairs.get(k, 0) for k in keys])
    inter_pairs = np.array([case.ref.residue_inter_pairs.get(k, 0) for k in keys])
    for m, w in enumerate(want):
        assert got["preserved"][m, 0].tolist() == w["all"].tolist(), (m, got["preserved"][m, 0], w["all"])
        assert got["preserved"][m, 1].tolist() == w["inter"].tolist(), (m, got["preserved"][m, 1], w["inter"])
        per = np.array([[w["residue_all"].get(k, zero), w["residue_inter"].get(k, zero)] for k in keys])
        assert np.array_equal(got["residue_preserved"][m], per), (m, np.argwhere(got["residue_preserved"][m] != per)[:4])
        assert got["lddt"][m] == w["lddt"] and got["ilddt"][m] == w["ilddt"], (m, got["lddt"][m], w["lddt"], got["ilddt"][m], w["ilddt"])
        assert got["lddt"][m] == np.float64(int(got["preserved"][m, 0].sum())) / np.float64(K * case.ref.n_pairs)
        assert got["ilddt"][m] == np.float64(int(got["preserved"][m, 1].sum())) / np.float64(K * case.ref.n_inter_pairs)
        for key, c, den in (("residue_lddt", 0, pairs), ("residue_ilddt", 1, inter_pairs)):
            for r in range(NR):
                v = got[key][m, r]
                if den[r] == 0:
                    assert np.isnan(v), (key, m, r, v)
                else:
                    assert v == np.float64(int(per[r, c].sum())) / np.float64(K * int(den[r])), (key, m, r, v)


def assert_invariants(got):
    """what holds for any pose: counts do not decrease with the threshold, the per-residue counts sum to exactly twice
    the global ones, inter <= all"""
    p, rp = got["preserved"], got["residue_preserved"]
    assert np.all(np.diff(p, axis=2) >= 0) and np.all(np.diff(rp, axis=3) >= 0)
    assert np.array_equal(rp.sum(axis=1), 2 * p)
    assert np.all(p[:, 1] <= p[:, 0]) and np.all(rp[:, :, 1] <= rp[:, :, 0]) and np.all(p >= 0)


def assert_bits_equal(a, b, ia=None, ib=None):
    assert sorted(a) == sorted(b)
    for k in a:
        x = a[k] if ia is None else a[k][ia]
        y = b[k] if ib is None else b[k][ib]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


# ---- 1. 1ATN -----------------------------------------------------------------------------------------------------------
_ATN = None


def atn():
    """the four 1ATN poses against the reference structure of scores_1ATN.npz"""
    global _ATN
    if _ATN is None:
        s, _ = S.atn()
        _ATN = Case("1ATN", (s.chain, s.seq, s.res_name, s.atom, s.poses[0]), s.ref_atoms, s.poses)
    return _ATN


def check_atn(api, device):
    case = atn()
    L = case.lref
    assert (L.n_pairs, L.n_inter_pairs, L.n_ref_atoms, L.n_matched_atoms) == (1042401, 41922, 4942, 4915)
    assert_reference_equals_rule(case)
    got = case.run(api, device)
    print("1ATN lddt", got["lddt"], "ilddt", got["ilddt"])
    assert_equals_rule(case, got)
    assert_invariants(got)
    assert np.all(np.abs(got["lddt"] - np.array([0.7808, 0.7878, 0.7879, 0.7915])) < 5e-5)      # (the issue's, for orientation)
    assert 0.042 <= got["ilddt"].min() < 0.043 and 0.089 <= got["ilddt"].max() < 0.090
    return got


# ---- 2. hand-made complexes on the grid --------------------------------------------------------------------------------
STEP = 0.125
GAP = 40.0                          # between the groups along y: no pair across groups


def edge_case(with_unmatched=True):
    """Groups g of a few residues, A 100 + g and B 200 + g, at y = 40 g, each its own little complex; two poses.

      0 - 7    d_ref = 8, the pose distance 8 + t (even g) or 8 - t (odd g) for each threshold t: pose 0 at exactly the
               threshold (preserved from t on), pose 1 one grid step further (preserved only beyond t)
      8        d_ref = 1.5, so d_ref - t < 0 for t = 2, 4: pose 0 has the atoms in one place (preserved at 2 and 4: lo = 0),
               pose 1 at 3.625 (preserved at 4 alone)
      9        d_ref = exactly 15.0: no pair, both residues without a reference pair
      10       d_ref = 14.875: a pair
      11       A 111 has a CB the decoy lacks: in the denominators, never counted (with_unmatched False: the reference
               lacks it too)
      12       the decoy's A 112 has a CG the reference lacks: ignored
      13       hydrogens on both sides, under the names H, HA, 1HB, 2HB: ignored
      14       A 114, A 115 and B 214: an intra-chain pair and two inter-chain ones; the reference's A 199 beside them is not
               in the decoy, the decoy's B 299 (within 8.5 A of A 114: an interface node) not in the reference"""
    ref, decoy, moved = [], [], [{}, {}]

    def both(chain, seq, atoms):
        ref.append((chain, seq, atoms))
        decoy.append((chain, seq, list(atoms)))

    for k, t in enumerate(THRESHOLDS):
        for sign in (1.0, -1.0):
            g = 2 * k + (sign < 0)
            both("A", 100 + g, [("CA", (0.0, GAP * g, 0.0))])
            both("B", 200 + g, [("CA", (8.0, GAP * g, 0.0))])
            moved[0][("B", 200 + g, "CA")] = (8.0 + sign * t, GAP * g, 0.0)
            moved[1][("B", 200 + g, "CA")] = (8.0 + sign * (t + STEP), GAP * g, 0.0)
    y = GAP * 8
    both("A", 108, [("CA", (0.0, y, 0.0))])
    both("B", 208, [("CA", (1.5, y, 0.0))])
    moved[0][("B", 208, "CA")] = (0.0, y, 0.0)
    moved[1][("B", 208, "CA")] = (3.625, y, 0.0)
    both("A", 109, [("CA", (0.0, GAP * 9, 0.0))])
    both("B", 209, [("CA", (15.0, GAP * 9, 0.0))])
    both("A", 110, [("CA", (0.0, GAP * 10, 0.0))])
    both("B", 210, [("CA", (14.875, GAP * 10, 0.0))])
    y = GAP * 11
    ref.append(("A", 111, [("CA", (0.0, y, 0.0))] + ([("CB", (1.0, y, 0.0))] if with_unmatched else [])))
    decoy.append(("A", 111, [("CA", (0.0, y, 0.0))]))
    both("B", 211, [("CA", (8.0, y, 0.0))])
    y = GAP * 12
    ref.append(("A", 112, [("CA", (0.0, y, 0.0))]))
    decoy.append(("A", 112, [("CA", (0.0, y, 0.0)), ("CG", (1.0, y, 1.0))]))
    both("B", 212, [("CA", (8.0, y, 0.0))])
    y = GAP * 13
    ref.append(("A", 113, [("CA", (0.0, y, 0.0)), ("H", (1.0, y, 0.0)), ("1HB", (0.0, y + 1.0, 0.0))]))
    decoy.append(("A", 113, [("H", (1.0, y, 0.5)), ("CA", (0.0, y, 0.0)), ("2HB", (0.0, y - 1.0, 0.0))]))
    ref.append(("B", 213, [("HA", (7.0, y, 0.0)), ("CA", (8.0, y, 0.0))]))
    decoy.append(("B", 213, [("CA", (8.0, y, 0.0)), ("HA", (7.0, y, 1.0))]))
    y = GAP * 14
    both("A", 114, [("CA", (0.0, y, 0.0))])
    both("A", 115, [("CA", (6.0, y, 0.0))])
    both("B", 214, [("CA", (3.0, y, 6.0))])
    ref.append(("A", 199, [("CA", (0.0, y + 5.0, 0.0))]))
    decoy.append(("B", 299, [("CA", (4.0, y, 0.0))]))
    chain, seq, _, atom, base = atoms_of(decoy)
    poses = []
    for fix in moved:
        x = base.copy()
        for i, k in enumerate(zip(chain.tolist(), seq.tolist(), atom.tolist())):
            if k in fix:
                x[i] = fix[k]
        poses.append(x)
    poses[1][(seq == 115)] += (0.0, 0.0, 0.75)                        # (the triangle of group 14 changes in pose 1)
    return Case("edges" if with_unmatched else "edges_without", decoy, ref, poses)


_EDGES = None


def edges():
    global _EDGES
    if _EDGES is None:
        _EDGES = edge_case()
    return _EDGES


def check_edges(api, device):
    case = edges()
    L = case.lref
    assert_reference_equals_rule(case)
    got = case.run(api, device)
    assert_equals_rule(case, got)
    assert_invariants(got)
    K = len(THRESHOLDS)
    rp = got["residue_preserved"]
    for k in range(K):
        for g in (2 * k, 2 * k + 1):
            for key in (("A", 100 + g), ("B", 200 + g)):              # one pair, inter-chain, counted for both residues
                r = case.residue(*key)
                assert L.n_pairs_of_residue[r] == L.n_inter_pairs_of_residue[r] == 1
                assert rp[0, r, 0].tolist() == rp[0, r, 1].tolist() == [int(j >= k) for j in range(K)], (g, rp[0, r])
                assert rp[1, r, 0].tolist() == rp[1, r, 1].tolist() == [int(j > k) for j in range(K)], (g, rp[1, r])
    r = case.residue("B", 208)
    assert rp[0, r, 0].tolist() == [0, 0, 1, 1] and rp[1, r, 0].tolist() == [0, 0, 0, 1]
    for key in (("A", 109), ("B", 209), ("B", 299)):                  # exactly 15.0 A; not in the reference
        r = case.residue(*key)
        assert L.n_pairs_of_residue[r] == 0 and not rp[:, r].any()
        assert np.all(np.isnan(got["residue_lddt"][:, r])) and np.all(np.isnan(got["residue_ilddt"][:, r]))
    r = case.residue("A", 110)
    assert L.n_pairs_of_residue[r] == 1 and rp[0, r, 0].tolist() == [1] * K
    r = case.residue("A", 111)                                         # CB of the reference alone: 2 pairs, 1 matched
    assert L.n_pairs_of_residue[r] == 2 and rp[0, r, 0].tolist() == [1] * K and got["residue_lddt"][0, r] == 0.5
    assert L.n_pairs_of_residue[case.residue("A", 112)] == 1 and L.n_pairs_of_residue[case.residue("A", 113)] == 1
    assert L.n_pairs_of_residue[case.residue("A", 114)] == 3          # A 115, B 214 and the reference's A 199
    assert np.isnan(got["residue_ilddt"][0, case.residue("A", 109)])
    # the unmatched atom: the counts do not change, the denominators do
    other = edge_case(with_unmatched=False)
    assert (other.lref.n_pairs, other.lref.n_inter_pairs) == (L.n_pairs - 1, L.n_inter_pairs - 1)
    assert other.lref.n_matched_pairs == L.n_matched_pairs and other.lref.n_ref_atoms == L.n_ref_atoms - 1
    less = other.run(api, device)
    assert np.array_equal(less["preserved"], got["preserved"]) and np.array_equal(less["residue_preserved"], rp)
    assert np.all(less["lddt"] > got["lddt"])
    return got


def check_edges_node_data(api, device):
    """the residue without a reference pair is an interface node: NaN per residue, 0 in node_data/lddt"""
    from deeprank_gnn_amd.interface import AtomTable, interface_graphs
    case = edges()
    got = case.run(api, device)
    names = ["pose0", "pose1"]
    store = interface_graphs(AtomTable.poses(case.table, np.stack(case.poses)), names, api=api, device=device, lddt=case.lref)
    r = case.residue("B", 299)
    for m, mol in enumerate(names):
        nodes = store.get(mol, "node_data/residue")
        per = got["residue_lddt"][m]
        assert r in nodes.tolist() and np.isnan(per[r])
        want = np.where(np.isnan(per), 0.0, per)[nodes]
        have = store.get(mol, "node_data/lddt")
        assert have.dtype == np.float64 and have.shape == (len(nodes),) and have.tobytes() == want.tobytes()
        assert have[nodes.tolist().index(r)] == 0.0
        assert store.get(mol, "score/lddt")[()] == got["lddt"][m] and store.get(mol, "score/ilddt")[()] == got["ilddt"][m]


# ---- 3. lane and stride edges ------------------------------------------------------------------------------------------
def star_case(name, sizes, thresholds=THRESHOLDS, n_poses=3, seed=0):
    """Group g: A 100 + g with one atom and B 200 + g with sizes[g] atoms within 15 A of it (0: no B residue), groups 40 A
    apart: both residues own sizes[g] entries.  Poses: the reference itself, then every atom moved by up to 0.5 A per axis
    on the grid."""
    rng = np.random.default_rng(seed)
    res = []
    for g, n in enumerate(sizes):
        res.append(("A", 100 + g, [("CA", (0.0, GAP * g, 0.0))]))
        pts = set()
        while len(pts) < n:
            pts.add(tuple(grid(np.array([7.0, GAP * g, 0.0]) + rng.uniform(-2.0, 2.0, 3)).tolist()))
        if n:
            res.append(("B", 200 + g, [("X%03d" % k, p) for k, p in enumerate(sorted(pts))]))
    base = atoms_of(res)[4]
    poses = [base] + [base + rng.integers(-4, 5, base.shape) / 8.0 for _ in range(n_poses - 1)]
    return Case(name, res, res, poses, thresholds)


LANE_SIZES = (0, 1, 63, 64, 65, 129)
WIDE = (255, 256, 257, 129, 65, 64, 63, 1, 0)                          # 1 090 pairs
STARS = {
    "lanes": (LANE_SIZES, THRESHOLDS),
    "entries_4094": (WIDE + (479, 478), THRESHOLDS),
    "entries_4096": (WIDE + (479, 479), THRESHOLDS),
    "entries_4098": (WIDE + (479, 480), THRESHOLDS),
    "residues_63": ((2,) * 31 + (0,), THRESHOLDS),
    "residues_64": ((2,) * 32, THRESHOLDS),
    "residues_65": ((2,) * 32 + (0,), THRESHOLDS),
    "residues_129": ((3,) * 64 + (0,), THRESHOLDS),
    "one_residue_per_chain": ((5,), THRESHOLDS),
    "one_threshold": (LANE_SIZES, (1.0,)),
    "eight_thresholds": (LANE_SIZES, (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)),
}
_STAR = {}


def star(name):
    if name not in _STAR:
        _STAR[name] = star_case(name, *STARS[name])
    return _STAR[name]


def check_star(name, api, device):
    case = star(name)
    sizes = STARS[name][0]
    L = case.lref
    owned = np.diff(L.entry_ptr).tolist()
    assert sorted(owned) == sorted([n for n in sizes for _ in range(2 if n else 1)]), owned
    assert L.entry_ptr[-1] == 2 * sum(sizes) and case.table.n_residues == len(owned)
    if name.startswith("entries_"):
        assert L.entry_ptr[-1] == int(name[8:]) and abs(L.entry_ptr[-1] - WG_ENTRIES) <= 2 and {255, 256, 257} <= set(owned)
    if name.startswith("residues_"):
        assert case.table.n_residues == int(name[9:])
    if name == "one_residue_per_chain":
        assert case.table.n_residues == 2 and case.table.split == 1
    assert_reference_equals_rule(case)
    got = case.run(api, device)
    assert_equals_rule(case, got)
    assert_invariants(got)
    K = len(case.thresholds)
    assert got["preserved"][0, 0].tolist() == [L.n_pairs] * K and got["lddt"][0] == 1.0      # (the reference itself)
    assert 0 < got["preserved"][1, 0, 0] < L.n_pairs or L.n_pairs < 8                        # (the moved poses lose pairs)
    return got


# ---- 4. invariants -----------------------------------------------------------------------------------------------------
_RIGID = None


def rigid_case():
    """score_cases' plain complex as the reference; the decoy lacks four of its atoms.  Pose 0: the matched reference
    coordinates; pose 1: every atom moved by up to 0.5 A per axis on the grid"""
    global _RIGID
    if _RIGID is None:
        ref = S.plain_complex(seed=9)
        decoy = [(c, s, atoms[:-1] if s in (12, 14, 22, 24) else atoms) for c, s, atoms in ref]
        base = atoms_of(decoy)[4]
        rng = np.random.default_rng(4)
        _RIGID = Case("rigid", decoy, ref, [base, base + rng.integers(-4, 5, base.shape) / 8.0])
    return _RIGID


def check_rigid_motion(api, device):
    case = rigid_case()
    L = case.lref
    K = len(case.thresholds)
    assert 0 < L.n_matched_pairs < L.n_pairs and 0 < L.n_inter_pairs < L.n_pairs
    got = case.run(api, device)
    assert_equals_rule(case, got)
    assert_invariants(got)
    assert got["preserved"][0, 0].tolist() == [L.n_matched_pairs] * K
    assert got["lddt"][0] == L.n_matched_pairs / L.n_pairs
    assert 0 < got["preserved"][1, 0, 0] < got["preserved"][1, 0, K - 1] <= L.n_matched_pairs
    x = case.poses[1]
    moved = [x @ RZ.T + (3.0, -2.5, 8.0), x @ RX.T @ RZ.T + (-16.0, 4.125, 0.5), x @ (RZ @ RZ).T + (0.0, 0.0, -7.0),
             x + (100.0, -50.0, 25.0), x @ MIRROR.T, x @ MIRROR.T @ RX.T + (1.0, 2.0, 3.0)]
    again = case.run(api, device, moved)
    for m in range(len(moved)):
        assert_bits_equal(got, again, ia=slice(1, 2), ib=slice(m, m + 1))
    return got


# ---- 5. independence ---------------------------------------------------------------------------------------------------
_BATCH = None


def batch_case():
    """seven poses (not a multiple of the poses of a pass) of the lane complex"""
    global _BATCH
    if _BATCH is None:
        _BATCH = star_case("batch", LANE_SIZES, n_poses=7, seed=5)
    return _BATCH


def check_independence(api, device):
    from deeprank_gnn_amd.interface import lddt_raw
    case = batch_case()
    batch = case.run(api, device)
    assert_equals_rule(case, batch)
    assert_bits_equal(batch, case.run(api, device))                    # two runs
    for chunk in (1, 3, 4, 7):
        assert_bits_equal(batch, case.run(api, device, chunk=chunk))
    order = np.random.default_rng(0).permutation(7)
    assert_bits_equal(batch, case.run(api, device, [case.poses[k] for k in order]), ia=order)
    for m in (0, 3, 6):
        assert_bits_equal(batch, case.run(api, device, [case.poses[m]]), ia=slice(m, m + 1))
    assert_bits_equal(batch, case.run(api, device, case.poses[2:]), ia=slice(2, 7))
    L, t = case.lref, case.table
    xyz = np.stack(case.poses).astype(np.float32)[:, t.order]
    for pp in (0, 1, 4):                                               # the poses that share a pass change nothing
        counts, per = lddt_raw(api, xyz, L.entry_ptr, L.self_atom, L.other_atom, L.d_ref, L.n_chain_a_atoms, L.thresholds,
                               residue_counts=True, device=device, poses_per_pass=pp)
        assert np.array_equal(counts, batch["preserved"]) and np.array_equal(per, batch["residue_preserved"]), pp
    counts, per = lddt_raw(api, xyz, L.entry_ptr, L.self_atom, L.other_atom, L.d_ref, L.n_chain_a_atoms, L.thresholds, device=device)
    assert per is None and np.array_equal(counts, batch["preserved"])  # (without the optional output)
    return batch


def device_cases():
    """the cases whose bits the device is held to the emulation's on"""
    return [atn(), edges(), rigid_case(), batch_case()] + [star(n) for n in sorted(STARS)]


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def check_refusals(api, device):
    """every DRGNN_E_ARG and DRGNN_E_CAPACITY condition of drgnn_pose_lddt, checked on the host tables before a launch: the
    outputs keep their fill"""
    import pytest
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._lib import DrgnnError
    case = star("lanes")
    L, t = case.lref, case.table
    dev = torch.device(device)
    K, R, T, E = len(case.thresholds), t.n_residues, t.n_atoms, len(L.self_atom)
    host = {"entry_ptr": L.entry_ptr.copy(), "self_atom": L.self_atom.copy(), "other_atom": L.other_atom.copy()}
    d = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    d["d_ref"] = torch.from_numpy(L.d_ref).to(dev)
    d["xyz"] = torch.from_numpy(t.xyz[None].copy()).to(dev)
    out = {"counts": torch.full((1, 2, K), -7, dtype=torch.int32, device=dev),
           "residue_counts": torch.full((1, R, 2, K), -7, dtype=torch.int32, device=dev)}

    def request(**over):
        q = _lib.LddtRequest()
        for k in ("xyz", "entry_ptr", "self_atom", "other_atom", "d_ref"):
            setattr(q, k, d[k].data_ptr())
        h = {k: np.ascontiguousarray(over.pop("tab_" + k, v), dtype=np.int32) for k, v in host.items()}
        q.host_entry_ptr, q.host_self_atom, q.host_other_atom = (h[k].ctypes.data for k in ("entry_ptr", "self_atom", "other_atom"))
        q.n_poses, q.n_atoms, q.n_residues, q.n_entries, q.n_chain_a_atoms = 1, T, R, E, L.n_chain_a_atoms
        q.thresholds = type(q.thresholds)(*over.pop("thr", case.thresholds))
        q.n_thresholds, q.poses_per_pass = K, 0
        q.counts, q.residue_counts = out["counts"].data_ptr(), out["residue_counts"].data_ptr()
        for k, v in over.items():
            setattr(q, k, v)
        return q, h

    def put(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    stream = _lib.current_stream(d["xyz"])
    ep, sa, oa = host["entry_ptr"], host["self_atom"], host["other_atom"]
    bad = [dict([(k, None)]) for k in ("xyz", "entry_ptr", "self_atom", "other_atom", "d_ref", "host_entry_ptr", "host_self_atom",
                                       "host_other_atom", "counts")]
    bad += [{"tab_entry_ptr": put(ep, 0, 1)}, {"tab_entry_ptr": put(ep, 3, ep[2] - 1)}, {"tab_entry_ptr": put(ep, R, E - 1)},
            {"n_entries": E - 2}, {"tab_self_atom": put(sa, 0, -1)}, {"tab_self_atom": put(sa, E - 1, T)},
            {"tab_other_atom": put(oa, 5, -1)}, {"tab_other_atom": put(oa, E - 1, T)},
            {"n_thresholds": 0}, {"n_thresholds": 9}, {"n_thresholds": -1},
            {"thr": (-0.5, 1.0, 2.0, 4.0)}, {"thr": (0.5, 0.5, 2.0, 4.0)}, {"thr": (0.5, 2.0, 1.0, 4.0)}, {"thr": (0.5, 1.0, 2.0, float("nan"))},
            {"n_poses": -1}, {"n_atoms": 0}, {"n_residues": 0}, {"n_entries": -1}, {"n_chain_a_atoms": -1}, {"n_chain_a_atoms": T + 1},
            {"poses_per_pass": 2}]
    for over in bad:
        q, keep = request(**over)
        with pytest.raises(DrgnnError, match="bad argument"):
            api.pose_lddt(q, stream)
    with pytest.raises(DrgnnError, match="bad argument"):
        _lib._check(api.lib.drgnn_pose_lddt(None, stream), "drgnn_pose_lddt")
    for over in ({"n_poses": 2 ** 31}, {"n_atoms": (2 ** 31 - 1) // 3 + 1}, {"n_entries": 2 ** 31}):
        q, keep = request(**over)
        with pytest.raises(DrgnnError, match="capacity"):
            api.pose_lddt(q, stream)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in out.values())            # nothing was launched
    q, keep = request()
    api.pose_lddt(q, stream)                                           # and the good request runs
    assert out["counts"].cpu()[0, 0].tolist() == [L.n_pairs] * K
    assert int(out["residue_counts"].cpu().sum()) == 2 * int(out["counts"].cpu().sum())


def check_value_errors():
    import pytest
    from deeprank_gnn_amd.interface import AtomTable, LddtReference, interface_graphs, lddt_scores
    case = rigid_case()
    c, s, _, n, x = case.ref_atoms
    bare = AtomTable(case.chain, case.seq, case.res_name, case.poses[0])
    with pytest.raises(ValueError, match="atom_name"):
        LddtReference(bare, c, s, n, x)
    apart = x * 1000.0                                                 # every atom beyond 15 A of every other residue
    with pytest.raises(ValueError, match="no atom pair"):
        LddtReference(case.table, c, s, n, apart)
    far = x + np.where(c == "B", 100.0, 0.0)[:, None]
    with pytest.raises(ValueError, match="no inter-chain atom pair"):
        LddtReference(case.table, c, s, n, far)
    for thresholds in ((), (0.5,) * 2, (1.0, 0.5), (-1.0, 1.0), tuple(range(1, 10))):
        with pytest.raises(ValueError, match="thresholds"):
            LddtReference(case.table, c, s, n, x, thresholds=thresholds)
    other = AtomTable(case.chain, case.seq, case.res_name, case.poses[0], atom_name=case.atom)
    with pytest.raises(ValueError, match="reference's AtomTable"):
        lddt_scores(other, case.lref, api=object(), device="cpu")
    with pytest.raises(ValueError, match="reference's AtomTable"):
        interface_graphs([other], ["x"], api=object(), device="cpu", lddt=case.lref)


# ---- 7. binding --------------------------------------------------------------------------------------------------------
def check_binding(api):
    """the second table's entries meet what test_every_registered_entry_point_is_a_method_of_api asks of the first, and the
    record has the header's fields in the header's order"""
    import ctypes
    import re
    from deeprank_gnn_amd import _lib
    from helpers import ROOT
    assert ("pose_lddt", "drgnn_pose_lddt", _lib.LddtRequest) in _lib.REQUEST_CALLS_2
    assert not {n for n, _, _ in _lib.REQUEST_CALLS} & {n for n, _, _ in _lib.REQUEST_CALLS_2}
    for name, symbol, record in _lib.REQUEST_CALLS_2:
        assert callable(vars(_lib.Api)[name]) and vars(_lib.Api)[name].__code__.co_varnames[:3] == ("self", "request", "stream")
        assert issubclass(record, ctypes.Structure)
        assert getattr(api.lib, symbol).argtypes == [ctypes.POINTER(record), ctypes.c_void_p]
    assert api.lib.drgnn_abi_version() == 5
    text = open(os.path.join(ROOT, "include", "drgnn.h")).read()
    body = re.search(r"typedef struct drgnn_lddt_request \{(.*?)\} drgnn_lddt_request;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        fields += [re.sub(r"\[\d+\]", "", n).strip(" *") for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip()).split(",") if n.strip()]
    assert fields == [n for n, _ in _lib.LddtRequest._fields_], fields
    assert ctypes.sizeof(_lib.LddtRequest) == 8 * 8 + 5 * 8 + 8 * 8 + 2 * 4 + 2 * 8


# ---- 8. end to end -----------------------------------------------------------------------------------------------------
def check_end_to_end(api, device):
    from deeprank_gnn_amd.dataset import GraphDataSet
    from deeprank_gnn_amd.interface import AtomTable, attach_scores, interface_graphs, lddt_scores
    case = atn()
    _, record = S.atn()
    mols = record["mols"]
    poses = AtomTable.poses(case.table, np.stack(case.poses))
    store = interface_graphs(poses, mols, api=api, device=device, lddt=case.lref)
    plain = interface_graphs(poses, mols, api=api, device=device)
    scores = lddt_scores(poses, case.lref, per_residue=True, api=api, device=device)
    for m, mol in enumerate(mols):
        assert sorted(store._mols[mol]) == sorted(list(plain._mols[mol]) + ["score/lddt", "score/ilddt", "node_data/lddt"])
        for k in plain._mols[mol]:                                     # without `lddt`: what it is today
            assert store.get(mol, k).tobytes() == plain.get(mol, k).tobytes(), (mol, k)
        for k in ("lddt", "ilddt"):
            v = store.get(mol, "score/" + k)
            assert v.shape == () and v.dtype == np.float64 and v[()] == scores[k][m], (mol, k)
        nodes = store.get(mol, "node_data/residue")
        per = scores["residue_lddt"][m]
        assert store.get(mol, "node_data/lddt").tobytes() == np.where(np.isnan(per), 0.0, per)[nodes].tobytes()
    again = attach_scores(interface_graphs(poses, mols, api=api, device=device), mols, scores)
    for mol in mols:
        assert again.get(mol, "score/lddt")[()] == store.get(mol, "score/lddt")[()]
        assert not again.has(mol, "score/residue_lddt") and not again.has(mol, "score/preserved")
    ds = GraphDataSet(store, node_feature=["type", "polarity", "charge", "lddt"], edge_feature=["dist"], target="lddt")
    y = np.array([float(ds[m].y) for m in range(4)])
    assert np.array_equal(y, scores["lddt"].astype(np.float32).astype(np.float64))
    assert ds[0].x.shape[1] == 20 + 4 + 1 + 1
