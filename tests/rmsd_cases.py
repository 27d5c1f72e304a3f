"""Inputs and checks shared by tests/test_rmsd.py (host emulation) and tests/test_gpu_rmsd.py (the device): the pose-by-pose
RMSD matrix and RMSD clustering of deeprank_gnn_amd.interface (drgnn_pose_rmsd / drgnn_pose_cluster_dist,
csrc/drgnn_rmsd.h) against the numpy statement of the rules in tests/rmsd_ref.py, which sees the float32 coordinates
the kernels see.

Tolerance.  SQUARED RMSD is compared: the cancellation A_i + A_j - 2 sum R o C of the moment form costs an absolute
error in A^2 whatever the RMSD, which a square root would turn into ~3e-6 A on a diagonal.  The bound of a pair is
    TOL_K * 2^-52 * (A_i + A_j) / nR,     A = sum |x|^2 of the rms atoms about the fit centroid,
with TOL_K = 16 * K_MEASURED, and K_MEASURED the smallest k under which the two statements of the rule in rmsd_ref, (a)
explicit Kabsch and (b) the moment form with LAPACK's eigenvectors, agree on every input of this file (`measure_k`:
measured on the CPU from the reference alone, never from the kernels; test_the_two_forms_of_the_rule_agree recomputes
it).  The factor 16 covers Jacobi against LAPACK and the order of the sums.  Without fit there is no cancellation: the
bound is nR * 2^-52 relative.  The clustering is compared by exact equality, on the same matrix.

Hand-made atoms live on the 1/8 A grid: translations and quarter turns keep them exact."""
import numpy as np

import fcc_cases as F
import rmsd_ref as R
from bsa_cases import atn, same_bits
from fcc_cases import NoLaunch, kw
from hse_cases import RZ, Chains

K_MEASURED = 8.7           # measured: 8.70 (1ATN, kind "ligand"); the 130-pose family 7.50, 1ATN "interface" 6.55, the hand-made sets <= 2.2
TOL_K = 16 * K_MEASURED    # 139.2
EPS = 2.0 ** -52
STAGE = 32                 # RM_K of drgnn_rmsd.h: atoms staged at a time
BATCH_SIZES = (1, 2, 17, 33, 65)
CUTOFF, MIN_SIZE = 3.0, 4  # of the end-to-end clustering of the 130-pose family (kind "ligand")
_CACHE = {}


def once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- inputs ------------------------------------------------------------------------------------------------------------
def atn_poses():
    from deeprank_gnn_amd.interface import AtomTable
    a = atn()
    return a["table"], AtomTable.poses(a["table"], a["xyz"])


def atn_interface():
    """the residues in contact (heavy atoms, 5 A) in at least one of the four poses, by fcc_ref"""
    maps = F.atn_maps(True)
    t = atn()["table"]
    return np.concatenate((np.flatnonzero(maps.any(axis=(0, 2))), t.split + np.flatnonzero(maps.any(axis=(0, 1))))).astype(np.int64)


def family(M=130):
    from deeprank_gnn_amd.interface import AtomTable
    table, xyz = F.family_batch()
    return table, AtomTable.poses(table, xyz[:M])


def ref_lists(table, kind, residues=None):
    rms, fit = R.kind_lists(kind, table.atom_name, table.res_chain, table.atom_ptr, residues)
    return rms, fit


BASE_A = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, 3.0)]            # a chiral four-atom set
BASE_B = [(5.0, 1.0, 0.0), (6.0, 1.0, 1.0), (5.0, 3.0, 0.125), (7.0, 0.0, 2.0)]


def hand():
    """(table, Poses): 0 the base, 1 translated by (3, 4, 0), 2 a quarter turn and a translation, 3 chain B alone
    translated by (3, 4, 0), 4 the mirror image"""
    def make():
        from deeprank_gnn_amd.interface import AtomTable
        atoms = Chains([F.atoms_of(c, [("CA", np.array(p))]) for c, pts in (("A", BASE_A), ("B", BASE_B)) for p in pts])
        x = atoms.xyz
        isb = atoms.chain == "B"
        xyz = np.stack([x, x + (3.0, 4.0, 0.0), x @ RZ.T + (1.0, -2.0, 0.5), x + np.where(isb[:, None], (3.0, 4.0, 0.0), 0.0),
                        x * (-1.0, 1.0, 1.0)])
        t = atoms.table()
        return t, AtomTable.poses(t, xyz)
    return once("hand", make)


HAND_LISTS = {                                                         # name -> (rms, fit)
    "all": (np.arange(8), np.arange(8)),
    "ligand": (np.arange(4, 8), np.arange(4)),
    "fixed": (np.arange(4, 8), None),
    "chiral": (np.arange(4), np.arange(4)),
    "nF_3": (np.arange(4, 8), np.arange(3)),
    "nR_1": (np.array([6]), np.arange(4)),
    "nR_1_fixed": (np.array([6]), None),
}


def stage_lists(table, n):
    bb = R.select(table.atom_name, table.res_chain, table.atom_ptr)
    return bb[-n:], bb[:n]                                             # (rms, fit)


def inputs():
    """name -> (xyz float32 [M, T, 3], rms, fit): every input the kernels are compared on"""
    out = {}
    t, p = atn_poses()
    for kind in ("ligand", "interface", "fixed", "all"):
        out["1ATN " + kind] = (p.xyz,) + ref_lists(t, kind, atn_interface() if kind == "interface" else None)
    t, p = hand()
    for name, (rms, fit) in HAND_LISTS.items():
        if name != "nR_1_fixed":                                       # (one atom, no fit: held to its exact answers, check_hand)
            out["hand " + name] = (p.xyz, rms, fit)
    t, p = family(6)
    for n in (STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 1):
        out["stage %d" % n] = (p.xyz,) + stage_lists(t, n)
    t, p = family(65)
    out["family 65"] = (p.xyz,) + ref_lists(t, "ligand")
    t, p = family(130)
    out["family 130"] = (p.xyz,) + ref_lists(t, "ligand")
    return out


def ref_sq(name):
    """rmsd_ref (a) on an input, once: (sum of squares [M, M], A_i + A_j [M, M])"""
    return once(("ref", name), lambda: R.matrix_sq(*inputs()[name]))


def bound_sq(name):
    """the bound on D^2 of every pair of an input"""
    xyz, rms, fit = inputs()[name]
    sq, scale = ref_sq(name)
    return (len(rms) * EPS * sq if fit is None else TOL_K * EPS * scale) / len(rms)


def measure_k():
    """name -> the smallest k under which (a) and (b) agree on that input"""
    out = {}
    for name, (xyz, rms, fit) in inputs().items():
        if fit is None:
            continue
        sq, scale = ref_sq(name)
        mom = R.matrix_sq(xyz, rms, fit, form="moments")[0]
        off = ~np.eye(len(xyz), dtype=bool)
        out[name] = float((np.abs(sq - mom)[off] / (EPS * scale[off])).max()) if off.any() else 0.0
    return out


def check_forms_agree():
    k = measure_k()
    print("smallest k per input:", {n: round(v, 2) for n, v in k.items()})
    assert max(k.values()) <= 2 * K_MEASURED, k                        # (another LAPACK may round otherwise: a factor 2, far inside the 16)
    assert TOL_K == 16 * K_MEASURED


def assert_matrix(got, name, what=""):
    """a device-made square matrix against (a): dtype, exact symmetry, zero diagonal, the bound on D^2"""
    d = got.cpu().numpy()
    sq, _ = ref_sq(name)
    nR = len(inputs()[name][1])
    assert got.dtype.is_floating_point and d.dtype == np.float64 and d.shape == sq.shape, (name, what)
    assert np.array_equal(d, d.T) and not np.diag(d).any() and np.isfinite(d).all(), (name, what)
    dev = np.abs(d * d - sq / nR)
    bound = bound_sq(name)
    worst = np.unravel_index(np.argmax(dev / np.where(bound > 0, bound, 1.0)), dev.shape)
    print("%s%s: largest |D^2 - ref| %.3g A^2; closest to its bound %.3g A^2 of %.3g" % (name, what, dev.max(), dev[worst], bound[worst]))
    assert (dev <= bound).all(), (name, what, worst, dev[worst], bound[worst])
    return d


# ---- 1 values ----------------------------------------------------------------------------------------------------------
def check_atn(api, device):
    from deeprank_gnn_amd.interface import pose_rmsd, select_atoms
    t, p = atn_poses()
    for kind in ("ligand", "interface", "fixed", "all"):
        res = atn_interface() if kind == "interface" else None
        d = assert_matrix(pose_rmsd(p, kind=kind, residues=res, **kw(api, device)), "1ATN " + kind)
        rms, fit = ref_lists(t, kind, res)
        again = pose_rmsd(p, rms=rms, fit=fit, **kw(api, device))      # the same lists given explicitly
        assert same_bits(again.cpu().numpy(), d)
        assert d[np.triu_indices(4, 1)].min() > 0.5                    # four different poses
    assert np.array_equal(select_atoms(t), R.select(t.atom_name, t.res_chain, t.atom_ptr))
    assert np.array_equal(select_atoms(t, names=None, chain=1), np.arange(t.atom_ptr[t.split], t.n_atoms))
    assert np.array_equal(select_atoms(t, names=("CA",), chain=0, residues=[2, 5]),
                          R.select(t.atom_name, t.res_chain, t.atom_ptr, names=("CA",), chain=0, residues=[2, 5]))
    assert select_atoms(t).dtype == np.int32


def check_hand(api, device):
    from deeprank_gnn_amd.interface import pose_rmsd
    t, p = hand()
    d = {}
    for name, (rms, fit) in HAND_LISTS.items():
        got = pose_rmsd(p, rms=rms, fit=fit, **kw(api, device))
        d[name] = assert_matrix(got, "hand " + name) if name != "nR_1_fixed" else got.cpu().numpy()
    one = d["nR_1_fixed"]                                              # |x_i[6] - x_j[6]|: 5 A or nothing where the answer is a float64
    assert np.array_equal(one, one.T) and not np.diag(one).any() and one[1, 3] == 0.0 and one[0, 4] == 10.0
    # the shorthand kinds on this table: equal residue counts, so the first chain is the one fitted on
    for kind in ("all", "ligand", "fixed"):
        assert same_bits(pose_rmsd(p, kind=kind, **kw(api, device)).cpu().numpy(), d[kind])
    tol = lambda name, i, j: bound_sq("hand " + name)[i, j]
    # a translation and a quarter turn of the whole complex: 0 under a fit, the known distance without one
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert d["all"][i, j] ** 2 <= tol("all", i, j) and d["ligand"][i, j] ** 2 <= tol("ligand", i, j)
    assert d["fixed"][0, 1] == 5.0 and d["fixed"][0, 3] == 5.0 and d["nR_1_fixed"][0, 1] == 5.0
    x = p.xyz.astype(np.float64)
    turned = ((x[0, 4:] - x[2, 4:]) ** 2).sum() / 4.0                  # exact: grid coordinates
    assert turned > 1.0 and abs(d["fixed"][0, 2] ** 2 - turned) <= 4 * EPS * turned
    # chain B alone moved by 5 A: the fit on chain A is the identity
    assert abs(d["ligand"][0, 3] ** 2 - 25.0) <= tol("ligand", 0, 3) and abs(d["nF_3"][0, 3] ** 2 - 25.0) <= tol("nF_3", 0, 3)
    assert abs(d["nR_1"][0, 3] ** 2 - 25.0) <= tol("nR_1", 0, 3)
    # the mirror image: a reflection would give 0, the proper rotation does not
    want = ref_sq("hand chiral")[0][0, 4] / 4.0
    assert want > 0.25 and abs(d["chiral"][0, 4] ** 2 - want) <= tol("chiral", 0, 4)


def check_stage_sizes(api, device):
    from deeprank_gnn_amd.interface import pose_rmsd
    t, p = family(6)
    for n in (STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 1):
        rms, fit = stage_lists(t, n)
        assert len(rms) == len(fit) == n
        assert_matrix(pose_rmsd(p, rms=rms, fit=fit, **kw(api, device)), "stage %d" % n)


def family_matrix(api, device):
    """pose_rmsd(kind="ligand") of the first 65 poses of the family, once per library"""
    from deeprank_gnn_amd.interface import pose_rmsd
    return once(("family", id(api), device), lambda: pose_rmsd(family(65)[1], kind="ligand", **kw(api, device)))


def check_batch(api, device, M):
    """the first M poses: against (a), and bit for bit the block of the 65-pose matrix"""
    from deeprank_gnn_amd.interface import AtomTable, pose_rmsd
    full = family_matrix(api, device).cpu().numpy()
    if M == 65:
        assert_matrix(family_matrix(api, device), "family 65")
    t, p = family(M)
    got = pose_rmsd(p, kind="ligand", **kw(api, device)).cpu().numpy()
    assert same_bits(got, np.ascontiguousarray(full[:M, :M])), M
    assert np.array_equal(got, got.T) and not np.diag(got).any()


# ---- 2 invariance ------------------------------------------------------------------------------------------------------
def check_independence(api, device, M=17):
    """blocks (other=), chunk, place, permutation and run change no bit"""
    from deeprank_gnn_amd.interface import AtomTable, pose_rmsd
    t, p = family(M)
    full = np.ascontiguousarray(family_matrix(api, device).cpu().numpy()[:M, :M])
    run = lambda x, **o: pose_rmsd(x, kind="ligand", table=t, **dict(kw(api, device), **o)).cpu().numpy()
    assert same_bits(run(p.xyz), full) and same_bits(run(p.xyz), full)                 # two runs
    for chunk in (1, 5, 16, M):
        assert same_bits(run(p.xyz, chunk=chunk), full), chunk
    lo, hi = p.xyz[:6], p.xyz[6:]
    assert same_bits(run(lo, other=hi), np.ascontiguousarray(full[:6, 6:]))
    assert same_bits(run(hi, other=lo), np.ascontiguousarray(full[6:, :6]))            # below the diagonal: the reversed pairs
    assert same_bits(run(hi, other=p.xyz), np.ascontiguousarray(full[6:]))
    assert same_bits(run(hi, other=p.xyz, chunk=4), np.ascontiguousarray(full[6:]))
    assert same_bits(run(p.xyz[[11, 3]]), np.ascontiguousarray(full[[11, 3]][:, [11, 3]]))
    perm = np.random.default_rng(5).permutation(M)
    assert same_bits(run(p.xyz[perm]), np.ascontiguousarray(full[perm][:, perm]))
    for kind, o in (("fixed", {}), ("interface", {"residues": np.arange(40, 140)})):   # the other two paths, in short
        a = pose_rmsd(p, kind=kind, **dict(kw(api, device), **o)).cpu().numpy()
        b = pose_rmsd(AtomTable.poses(t, F.family_batch()[1][:M][perm]), kind=kind, chunk=7, **dict(kw(api, device), **o)).cpu().numpy()
        assert same_bits(b, np.ascontiguousarray(a[perm][:, perm])), kind


def check_split_at_capacity(api, device, monkeypatch):
    """pose_rmsd splits its calls at the capacity: the same matrix through blocks of at most 5 x 5 poses"""
    from deeprank_gnn_amd.interface import pose_rmsd
    t, p = family(17)
    whole = pose_rmsd(p, kind="ligand", **kw(api, device)).cpu().numpy()
    calls = []
    real = type(api).pose_rmsd
    monkeypatch.setattr(type(api), "rmsd_capacity", lambda self, what: 5 if what == 0 else 4096)
    monkeypatch.setattr(type(api), "pose_rmsd", lambda self, q, stream: (calls.append((q.n_a, q.n_b)), real(self, q, stream))[1])
    assert same_bits(pose_rmsd(p, kind="ligand", **kw(api, device)).cpu().numpy(), whole)
    assert len(calls) == 10 and max(max(c) for c in calls) == 5        # 4 diagonal blocks, 6 above them
    assert same_bits(pose_rmsd(p, kind="ligand", other=p, **kw(api, device)).cpu().numpy(), whole)


def check_against_scores(api, device, M=17):
    """docking_scores' lrmsd against pose 0 as the reference structure = column 0 of pose_rmsd(kind="ligand"), within the
    sum of both bounds: 1e-6 A of the scores (tests/score_cases.py; 1e-4 A at a true 0) and this file's"""
    from deeprank_gnn_amd.interface import ScoreReference, docking_scores
    t, p = family(M)
    res_of = np.repeat(np.arange(t.n_residues), np.diff(t.atom_ptr))
    ref = ScoreReference(t, np.array(t.chains)[t.res_chain[res_of]], t.res_seq[res_of], t.atom_name, p.xyz[0].astype(np.float64))
    assert ref.long_chain == (0 if t.split >= t.n_residues - t.split else 1)
    lr = docking_scores(p, ref, **kw(api, device))["lrmsd"]
    d = family_matrix(api, device).cpu().numpy()[:M, 0]
    bound = bound_sq("family 65")[:M, 0]
    assert lr[0] <= 1e-4 and d[0] == 0.0
    assert (np.abs(lr[1:] ** 2 - d[1:] ** 2) <= 2 * d[1:] * 1e-6 + 1e-12 + bound[1:]).all(), (lr, d)


# ---- 3 clustering ------------------------------------------------------------------------------------------------------
def check_raw_cluster(api, device, d, cutoff, min_size, what=""):
    """drgnn_pose_cluster_dist on a matrix against the numpy rule on the same matrix: every output, exactly"""
    from deeprank_gnn_amd.interface import pose_cluster_dist_raw
    host = d.cpu().numpy() if hasattr(d, "cpu") else np.asarray(d, dtype=np.float64)
    got = pose_cluster_dist_raw(api, d, cutoff, min_size, device)
    nb = R.neighbours_of(host, cutoff)
    M = len(host)
    assert np.array_equal(F.unpack(got["neighbours"], M), nb), what     # (unpack asserts the zero tail)
    assert np.array_equal(F.unpack(got["transposed"], M), nb.T), what
    labels, centres, sizes, ties = R.cluster(nb, min_size)
    assert np.array_equal(got["labels"], labels) and np.array_equal(got["centres"], centres) and np.array_equal(got["sizes"], sizes), what
    assert got["labels"].dtype == np.int32
    return got, ties


def check_hand_matrices(api, device):
    far = 9.0
    # two centres tie on deg 2: {0, 1, 2} and {3, 4, 5}; the smaller index wins
    d = np.full((7, 7), far)
    for grp in ((0, 1, 2), (3, 4, 5)):
        for i in grp:
            for j in grp:
                d[i, j] = 1.0
    np.fill_diagonal(d, 0.0)
    got, ties = check_raw_cluster(api, device, d, 2.0, 3)
    assert ties >= 1 and list(got["labels"]) == [0, 0, 0, 1, 1, 1, -1] and list(got["centres"]) == [0, 3] and list(got["sizes"]) == [3, 3]
    # nobody clustered; and min_size 1: every pose a cluster of its own, in index order
    got, _ = check_raw_cluster(api, device, d, 0.5, 2)
    assert list(got["labels"]) == [-1] * 7 and got["centres"].size == 0 and not got["neighbours"].any()
    got, _ = check_raw_cluster(api, device, d, 0.5, 1)
    assert list(got["labels"]) == list(range(7)) and list(got["sizes"]) == [1] * 7
    # an asymmetric matrix is taken as it is: 0 is a neighbour of 1 only
    got, _ = check_raw_cluster(api, device, np.array([[0.0, 5.0], [1.0, 0.0]]), 2.0, 2)
    assert np.array_equal(F.unpack(got["neighbours"], 2), [[False, False], [True, False]]) and list(got["labels"]) == [0, 0]
    assert list(got["centres"]) == [1]
    # exactly at the cutoff is a neighbour; the next float64 above it is not
    cut = 7.5
    got, _ = check_raw_cluster(api, device, np.array([[0.0, cut, np.nextafter(cut, 9.0)], [cut, 0.0, far], [np.nextafter(cut, 9.0), far, 0.0]]), cut, 2)
    assert list(got["labels"]) == [0, 0, -1]
    # the word edges
    rng = np.random.default_rng(3)
    for M in (64, 65, 130):
        d = rng.uniform(0.0, 10.0, size=(M, M))
        d[rng.integers(0, M, 40), rng.integers(0, M, 40)] = 2.5        # some entries exactly at the cutoff
        check_raw_cluster(api, device, d, 2.5, 3, "M = %d" % M)
        check_raw_cluster(api, device, (d + d.T) / 2, 1.5, 2, "M = %d" % M)


def family_ref():
    """rmsd_ref on the 130 poses, once: (D by (a), its clusters at CUTOFF / MIN_SIZE)"""
    def make():
        sq, _ = ref_sq("family 130")
        d = np.sqrt(np.maximum(sq, 0.0) / len(inputs()["family 130"][1]))
        return d, R.cluster_dist(d, CUTOFF, MIN_SIZE)
    return once("family_ref", make)


def check_family_ref():
    """on the reference alone: at least 3 clusters, a pose in none, and no pair within 1e-6 A of the cutoff (the kernels'
    D then decides every neighbour as the reference's does: the bound is ~1e-11 A^2)"""
    d, (labels, centres, sizes, ties) = family_ref()
    assert len(centres) >= 3 and (labels == -1).sum() >= 1, (sizes, labels)
    assert np.abs(d - CUTOFF)[np.triu_indices(130, 1)].min() > 1e-6
    assert (bound_sq("family 130") < 1e-9).all()
    print("130 poses, cutoff %g: clusters of sizes %s, %d poses in none, %d tied centre choices" % (CUTOFF, sizes.tolist(), (labels == -1).sum(), ties))


def check_family_clusters(api, device):
    from deeprank_gnn_amd.interface import cluster_poses_rmsd, pose_rmsd
    t, p = family(130)
    want, (labels, centres, sizes, _) = family_ref()
    d = pose_rmsd(p, kind="ligand", **kw(api, device))
    assert_matrix(d, "family 130")
    check_raw_cluster(api, device, d, CUTOFF, MIN_SIZE, "the device's own matrix")
    for r in (cluster_poses_rmsd(d, cutoff=CUTOFF, min_size=MIN_SIZE, **kw(api, device)),
              cluster_poses_rmsd(p, cutoff=CUTOFF, min_size=MIN_SIZE, kind="ligand", **kw(api, device)),
              cluster_poses_rmsd(d.cpu().numpy(), cutoff=CUTOFF, min_size=MIN_SIZE, **kw(api, device))):
        assert r.n_contacts is None and r.labels.dtype == np.int64
        assert np.array_equal(r.labels, labels) and np.array_equal(r.centres, centres) and np.array_equal(r.sizes, sizes)
    # ranking works on the result
    scores = np.random.default_rng(4).normal(size=130)
    order, means = r.rank(scores, top=4)
    want_order, want_means = F.R.rank(labels, len(centres), scores, 4, False)
    assert np.array_equal(order, want_order) and same_bits(means, want_means)


def check_interface_residues(api, device):
    from deeprank_gnn_amd.interface import interface_residues, pose_contacts, pose_rmsd
    t, p = atn_poses()
    c = pose_contacts(p, **kw(api, device))
    maps = F.atn_maps(True)
    assert np.array_equal(interface_residues(c), atn_interface()) and interface_residues(c).dtype == np.int64
    for k in (2, 4):
        want = np.concatenate((np.flatnonzero(maps.any(axis=2).sum(axis=0) >= k), t.split + np.flatnonzero(maps.any(axis=1).sum(axis=0) >= k)))
        assert np.array_equal(interface_residues(c, min_poses=k), want)
    d = pose_rmsd(p, kind="interface", residues=interface_residues(c), **kw(api, device))
    assert_matrix(d, "1ATN interface")


# ---- 4 capacity, empty batch, refusals ---------------------------------------------------------------------------------
def check_empty_batch(api, device):
    from deeprank_gnn_amd.interface import AtomTable, cluster_poses_rmsd, pose_rmsd
    t, p = family(3)
    none = AtomTable.poses(t, F.family_batch()[1][:0])
    for a in (api, NoLaunch(api)):
        d = pose_rmsd(none, kind="ligand", api=a, device=device)
        assert tuple(d.shape) == (0, 0) and d.dtype.is_floating_point and d.element_size() == 8
        assert tuple(pose_rmsd(none, kind="all", other=p, api=a, device=device).shape) == (0, 3)
        assert tuple(pose_rmsd(p, kind="all", other=none, api=a, device=device).shape) == (3, 0)
        for r in (cluster_poses_rmsd(none, kind="ligand", api=a, device=device), cluster_poses_rmsd(np.zeros((0, 0)), api=a, device=device)):
            assert len(r) == 0 and r.labels.shape == (0,) and r.centres.shape == (0,) and r.sizes.shape == (0,) and r.n_contacts is None
            assert r.rank(np.zeros(0))[0].shape == (0,)


def check_capacity(api, device):
    """the documented capacities; one pose beyond either is refused, never answered"""
    import pytest
    import torch
    from deeprank_gnn_amd._lib import DrgnnError
    from deeprank_gnn_amd.interface import cluster_poses_rmsd, pose_cluster_dist_raw, pose_rmsd_raw
    pcap, ccap = api.rmsd_capacity(0), api.rmsd_capacity(1)
    assert pcap >= 1024 and ccap == api.fcc_capacity(2) and api.rmsd_capacity(2) == -1 and api.rmsd_capacity(-1) == -1
    assert api.rmsd_workspace(3, 2, 4, 5) == (8 * 29 * 5, [0, 8 * 29 * 3, 8 * 29 * 5])
    # a side at its capacity: one grid atom per pose, x = the pose index, against two poses
    x = np.zeros((pcap + 1, 1, 3), dtype=np.float32)
    x[:, 0, 0] = np.arange(pcap + 1)
    a, b = torch.from_numpy(x).to(device), torch.from_numpy(x[[0, 7]]).to(device)
    want = np.abs(np.arange(pcap + 1, dtype=np.float64)[:, None] - np.array([0.0, 7.0])[None])
    assert np.array_equal(pose_rmsd_raw(api, a[:pcap], b, [0]).cpu().numpy(), want[:pcap])
    assert np.array_equal(pose_rmsd_raw(api, b, a[:pcap], [0]).cpu().numpy(), want[:pcap].T)
    for args in ((a, b), (b, a)):
        with pytest.raises(DrgnnError, match="capacity"):
            pose_rmsd_raw(api, args[0], args[1], [0])
    # clustering at its capacity: three groups and 96 poses alone
    rng = np.random.default_rng(2)
    group = np.concatenate((np.zeros(1500), np.full(ccap - 2096, 1), np.full(500, 2), 3 + np.arange(96))).astype(np.int64)
    group = group[rng.permutation(ccap)]
    d = np.where(group[:, None] == group[None, :], 1.0, 9.0)
    np.fill_diagonal(d, 0.0)
    got, _ = check_raw_cluster(api, device, d, 2.0, 4, "at the cluster capacity")
    assert sorted(got["sizes"].tolist()) == sorted([1500, ccap - 2096, 500]) and (got["labels"] == -1).sum() == 96
    big = torch.zeros((ccap + 1, ccap + 1), dtype=torch.float64, device=device)
    with pytest.raises(DrgnnError, match="capacity"):
        pose_cluster_dist_raw(api, big, 2.0, 4, device)
    with pytest.raises(DrgnnError, match="capacity"):
        cluster_poses_rmsd(big, **kw(api, device))
    with pytest.raises(DrgnnError, match="capacity"):                  # refused before any distance is computed
        cluster_poses_rmsd(np.zeros((ccap + 1, 8, 3), np.float32), table=hand()[0], kind="all", api=NoLaunch(api), device=device)


def check_value_errors():
    """the Python side refuses before anything is uploaded (api=object() would fail at the first call)"""
    import pytest
    from deeprank_gnn_amd.interface import AtomTable, cluster_poses_rmsd, interface_residues, pose_rmsd, select_atoms
    t, p = hand()
    o = {"api": object(), "device": "cpu"}
    bare = AtomTable(np.array(["A"] * 4 + ["B"] * 4), np.arange(8), np.array(["ALA"] * 8), p.xyz[0])
    for bad, match in (({}, "rms="), ({"kind": "backbone"}, "kind must"), ({"kind": "all", "rms": [0]}, "one or the other"),
                       ({"kind": "all", "fit": [0, 1, 2]}, "one or the other"), ({"kind": "interface"}, "residues="),
                       ({"kind": "all", "residues": [0]}, "residues="), ({"rms": [0], "residues": [0]}, "residues="),
                       ({"rms": []}, "at least 1"), ({"rms": [0], "fit": [0, 1]}, "at least 3"), ({"rms": [8]}, "indices"),
                       ({"rms": [0], "fit": [0, 1, -1]}, "indices"), ({"rms": [0.5]}, "atom indices"), ({"rms": [[0]]}, "atom indices"),
                       ({"kind": "interface", "residues": [99]}, "residues"), ({"kind": "interface", "residues": []}, "at least 1")):
        with pytest.raises(ValueError, match=match):
            pose_rmsd(p, **dict(o, **bad))
    with pytest.raises(ValueError, match="atom_name"):
        pose_rmsd(AtomTable.poses(bare, p.xyz), kind="all", **o)
    with pytest.raises(ValueError, match="atom_name"):
        select_atoms(bare)
    with pytest.raises(ValueError, match="chain"):
        select_atoms(t, chain=2)
    with pytest.raises(ValueError, match="same AtomTable"):
        pose_rmsd(p, kind="all", other=AtomTable.poses(bare, p.xyz), **o)
    with pytest.raises(ValueError, match="table="):
        pose_rmsd(p.xyz, kind="all", **o)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cutoff"):
            cluster_poses_rmsd(p, cutoff=bad, kind="all", **o)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="min_size"):
            cluster_poses_rmsd(p, min_size=bad, kind="all", **o)
    with pytest.raises(ValueError, match="other"):
        cluster_poses_rmsd(p, kind="all", other=p, **o)
    with pytest.raises(ValueError, match="come with poses"):
        cluster_poses_rmsd(np.zeros((3, 3)), kind="all", **o)
    with pytest.raises(ValueError, match="PoseContacts"):
        interface_residues(p)


REQUESTS = {"rmsd": ("PoseRmsdRequest", "pose_rmsd", "drgnn_pose_rmsd"),
            "cluster_dist": ("PoseClusterDistRequest", "pose_cluster_dist", "drgnn_pose_cluster_dist")}


def refusal_cases():
    """(entry point, name) -> what to change in a good request; "tab_*": a host list; None: handled by name"""
    nan, inf = float("nan"), float("inf")
    cases = {("rmsd", "null " + k): {k: None} for k in ("xyz_a", "xyz_b", "rms_idx", "host_rms_idx", "fit_idx", "host_fit_idx",
                                                         "workspace", "d")}
    cases.update({("rmsd", k): v for k, v in {
        "n_a negative": {"n_a": -1}, "n_b negative": {"n_b": -1}, "n_atoms negative": {"n_atoms": -1}, "n_fit negative": {"n_fit": -1},
        "n_rms negative": {"n_rms": -1}, "n_rms 0": {"n_rms": 0}, "n_fit 1": {"n_fit": 1}, "n_fit 2": {"n_fit": 2},
        "rms index -1": {"tab_rms": [4, -1, 6, 7]}, "rms index T": {"tab_rms": [4, 5, 6, 8]}, "fit index T": {"tab_fit": [0, 8, 2, 3]},
        "fit index negative": {"tab_fit": [-2, 1, 2, 3]}, "n_atoms below an index": {"n_atoms": 7},
        "phases 4": {"phases": 4}, "phases negative": {"phases": -1}, "workspace misaligned": {"workspace": "odd"},
    }.items()})
    cases.update({("cluster_dist", "null " + k): {k: None} for k in ("d", "neighbours", "transposed", "labels", "centres", "sizes", "n_clusters")})
    cases.update({("cluster_dist", k): v for k, v in {
        "n_poses negative": {"n_poses": -1}, "min_size 0": {"min_size": 0}, "min_size negative": {"min_size": -3},
        "cutoff 0": {"cutoff": 0.0}, "cutoff negative": {"cutoff": -7.5}, "cutoff NaN": {"cutoff": nan}, "cutoff inf": {"cutoff": inf},
    }.items()})
    for entry in REQUESTS:
        cases[entry, "capacity"] = None
        cases[entry, "null request"] = None
    cases["rmsd", "capacity of side b"] = None
    cases["rmsd", "workspace too small"] = None
    return cases


def refusal_names():
    return sorted("%s: %s" % k for k in refusal_cases())


FILL = -7.0


def check_refusal(api, device, name):
    """one malformed field: refused on the host, before a launch (the outputs keep their fill); the good request then runs"""
    import pytest
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._lib import DrgnnError
    entry, what = name.split(": ", 1)
    over = refusal_cases()[entry, what]
    t, p = hand()
    M = len(p)
    dev = torch.device(device)
    rms, fit = HAND_LISTS["ligand"]
    xyz = torch.from_numpy(p.xyz).to(dev)
    nbytes = api.rmsd_workspace(M, M, 4, 4)[0]
    ws = torch.full((nbytes // 8 + 1,), FILL, dtype=torch.float64, device=dev)
    d = torch.full((M, M), FILL, dtype=torch.float64, device=dev)
    good_d = torch.from_numpy(np.sqrt(ref_sq("hand ligand")[0] / 4.0)).to(dev)
    nb = torch.full((2, M, 1), int(FILL), dtype=torch.int64, device=dev)
    res = torch.full((3, M), int(FILL), dtype=torch.int32, device=dev)
    k = torch.full((1,), int(FILL), dtype=torch.int32, device=dev)
    outputs = {"rmsd": (d, ws), "cluster_dist": (nb, res, k)}[entry]
    keep = []

    def request(**ch):
        q = getattr(_lib, REQUESTS[entry][0])()
        if entry == "rmsd":
            host = [np.ascontiguousarray(ch.pop("tab_" + n, v), dtype=np.int32) for n, v in (("rms", rms), ("fit", fit))]
            devl = [torch.from_numpy(h).to(dev) for h in host]
            keep.extend(host + devl)
            q.xyz_a = q.xyz_b = xyz.data_ptr()
            q.rms_idx, q.fit_idx, q.host_rms_idx, q.host_fit_idx = devl[0].data_ptr(), devl[1].data_ptr(), host[0].ctypes.data, host[1].ctypes.data
            q.n_a, q.n_b, q.n_atoms, q.n_fit, q.n_rms = M, M, 8, 4, 4
            q.workspace, q.workspace_bytes, q.d = ws.data_ptr(), nbytes, d.data_ptr()
            if ch.get("workspace") == "odd":
                ch["workspace"] = ws.data_ptr() + 4
        else:
            q.d, q.n_poses, q.cutoff, q.min_size = good_d.data_ptr(), M, 2.0, 2
            q.neighbours, q.transposed = nb[0].data_ptr(), nb[1].data_ptr()
            q.labels, q.centres, q.sizes, q.n_clusters = res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), k.data_ptr()
        for key, v in ch.items():
            setattr(q, key, v)
        return q

    call = getattr(api, REQUESTS[entry][1])
    stream = _lib.current_stream(xyz)
    if what == "null request":
        with pytest.raises(DrgnnError, match="bad argument"):
            _lib._check(getattr(api.lib, REQUESTS[entry][2])(None, stream), REQUESTS[entry][2])
    elif over is None:
        beyond = {"capacity": {"n_a": api.rmsd_capacity(0) + 1} if entry == "rmsd" else {"n_poses": api.rmsd_capacity(1) + 1},
                  "capacity of side b": {"n_b": api.rmsd_capacity(0) + 1}, "workspace too small": {"workspace_bytes": nbytes - 8}}[what]
        with pytest.raises(DrgnnError, match="capacity"):
            call(request(**beyond), stream)
    else:
        with pytest.raises(DrgnnError, match="bad argument"):
            call(request(**dict(over)), stream)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert all(bool((o == FILL).all()) for o in outputs)              # nothing was launched
    call(request(), stream)                                           # and the good request runs
    if entry == "rmsd":
        got = d.cpu().numpy()
        assert (np.abs(got * got - ref_sq("hand ligand")[0] / 4.0) <= bound_sq("hand ligand")).all() and np.array_equal(got, got.T)
        assert bool((ws[-1] == FILL).all())                           # the call stays inside the bytes it asked for
    else:
        host = good_d.cpu().numpy()
        labels, centres, sizes, _ = R.cluster_dist(host, 2.0, 2)
        K = int(k.cpu()[0])
        got = res.cpu().numpy()
        assert K == len(centres) and np.array_equal(got[0], labels) and np.array_equal(got[1, :K], centres) and np.array_equal(got[2, :K], sizes)
        assert np.array_equal(F.unpack(nb[0].cpu().numpy().view(np.uint64), M), R.neighbours_of(host, 2.0))
