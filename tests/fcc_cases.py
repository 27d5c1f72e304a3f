"""Inputs and checks shared by tests/test_fcc.py (host emulation) and tests/test_gpu_fcc.py (the device): FCC clustering
of deeprank_gnn_amd.interface (drgnn_pose_contacts / drgnn_pose_common / drgnn_pose_cluster, csrc/drgnn_fcc.h) against
the numpy statement of the rule in tests/fcc_ref.py, which sees the float32 coordinates the kernel sees.

Every comparison is exact equality: contacts, counts, common contacts, the fcc matrix (one float64 division on either
side), the neighbour relation, labels, centres and sizes.  Hand-made atoms live on the 1/8 A grid, so that distances
are exact in float32 and grid translations and quarter turns keep them exact."""
import numpy as np

import fcc_ref as R
from bsa_cases import atn, same_bits
from hse_cases import RX, RZ, Chains, zigzag

# the four 1ATN poses, heavy atoms / all atoms, cutoff 5 A (computed on the CPU with the rule of fcc_ref)
ATN_N = {True: [53, 43, 60, 19], False: [66, 59, 74, 23]}
ATN_COMMON = {True: [[53, 32, 41, 16], [32, 43, 37, 16], [41, 37, 60, 16], [16, 16, 16, 19]],
              False: [[66, 41, 50, 18], [41, 59, 44, 19], [50, 44, 74, 19], [18, 19, 19, 23]]}
BATCH_SIZES = (1, 2, 17, 64, 65, 130)
_CACHE = {}


def kw(api, device):
    return {"api": api, "device": device}


def ref_maps(table, xyz32, heavy_only=None, cutoff=5.0):
    """bool [M, nA, nB]: fcc_ref's contact maps of float32 poses xyz32 [M, T, 3] in the table's grouped order"""
    heavy = table.atom_name is not None if heavy_only is None else heavy_only
    cnt = R.counted(table.atom_name, table.n_atoms, heavy)
    return np.stack([R.contact_map(x, table.atom_ptr, table.split, cnt, cutoff) for x in xyz32])


def check_contacts(c, maps, what=""):
    """a PoseContacts against fcc_ref's maps: pairs, counts, the zero tail of every row.  Returns common of the maps"""
    assert len(c) == len(maps), what
    assert c.n_contacts.dtype == np.int64 and np.array_equal(c.n_contacts, maps.reshape(len(maps), -1).sum(axis=1)), what
    words = c.words()
    assert words.shape == (len(maps), c.n_a, (c.n_b + 63) // 64)
    for m in range(len(maps)):
        p = c.pairs(m)
        assert p.dtype == np.int32 and np.array_equal(p, R.pairs_of(maps[m])), (what, m)
    if c.n_b % 64 and words.size:
        assert not (words[:, :, -1] >> np.uint64(c.n_b % 64)).any(), what          # the tail bits are zero
    return R.common_of(maps)


def check_clusters(got, common, n, cutoff_fcc=0.6, strictness=0.75, min_size=4, what=""):
    """labels, centres, sizes of a PoseClusters (or a pose_cluster_raw dict) against fcc_ref"""
    labels, centres, sizes, ties = R.cluster(R.neighbours_of(common, n, cutoff_fcc, strictness), min_size)
    g = got if isinstance(got, dict) else {"labels": got.labels, "centres": got.centres, "sizes": got.sizes}
    assert np.array_equal(g["labels"], labels), (what, g["labels"], labels)
    assert np.array_equal(g["centres"], centres) and np.array_equal(g["sizes"], sizes), (what, g["centres"], centres, g["sizes"], sizes)
    return labels, centres, sizes, ties


def unpack(rows, M):
    """bool [M, M] of uint64 bit rows [M, ceil(M/64)]; asserts the zero tail"""
    bits = np.unpackbits(np.ascontiguousarray(rows).view(np.uint8).reshape(M, -1), axis=1, bitorder="little")
    assert not bits[:, M:].any()
    return bits[:, :M].astype(bool)


def check_raw_cluster(api, device, common, n, cutoff_fcc=0.6, strictness=0.75, min_size=4, what=""):
    """drgnn_pose_cluster on a hand-written common / n_contacts: the relation, its transpose and the clusters"""
    from deeprank_gnn_amd.interface import pose_cluster_raw
    common, n = np.asarray(common, dtype=np.int32), np.asarray(n, dtype=np.int32)
    got = pose_cluster_raw(api, common, n, cutoff_fcc, np.float64(cutoff_fcc) * np.float64(strictness), min_size, device)
    nb = R.neighbours_of(common, n, cutoff_fcc, strictness)
    assert np.array_equal(unpack(got["neighbours"], len(n)), nb), what
    assert np.array_equal(unpack(got["transposed"], len(n)), nb.T), what
    check_clusters(got, common, n, cutoff_fcc, strictness, min_size, what)
    return got


# ---- 1 the four 1ATN poses -------------------------------------------------------------------------------------------
def atn_maps(heavy):
    if ("atn", heavy) not in _CACHE:
        from deeprank_gnn_amd.interface import AtomTable
        a = atn()
        _CACHE["atn", heavy] = ref_maps(a["table"], AtomTable.poses(a["table"], a["xyz"]).xyz, heavy)
    return _CACHE["atn", heavy]


def check_ref_literals():
    """fcc_ref against the literals (no kernel: this pins the rule)"""
    for heavy in (True, False):
        common = R.common_of(atn_maps(heavy))
        assert np.array_equal(common, ATN_COMMON[heavy]) and list(np.diag(common)) == ATN_N[heavy]
    common = np.array(ATN_COMMON[True])
    f = R.fcc_of(common, np.diag(common))
    assert np.all(f[3, :3] > 0.84) and np.all(f[:3, 3] <= 0.38) and np.all(f[:3, 3] < 0.45)     # the directed relation decides
    labels, centres, sizes, _ = R.cluster(R.neighbours_of(common, np.diag(common)), 3)
    assert list(labels) == [0, 0, 0, -1] and list(centres) == [0] and list(sizes) == [3]
    assert list(R.cluster(R.neighbours_of(common, np.diag(common)), 4)[0]) == [-1] * 4


def check_atn(api, device):
    from deeprank_gnn_amd.interface import AtomTable, cluster_poses, common_contacts, fcc_matrix, pose_contacts
    a = atn()
    poses = AtomTable.poses(a["table"], a["xyz"])
    for heavy in (None, True, False):
        lit = True if heavy is None else heavy                         # the table has atom names: heavy atoms by default
        c = pose_contacts(poses, heavy_only=heavy, **kw(api, device))
        common = check_contacts(c, atn_maps(lit), "1ATN")
        assert list(c.n_contacts) == ATN_N[lit] and c.heavy_only == lit
        got = common_contacts(c)
        assert got.dtype == np.int32 and np.array_equal(got, ATN_COMMON[lit]) and np.array_equal(got, common)
        f = fcc_matrix(c)
        assert f.dtype == np.float64 and same_bits(f, R.fcc_of(common, c.n_contacts))
        r3, r4 = cluster_poses(c, min_size=3), cluster_poses(c)
        check_clusters(r3, common, c.n_contacts, min_size=3)
        check_clusters(r4, common, c.n_contacts)
        assert list(r3.labels) == [0, 0, 0, -1] and list(r3.centres) == [0] and list(r3.sizes) == [3] and len(r4) == 0
        assert list(r4.labels) == [-1] * 4 and np.array_equal(r3.n_contacts, ATN_N[lit])
    # from poses in one call, from a table, from coordinates + table
    r = cluster_poses(poses, min_size=3, heavy_only=False, **kw(api, device))
    assert list(r.labels) == [0, 0, 0, -1] and list(r.n_contacts) == ATN_N[False]
    one = pose_contacts(a["table"], **kw(api, device))
    assert list(one.n_contacts) == ATN_N[True][:1]
    again = pose_contacts(poses.xyz[1:3], table=a["table"], **kw(api, device))
    assert list(again.n_contacts) == ATN_N[True][1:3]


# ---- 2 hand-made atoms -----------------------------------------------------------------------------------------------
def atoms_of(chain, atoms, name="ALA"):
    return (chain, name, atoms)


def hand_cases():
    """name -> (Chains, {heavy_only: the pairs the rule gives by hand})"""
    ca = lambda p: ("CA", np.array(p, dtype=np.float64))
    cases = {
        # exactly 5.0 A is a contact, 5.125 A is not
        "cutoff_edge": (Chains([atoms_of("A", [ca((0, 0, 0))]), atoms_of("B", [ca((5, 0, 0))]), atoms_of("B", [ca((0, 5.125, 0))])]),
                        {True: [(0, 1)], False: [(0, 1)]}),
        "cutoff_edge_3_4": (Chains([atoms_of("A", [ca((1, 1, 1))]), atoms_of("B", [ca((4, 5, 1))]), atoms_of("B", [ca((4, 5, 1.125))])]),
                            {True: [(0, 1)], False: [(0, 1)]}),
        # a contact made by hydrogens only (names HA, and 2HB with a leading digit); a heavy atom named OH counts
        "hydrogen_only": (Chains([atoms_of("A", [ca((0, 0, 0)), ("OH", np.array((0.0, -20.0, 0.0)))]),
                                  atoms_of("B", [ca((9, 0, 0)), ("HA", np.array((4.0, 0.0, 0.0)))]),
                                  atoms_of("B", [ca((0, 9, 0)), ("2HB", np.array((0.0, 4.0, 0.0)))]),
                                  atoms_of("B", [ca((0, -29, 0)), ("H", np.array((0.0, -24.0, 0.0)))])]),
                          {True: [], False: [(0, 1), (0, 2), (0, 3)]}),
        # a residue spread over 20 A: its centroid is 14 A from the partner, one of its atoms 4 A
        "spread_residue": (Chains([atoms_of("A", [ca((0, 0, 0)), ("CB", np.array((20.0, 0.0, 0.0)))]),
                                   atoms_of("A", [ca((40, 0, 0))]),
                                   atoms_of("B", [ca((-4, 0, 0))]), atoms_of("B", [ca((30, 3, 0))])]),
                           {True: [(0, 2)], False: [(0, 2)]}),
    }
    return cases


def check_hand_case(name, api, device):
    from deeprank_gnn_amd.interface import pose_contacts
    atoms, want = hand_cases()[name]
    t = atoms.table()
    for heavy, pairs in want.items():
        c = pose_contacts(t, heavy_only=heavy, **kw(api, device))
        maps = ref_maps(t, t.xyz[None], heavy)
        check_contacts(c, maps, name)
        assert [tuple(p) for p in c.pairs(0)] == pairs, (name, heavy, c.pairs(0))
        assert list(c.n_contacts) == [len(pairs)]


def word_edge_table(n_b):
    """chain 1 of n_b CA-only residues 16 A apart; residue 0 of chain 0 has an atom 4 A from the residue at the first and
    at the last bit of every word (its atoms lie up to 16 n_b A apart), residue 1 touches the second bit of every word"""
    edge = sorted(set([b for b in range(n_b) if b % 64 in (0, 63)] + [n_b - 1]))
    second = [b for b in range(n_b) if b % 64 == 1]
    res = [atoms_of("A", [("CA" if k == 0 else "C%d" % k, np.array((16.0 * b, 4.0, 0.0))) for k, b in enumerate(edge)]),
           atoms_of("A", [("CA" if k == 0 else "C%d" % k, np.array((16.0 * b, 0.0, -3.0))) for k, b in enumerate(second)]
                    or [("CA", np.array((0.0, 0.0, -300.0)))])]
    res += [atoms_of("B", [("CA", np.array((16.0 * b, 0.0, 0.0)))]) for b in range(n_b)]
    return Chains(res).table(), [(0, 2 + b) for b in edge] + [(1, 2 + b) for b in second]


def check_word_edges(api, device, n_b):
    from deeprank_gnn_amd.interface import pose_contacts
    t, pairs = word_edge_table(n_b)
    c = pose_contacts(t, **kw(api, device))
    check_contacts(c, ref_maps(t, t.xyz[None]), "n_b = %d" % n_b)
    assert [tuple(p) for p in c.pairs(0)] == pairs and c.words().shape == (1, 2, (n_b + 63) // 64)


def no_contact_batch():
    """three poses of a small complex: the middle one has chain 1 moved 100 A away"""
    atoms = Chains(zigzag(6) + zigzag(5, x0=1.0, chain="B"))
    xyz = np.stack([atoms.xyz] * 3)
    xyz[:, atoms.chain == "B"] += (0.0, 4.0, 0.0)
    xyz[1, atoms.chain == "B"] += (0.0, 100.0, 0.0)
    return atoms, xyz


def check_no_contact_pose(api, device):
    from deeprank_gnn_amd.interface import AtomTable, cluster_poses, fcc_matrix, pose_cluster_raw, pose_contacts
    atoms, xyz = no_contact_batch()
    t = atoms.table()
    poses = AtomTable.poses(t, xyz)
    c = pose_contacts(poses, **kw(api, device))
    common = check_contacts(c, ref_maps(t, poses.xyz))
    assert c.n_contacts[1] == 0 and c.n_contacts[0] == c.n_contacts[2] > 0 and len(c.pairs(1)) == 0
    f = fcc_matrix(c)
    assert same_bits(f, R.fcc_of(common, c.n_contacts)) and not f[1].any() and not f[:, 1].any() and f[0, 2] == 1.0
    r = cluster_poses(c, min_size=2)
    check_clusters(r, common, c.n_contacts, min_size=2)
    assert list(r.labels) == [0, -1, 0]
    raw = check_raw_cluster(api, device, common, c.n_contacts, min_size=1)           # never a neighbour; a cluster of its own
    assert not unpack(raw["neighbours"], 3)[1].any() and not unpack(raw["neighbours"], 3)[:, 1].any()
    assert list(raw["labels"]) == [0, 1, 0] and list(raw["sizes"]) == [2, 1]


# ---- 3 pose batches ----------------------------------------------------------------------------------------------------
def rotation(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    t = np.deg2rad(degrees)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def family_batch(n=130, seed=7, jitter=(4.0, 1.0), within=12.0):
    """(table, xyz float64 [n, T, 3]): the residues of 1ATN pose 1w with an atom within `within` A of the other chain (None:
    all of them), and n
    poses made by rigid moves of chain 1: jitters (degrees, A: `jitter`) around three placements (families of different sizes), and every
    tenth pose thrown far off its family"""
    if ("family", n, seed, jitter, within) not in _CACHE:
        from deeprank_gnn_amd.interface import AtomTable
        a = atn()
        chain, seq, res, names = a["per_atom"]
        x = a["xyz"][0]
        ia, ib = np.flatnonzero(chain == "A"), np.flatnonzero(chain == "B")
        near = np.zeros(len(x), dtype=bool)                            # an atom within that distance of the other chain
        for lo in range(0, len(ia), 256):
            d2 = ((x[ia[lo:lo + 256]][:, None, :] - x[ib][None, :, :]) ** 2).sum(axis=2) < (1e30 if within is None else within * within)
            near[ia[lo:lo + 256]] |= d2.any(axis=1)
            near[ib] |= d2.any(axis=0)
        near_a, near_b = set(seq[ia][near[ia]]), set(seq[ib][near[ib]])
        keep = np.array([(c == "A" and s in near_a) or (c == "B" and s in near_b) for c, s in zip(chain, seq)])
        table = AtomTable(chain[keep], seq[keep], res[keep], x[keep], atom_name=names[keep])
        xs, isb = x[keep], chain[keep] == "B"
        centre = xs[isb].mean(axis=0)
        rng = np.random.default_rng(seed)
        places = [(rotation((1, 0, 0), 0.0), np.zeros(3)), (rotation((0, 1, 1), 14.0), np.array((2.0, -1.5, 1.0))),
                  (rotation((1, -1, 0), -20.0), np.array((-3.0, 2.0, 2.5)))]
        family = rng.choice(3, size=n, p=(0.5, 0.3, 0.2))
        out = np.repeat(xs[None], n, axis=0)
        for m in range(n):
            rot, shift = places[family[m]]
            wild = m % 10 == 9
            jit = rotation(rng.normal(size=3), rng.normal() * (40.0 if wild else jitter[0]))
            move = rng.normal(size=3) * (8.0 if wild else jitter[1])
            out[m, isb] = (xs[isb] - centre) @ (jit @ rot).T + centre + shift + move
        _CACHE["family", n, seed, jitter, within] = (table, out)
    return _CACHE["family", n, seed, jitter, within]


def family_ref():
    """fcc_ref on the 130 poses, once: (maps, common, n, clusters at min_size 4); batches of M poses are the first M"""
    if "family_ref" not in _CACHE:
        from deeprank_gnn_amd.interface import AtomTable
        table, xyz = family_batch()
        maps = ref_maps(table, AtomTable.poses(table, xyz).xyz)
        common = R.common_of(maps)
        n = np.diag(common).copy()
        labels, centres, sizes, ties = R.cluster(R.neighbours_of(common, n), 4)
        # the batch exercises what it is there for: several clusters of different sizes, poses left over, a tie on deg
        assert len(centres) >= 3 and len(set(sizes.tolist())) >= 2 and (labels == -1).sum() >= 1 and ties >= 1, (sizes, ties)
        assert table.n_residues - table.split > 64 and table.split > 64
        _CACHE["family_ref"] = (maps, common, n, (labels, centres, sizes, ties))
    return _CACHE["family_ref"]


def check_batch(api, device, M, contacts=None):
    """the first M poses of the family batch: contacts, common, fcc, relation and clusters against fcc_ref"""
    from deeprank_gnn_amd.interface import AtomTable, cluster_poses, common_contacts, fcc_matrix, pose_contacts
    table, xyz = family_batch()
    maps, common, n, _ = family_ref()
    maps, common, n = maps[:M], common[:M, :M], n[:M]
    c = contacts if contacts is not None else pose_contacts(AtomTable.poses(table, xyz[:M]), **kw(api, device))
    assert np.array_equal(check_contacts(c, maps, "M = %d" % M), common)
    assert np.array_equal(common_contacts(c), common)
    assert same_bits(fcc_matrix(c), R.fcc_of(common, n))
    for min_size in (4, 2):
        r = cluster_poses(c, min_size=min_size)
        labels, centres, sizes, ties = check_clusters(r, common, n, min_size=min_size, what="M = %d" % M)
        print("M = %d, min_size %d: %d clusters of sizes %s, %d poses in none, %d tied centre choices"
              % (M, min_size, len(centres), sizes.tolist(), (labels == -1).sum(), ties))
    check_raw_cluster(api, device, common, n, what="M = %d" % M)
    check_raw_cluster(api, device, common, n, cutoff_fcc=0.75, strictness=1.0, min_size=3, what="M = %d" % M)
    return c


def check_hand_relations(api, device):
    """hand-written common / n_contacts"""
    # two centres tie on deg 2: {0, 1, 2} and {3, 4, 5}, all n = 10; the smaller index must win, so labels follow the index
    n = np.full(7, 10)
    common = np.zeros((7, 7), dtype=np.int32)
    for grp in ((0, 1, 2), (3, 4, 5)):
        for i in grp:
            for j in grp:
                common[i, j] = 8
    np.fill_diagonal(common, 10)
    got = check_raw_cluster(api, device, common, n, min_size=3)
    assert list(got["labels"]) == [0, 0, 0, 1, 1, 1, -1] and list(got["centres"]) == [0, 3] and list(got["sizes"]) == [3, 3]
    # a star: 3 is linked to 0, 1, 2 and 4; 4 is also linked to 5 and 6.  deg: 3 -> 4, 4 -> 3.  The first cluster
    # {3, 0, 1, 2, 4} takes 4 away: 5 and 6 drop from deg 1 to 0; with min_size 2 nothing else is left to cluster
    common = np.zeros((7, 7), dtype=np.int32)
    for i, j in ((3, 0), (3, 1), (3, 2), (3, 4), (4, 5), (4, 6)):
        common[i, j] = common[j, i] = 9
    np.fill_diagonal(common, 10)
    got = check_raw_cluster(api, device, common, n, min_size=2)
    assert list(got["labels"]) == [0, 0, 0, 0, 0, -1, -1] and list(got["centres"]) == [3] and list(got["sizes"]) == [5]
    # ... and a second centre whose deg falls below min_size - 1 when the first cluster removes its neighbours:
    # 0 is linked to 1, 2, 3, 4; 5 is linked to 3, 4, 6.  deg 0 -> 4, 5 -> 3; after {0, 1, 2, 3, 4} pose 5 keeps only 6
    common = np.zeros((7, 7), dtype=np.int32)
    for i, j in ((0, 1), (0, 2), (0, 3), (0, 4), (5, 3), (5, 4), (5, 6)):
        common[i, j] = common[j, i] = 9
    np.fill_diagonal(common, 10)
    got = check_raw_cluster(api, device, common, n, min_size=3)
    assert list(got["labels"]) == [0, 0, 0, 0, 0, -1, -1] and list(got["sizes"]) == [5]
    assert list(check_raw_cluster(api, device, common, n, min_size=2)["labels"]) == [0, 0, 0, 0, 0, 1, 1]
    # the directed relation on an asymmetric pair: 1 has few contacts, all shared; fcc[1, 0] = 1, fcc[0, 1] = 0.3
    n2 = np.array([10, 3])
    common = np.array([[10, 3], [3, 3]], dtype=np.int32)
    got = check_raw_cluster(api, device, common, n2, min_size=2)
    assert list(got["labels"]) == [-1, -1] and not got["neighbours"].any()
    got = check_raw_cluster(api, device, common, n2, strictness=0.5, min_size=2)      # 0.3 >= 0.6 * 0.5: 0 is a neighbour of 1 only
    assert np.array_equal(unpack(got["neighbours"], 2), [[False, False], [True, False]]) and list(got["labels"]) == [0, 0]
    assert list(got["centres"]) == [1]
    # exactly on the thresholds: 6 / 10 >= 0.6 and 9 / 20 >= 0.6 * 0.75 in float64 as numpy has them
    check_raw_cluster(api, device, np.array([[10, 6], [9, 20]], dtype=np.int32), np.array([10, 20]), min_size=2)
    # a common matrix that is not symmetric is taken as it is
    rng = np.random.default_rng(1)
    n3 = rng.integers(0, 12, size=70)
    check_raw_cluster(api, device, rng.integers(0, 12, size=(70, 70)), n3, cutoff_fcc=0.5, strictness=0.5, min_size=2)


def one_relation_inputs(M):
    """(common int32 [M, M], n_contacts, d float64 [M, M]): the FCC rule at cutoff_fcc 0.5, strictness 1 on (common, 128)
    and the distance rule at cutoff 64 on d = 128 - common define one relation.  Every quotient and threshold is a binary
    fraction, so the two predicates agree exactly, the pairs with common = 64 (on the threshold of both) included"""
    rng = np.random.default_rng(11)
    common = rng.integers(0, 64, size=(M, M))
    high = rng.random((M, M)) < 0.06
    common[high] = rng.integers(64, 129, size=int(high.sum()))
    common[rng.integers(0, M, 30), rng.integers(0, M, 30)] = 64
    common = np.triu(common, 1)
    common = (common + common.T).astype(np.int32)
    np.fill_diagonal(common, 128)
    return common, np.full(M, 128, dtype=np.int32), 128.0 - common.astype(np.float64)


def check_one_relation_one_greedy(api, device, M):
    """the two rules drive one relation kernel and one greedy: on inputs that define the same relation, pose_cluster_raw
    and pose_cluster_dist_raw give identical outputs, and both equal fcc_ref.cluster on that relation.
    On the references alone: M = 65: 16 pairs at the threshold, 8 clusters, 14 poses in none, 3 tied centre choices;
    M = 130: 24, 15, 10, 7"""
    import rmsd_ref
    from deeprank_gnn_amd.interface import pose_cluster_dist_raw, pose_cluster_raw
    common, n, d = one_relation_inputs(M)
    nb = R.neighbours_of(common, n, 0.5, 1.0)
    labels, centres, sizes, ties = R.cluster(nb, 3)
    at_threshold = int((np.triu(common, 1) == 64).sum())
    print("M = %d: %d pairs at the threshold, %d clusters, %d poses in none, %d tied centre choices"
          % (M, at_threshold, len(centres), (labels == -1).sum(), ties))
    assert np.array_equal(rmsd_ref.neighbours_of(d, 64.0), nb)
    assert len(centres) >= 2 and (labels == -1).sum() >= 1 and ties >= 1 and at_threshold >= 1
    by_fcc = pose_cluster_raw(api, common, n, 0.5, 0.5, 3, device)
    by_dist = pose_cluster_dist_raw(api, d, 64.0, 3, device)
    want = {"neighbours": nb, "transposed": nb.T, "labels": labels, "centres": centres, "sizes": sizes}
    for key in ("neighbours", "transposed", "labels", "centres", "sizes"):
        assert by_fcc[key].dtype == by_dist[key].dtype and np.array_equal(by_fcc[key], by_dist[key]), (M, key)
        got = unpack(by_fcc[key], M) if key in ("neighbours", "transposed") else by_fcc[key]
        assert np.array_equal(got, want[key]), (M, key)


# ---- 4 independence ----------------------------------------------------------------------------------------------------
def check_independence(api, device, M=17):
    """M, chunk, place and run change no bit; blocks of common; permutations.  Returns the batch's PoseContacts"""
    from deeprank_gnn_amd.interface import AtomTable, cluster_poses, common_contacts, fcc_matrix, pose_contacts
    table, xyz = family_batch()
    xyz = xyz[:M]
    full = pose_contacts(AtomTable.poses(table, xyz), **kw(api, device))
    words, n = full.words(), full.n_contacts
    for chunk in (1, 5, M):
        again = pose_contacts(AtomTable.poses(table, xyz), chunk=chunk, **kw(api, device))
        assert same_bits(again.words(), words) and same_bits(again.n_contacts, n), chunk
    for m in (0, M // 2, M - 1):
        alone = pose_contacts(AtomTable.poses(table, xyz[m:m + 1]), **kw(api, device))
        assert same_bits(alone.words()[0], words[m]) and alone.n_contacts[0] == n[m]
    perm = np.random.default_rng(5).permutation(M)
    moved = pose_contacts(AtomTable.poses(table, xyz[perm]), **kw(api, device))
    assert same_bits(moved.words(), words[perm]) and same_bits(moved.n_contacts, n[perm])
    common, f = common_contacts(full), fcc_matrix(full)
    assert same_bits(common_contacts(moved), np.ascontiguousarray(common[perm][:, perm]))
    assert same_bits(fcc_matrix(moved), np.ascontiguousarray(f[perm][:, perm]))
    assert np.array_equal(common, common.T) and np.array_equal(np.diag(common), n)
    lo, hi = pose_contacts(AtomTable.poses(table, xyz[:6]), **kw(api, device)), pose_contacts(AtomTable.poses(table, xyz[6:]), **kw(api, device))
    assert same_bits(common_contacts(lo, hi), np.ascontiguousarray(common[:6, 6:]))
    assert same_bits(common_contacts(hi, lo), np.ascontiguousarray(common[6:, :6]))
    assert same_bits(common_contacts(hi, full), np.ascontiguousarray(common[6:]))
    assert same_bits(fcc_matrix(hi, lo), np.ascontiguousarray(f[6:, :6]))
    for min_size in (2, 4):                                            # the permuted batch against the ref on the same permutation
        check_clusters(cluster_poses(moved, min_size=min_size), common[perm][:, perm], n[perm], min_size=min_size)
    first, second = cluster_poses(full, min_size=2), cluster_poses(full, min_size=2)           # two runs
    assert all(same_bits(getattr(first, k), getattr(second, k)) for k in ("labels", "centres", "sizes", "n_contacts"))
    assert same_bits(common_contacts(full), common)
    return full


def assert_same_results(x, y):
    """two PoseContacts (the device's and the emulation's), and everything derived from them, exactly"""
    from deeprank_gnn_amd.interface import cluster_poses, common_contacts
    assert same_bits(x.words(), y.words()) and same_bits(x.n_contacts, y.n_contacts)
    assert same_bits(common_contacts(x), common_contacts(y))
    for min_size in (2, 4):
        a, b = cluster_poses(x, min_size=min_size), cluster_poses(y, min_size=min_size)
        assert all(same_bits(getattr(a, k), getattr(b, k)) for k in ("labels", "centres", "sizes"))


# ---- 5 rigid motions ---------------------------------------------------------------------------------------------------
def check_rigid_motion(api, device):
    """grid translations and quarter turns of whole complexes change no bit of any output"""
    from deeprank_gnn_amd.interface import AtomTable, cluster_poses, common_contacts, pose_contacts
    atoms = Chains(zigzag(9) + zigzag(7, x0=1.0, chain="B"))
    isb = atoms.chain == "B"
    shifts = [(0.0, 4.0, 0.0), (0.125, 4.0, 0.0), (0.0, 4.25, 0.5), (2.25, 5.0, 0.0), (2.25, 5.0, 0.125), (4.5, 4.0, 1.0),
              (0.0, 60.0, 0.0), (2.375, 5.0, 0.0)]
    xyz = np.stack([atoms.xyz] * len(shifts))
    for m, s in enumerate(shifts):
        xyz[m, isb] += s
    t = atoms.table()

    def run(x):
        c = pose_contacts(AtomTable.poses(t, x), **kw(api, device))
        r = cluster_poses(c, min_size=2)
        return c, (c.words(), c.n_contacts, common_contacts(c), r.labels, r.centres, r.sizes)

    c, base = run(xyz)
    common = check_contacts(c, ref_maps(t, AtomTable.poses(t, xyz).xyz))
    check_clusters(cluster_poses(c, min_size=2), common, c.n_contacts, min_size=2)
    assert len(set(c.n_contacts.tolist())) >= 3 and base[4].size >= 1
    for moved in (xyz + (3.0, -2.5, 8.0), xyz @ RZ.T, xyz @ (RX @ RZ).T + (0.0, 16.0, -7.125),
                  xyz @ (RZ @ RZ @ RX).T - (100.0, 0.125, 64.0)):
        assert all(same_bits(u, v) for u, v in zip(run(moved)[1], base))


# ---- 6 capacity, refusals, empty batch ---------------------------------------------------------------------------------
def ladder_table(n_a, n_b):
    """CA-only residues 4 A apart along x, the two chains 4 A apart in y: residue i of one chain touches residue i of the other"""
    from deeprank_gnn_amd.interface import AtomTable
    i = np.concatenate((np.arange(n_a), np.arange(n_b)))
    chain = np.array(["A"] * n_a + ["B"] * n_b)
    xyz = np.stack((4.0 * i, np.where(chain == "A", 0.0, 4.0), np.zeros(n_a + n_b)), axis=1)
    return AtomTable(chain, np.arange(n_a + n_b) + 1, np.array(["ALA"] * (n_a + n_b)), xyz, atom_name=np.array(["CA"] * (n_a + n_b)))


def check_capacity(api, device):
    """at each documented capacity the call is served and right; one beyond it is refused, never answered"""
    import pytest
    import torch
    from deeprank_gnn_amd._lib import DrgnnError
    from deeprank_gnn_amd.interface import cluster_poses, pose_cluster_raw, pose_common_raw, pose_contacts
    rcap, pcap, ccap = api.fcc_capacity(0), api.fcc_capacity(1), api.fcc_capacity(2)
    assert rcap >= 2048 and pcap >= 4096 and ccap >= 1024 and api.fcc_capacity(3) == -1 and api.fcc_capacity(-1) == -1
    # residues of a complex
    fits = ladder_table(rcap - 65, 65)
    c = pose_contacts(fits, **kw(api, device))
    check_contacts(c, ref_maps(fits, fits.xyz[None]), "at the residue capacity")
    assert list(c.n_contacts) == [65] and [tuple(p) for p in c.pairs(0)] == [(i, rcap - 65 + i) for i in range(65)]
    with pytest.raises(DrgnnError, match="capacity"):
        pose_contacts(ladder_table(rcap - 64, 65), **kw(api, device))
    # poses on a side of a common call
    rng = np.random.default_rng(2)
    wa, wb = rng.integers(0, 2 ** 62, size=(pcap + 1, 3)), rng.integers(0, 2 ** 62, size=(2, 3))
    pop = lambda w: np.unpackbits(np.ascontiguousarray(w).view(np.uint8), axis=-1).sum(axis=-1)
    want = pop(wa[:, None, :] & wb[None, :, :]).astype(np.int32)
    da, db = torch.from_numpy(wa).to(device), torch.from_numpy(wb).to(device)
    assert np.array_equal(pose_common_raw(api, da[:pcap], db).cpu().numpy(), want[:pcap])
    assert np.array_equal(pose_common_raw(api, db, da[:pcap]).cpu().numpy(), want[:pcap].T)
    for args in ((da, db), (db, da)):
        with pytest.raises(DrgnnError, match="capacity"):
            pose_common_raw(api, *args)
    # poses of a cluster call: three groups and 96 poses alone
    group = np.concatenate((np.zeros(1500), np.full(ccap - 2096, 1), np.full(500, 2), 3 + np.arange(96))).astype(np.int64)
    group = group[rng.permutation(ccap)]
    common = np.where(group[:, None] == group[None, :], 9, 2).astype(np.int32)
    np.fill_diagonal(common, 10)
    n = np.full(ccap, 10, dtype=np.int32)
    got = check_raw_cluster(api, device, common, n, what="at the cluster capacity")
    assert sorted(got["sizes"].tolist()) == sorted([1500, ccap - 2096, 500]) and (got["labels"] == -1).sum() == 96
    big = np.full((ccap + 1, ccap + 1), 10, dtype=np.int32)
    with pytest.raises(DrgnnError, match="capacity"):
        pose_cluster_raw(api, big, np.full(ccap + 1, 10, dtype=np.int32), device=device)


def check_common_is_split(api, device, monkeypatch):
    """common_contacts splits its calls at the capacity: the same matrix through blocks of at most 5 x 5 poses"""
    from deeprank_gnn_amd.interface import AtomTable, common_contacts, pose_contacts
    table, xyz = family_batch()
    c = pose_contacts(AtomTable.poses(table, xyz[:17]), **kw(api, device))
    whole = common_contacts(c)
    assert np.array_equal(whole, family_ref()[1][:17, :17])
    monkeypatch.setattr(type(api), "fcc_capacity", lambda self, what: 5 if what == 1 else 4096)
    assert same_bits(common_contacts(c), whole) and same_bits(common_contacts(c, c), whole)


def check_empty_batch(api, device):
    from deeprank_gnn_amd.interface import AtomTable, cluster_poses, common_contacts, fcc_matrix, pose_contacts
    table, xyz = family_batch()
    c = pose_contacts(AtomTable.poses(table, xyz[:0]), **kw(api, device))
    assert len(c) == 0 and c.n_contacts.shape == (0,) and c.words().shape == (0, table.split, (table.n_residues - table.split + 63) // 64)
    assert common_contacts(c).shape == (0, 0) and fcc_matrix(c).shape == (0, 0)
    some = pose_contacts(AtomTable.poses(table, xyz[:3]), **kw(api, device))
    assert common_contacts(c, some).shape == (0, 3) and common_contacts(some, c).shape == (3, 0)
    r = cluster_poses(c)
    assert r.labels.shape == (0,) and r.centres.shape == (0,) and r.sizes.shape == (0,) and len(r) == 0
    assert r.rank(np.zeros(0))[0].shape == (0,)
    # no launch: a library that cannot be called at all serves the empty batch
    r = cluster_poses(AtomTable.poses(table, xyz[:0]), api=NoLaunch(api), device=device)
    assert len(r) == 0 and r.labels.shape == (0,)


class NoLaunch(object):
    """an api that answers capacities and fails on every call that would launch"""

    def __init__(self, api):
        self.fcc_capacity, self.rmsd_capacity = api.fcc_capacity, api.rmsd_capacity


def check_value_errors():
    """the Python side refuses before anything is uploaded (api=object() would fail at the first call)"""
    import pytest
    from deeprank_gnn_amd.interface import AtomTable, cluster_poses, common_contacts, pose_contacts
    atoms, xyz = no_contact_batch()
    kwargs = {"api": object(), "device": "cpu"}
    good = atoms.table()
    bare = AtomTable(atoms.chain, atoms.seq, atoms.res_name, atoms.xyz)
    other = atoms.table()
    poses = AtomTable.poses(good, xyz)
    for bad in (0.0, -5.0, float("nan")):
        with pytest.raises(ValueError, match="cutoff"):
            pose_contacts(poses, cutoff=bad, **kwargs)
        with pytest.raises(ValueError, match="cutoff"):
            cluster_poses(poses, cutoff=bad, **kwargs)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="cutoff_fcc"):
            cluster_poses(poses, cutoff_fcc=bad, **kwargs)
        with pytest.raises(ValueError, match="strictness"):
            cluster_poses(poses, strictness=bad, **kwargs)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="min_size"):
            cluster_poses(poses, min_size=bad, **kwargs)
    with pytest.raises(ValueError, match="atom_name"):
        pose_contacts(bare, heavy_only=True, **kwargs)
    with pytest.raises(ValueError, match="atom_name"):
        cluster_poses(AtomTable.poses(bare, xyz), heavy_only=True, **kwargs)
    with pytest.raises(ValueError, match="given AtomTable"):
        pose_contacts(poses, table=other, **kwargs)
    with pytest.raises(ValueError, match="xyz"):
        pose_contacts(poses.xyz[:, :-1], table=good, **kwargs)
    with pytest.raises(ValueError, match="table="):
        pose_contacts(poses.xyz, **kwargs)
    with pytest.raises(ValueError, match="PoseContacts"):
        common_contacts(poses)


REQUESTS = {
    "contacts": ("PoseContactsRequest", "pose_contacts", "drgnn_pose_contacts"),
    "common": ("PoseCommonRequest", "pose_common", "drgnn_pose_common"),
    "cluster": ("PoseClusterRequest", "pose_cluster", "drgnn_pose_cluster"),
}


def refusal_cases():
    """(entry point, name) -> what to change in a good request; "tab_atom_ptr": the host table"""
    t = no_contact_batch()[0].table()
    ap = t.atom_ptr.astype(np.int32)

    def put(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    nan, inf = float("nan"), float("inf")
    cases = {("contacts", "null " + k): {k: None} for k in ("xyz", "atom_ptr", "host_atom_ptr", "bits", "n_contacts")}
    cases.update({("contacts", k): v for k, v in {
        "n_poses negative": {"n_poses": -1}, "n_atoms negative": {"n_atoms": -1}, "n_residues negative": {"n_residues": -1},
        "n_chain_a negative": {"n_chain_a": -1}, "n_chain_a past the residues": {"n_chain_a": t.n_residues + 1},
        "atom_ptr starts at 1": {"tab_atom_ptr": put(ap, 0, 1)}, "atom_ptr decreases": {"tab_atom_ptr": put(ap, 2, ap[1] - 1)},
        "atom_ptr ends past the atoms": {"tab_atom_ptr": put(ap, t.n_residues, t.n_atoms + 1)},
        "n_atoms is not where atom_ptr ends": {"n_atoms": t.n_atoms - 1},
        "cutoff 0": {"cutoff": 0.0}, "cutoff negative": {"cutoff": -5.0}, "cutoff NaN": {"cutoff": nan}, "cutoff inf": {"cutoff": inf},
    }.items()})
    cases.update({("common", "null " + k): {k: None} for k in ("bits_a", "bits_b", "common")})
    cases.update({("common", k): v for k, v in {"n_a negative": {"n_a": -1}, "n_b negative": {"n_b": -1},
                                                "n_words negative": {"n_words": -1}}.items()})
    cases.update({("cluster", "null " + k): {k: None} for k in ("common", "n_contacts", "neighbours", "transposed", "labels",
                                                               "centres", "sizes", "n_clusters")})
    cases.update({("cluster", k): v for k, v in {
        "n_poses negative": {"n_poses": -1}, "min_size 0": {"min_size": 0}, "min_size negative": {"min_size": -3},
        "cutoff_fcc 0": {"cutoff_fcc": 0.0}, "cutoff_fcc above 1": {"cutoff_fcc": 1.5}, "cutoff_fcc NaN": {"cutoff_fcc": nan},
        "cutoff_reverse 0": {"cutoff_reverse": 0.0}, "cutoff_reverse above 1": {"cutoff_reverse": 1.0000001},
        "cutoff_reverse NaN": {"cutoff_reverse": nan}, "cutoff_reverse negative": {"cutoff_reverse": -0.45},
    }.items()})
    for entry in REQUESTS:
        cases[entry, "capacity"] = None
        cases[entry, "null request"] = None
    return cases


def refusal_names():
    return sorted("%s: %s" % k for k in refusal_cases())


FILL = -7


def check_refusal(api, device, name):
    """one malformed field: refused on the host, before a launch (the outputs keep their fill); the good request then runs"""
    import pytest
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._lib import DrgnnError
    from deeprank_gnn_amd.interface import AtomTable
    entry, what = name.split(": ", 1)
    over = refusal_cases()[entry, what]
    atoms, xyz = no_contact_batch()
    t = atoms.table()
    poses = AtomTable.poses(t, xyz)
    maps = ref_maps(t, poses.xyz, False)
    common, M = R.common_of(maps), 3
    n = np.diag(common).astype(np.int32)
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nA, WB = t.split, (t.n_residues - t.split + 63) // 64
    ap = t.atom_ptr.astype(np.int32)
    d = {"xyz": up(poses.xyz), "atom_ptr": up(ap)}
    bits = torch.full((M, nA, WB), FILL, dtype=torch.int64, device=dev)
    count = torch.full((M,), FILL, dtype=torch.int32, device=dev)
    good_bits = up(np.packbits(np.pad(maps, ((0, 0), (0, 0), (0, 64 * WB - maps.shape[2]))), axis=2, bitorder="little").view(np.int64))
    d_common = torch.full((M, M), FILL, dtype=torch.int32, device=dev)
    in_common, in_n = up(common), up(n)
    nb = torch.full((2, M, 1), FILL, dtype=torch.int64, device=dev)
    res = torch.full((3, M), FILL, dtype=torch.int32, device=dev)
    k = torch.full((1,), FILL, dtype=torch.int32, device=dev)
    outputs = {"contacts": (bits, count), "common": (d_common,), "cluster": (nb, res, k)}[entry]
    keep = []

    def request(**ch):
        q = getattr(_lib, REQUESTS[entry][0])()
        if entry == "contacts":
            host = np.ascontiguousarray(ch.pop("tab_atom_ptr", ap), dtype=np.int32)
            keep.append(host)
            q.xyz, q.atom_ptr, q.host_atom_ptr = d["xyz"].data_ptr(), d["atom_ptr"].data_ptr(), host.ctypes.data
            q.n_poses, q.n_atoms, q.n_residues, q.n_chain_a, q.cutoff = M, t.n_atoms, t.n_residues, nA, 5.0
            q.bits, q.n_contacts = bits.data_ptr(), count.data_ptr()
        elif entry == "common":
            q.bits_a = q.bits_b = good_bits.data_ptr()
            q.n_a, q.n_b, q.n_words, q.common = M, M, nA * WB, d_common.data_ptr()
        else:
            q.common, q.n_contacts, q.n_poses = in_common.data_ptr(), in_n.data_ptr(), M
            q.cutoff_fcc, q.cutoff_reverse, q.min_size = 0.6, 0.45, 2
            q.neighbours, q.transposed = nb[0].data_ptr(), nb[1].data_ptr()
            q.labels, q.centres, q.sizes, q.n_clusters = res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), k.data_ptr()
        for key, v in ch.items():
            setattr(q, key, v)
        return q

    call = getattr(api, REQUESTS[entry][1])
    stream = _lib.current_stream(d["xyz"])
    if what == "capacity":
        beyond = {"contacts": {"n_residues": api.fcc_capacity(0) + 1}, "common": {"n_b": api.fcc_capacity(1) + 1},
                  "cluster": {"n_poses": api.fcc_capacity(2) + 1}}[entry]
        with pytest.raises(DrgnnError, match="capacity"):
            call(request(**beyond), stream)
    elif what == "null request":
        with pytest.raises(DrgnnError, match="bad argument"):
            _lib._check(getattr(api.lib, REQUESTS[entry][2])(None, stream), REQUESTS[entry][2])
    else:
        with pytest.raises(DrgnnError, match="bad argument"):
            call(request(**dict(over)), stream)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert all(bool((o == FILL).all()) for o in outputs)              # nothing was launched
    call(request(), stream)                                           # and the good request runs
    if entry == "contacts":
        assert np.array_equal(bits.cpu().numpy(), good_bits.cpu().numpy()) and np.array_equal(count.cpu().numpy(), n)
    elif entry == "common":
        assert np.array_equal(d_common.cpu().numpy(), common)
    else:
        labels, centres, sizes, _ = R.cluster(R.neighbours_of(common, n), 2)
        K = int(k.cpu()[0])
        got = res.cpu().numpy()
        assert K == len(centres) and np.array_equal(got[0], labels) and np.array_equal(got[1, :K], centres) and np.array_equal(got[2, :K], sizes)
        assert np.array_equal(unpack(nb[0].cpu().numpy().view(np.uint64), M), R.neighbours_of(common, n))


# ---- 7 PoseClusters.rank -----------------------------------------------------------------------------------------------
def check_rank():
    import pytest
    from deeprank_gnn_amd.interface import PoseClusters
    labels = np.array([0, 0, 1, -1, 1, 0, 2, 0, 0, 1, -1, 2, 3])
    pc = PoseClusters(labels, np.array([0, 2, 6, 12]), np.array([5, 3, 2, 1]), np.zeros(13, np.int64))
    rng = np.random.default_rng(4)
    tied = np.array([0.5, 0.25, 0.75, 9.0, 0.25, 0.5, 0.5, 0.5, 0.125, 0.5, 9.0, 0.5, 0.5])      # clusters 2 and 3 tie at top = 2
    for scores in (rng.normal(size=13), tied, np.round(rng.normal(size=13), 1)):
        for top in (1, 2, 4, 7):                                       # 4 and 7: larger than some or all clusters
            for ascending in (False, True):
                order, means = pc.rank(scores, top=top, ascending=ascending)
                want_order, want_means = R.rank(labels, 4, scores, top, ascending)
                assert order.dtype == np.int64 and np.array_equal(order, want_order), (top, ascending, order, want_order)
                assert same_bits(means, want_means)
    order, means = pc.rank(tied, top=2)
    assert means[2] == means[3] == 0.5 and list(order).index(2) < list(order).index(3)          # a tie: the earlier cluster first
    assert list(pc.rank(tied, top=1, ascending=True)[0]) == [0, 1, 2, 3] and list(pc.rank(tied, top=1)[0]) == [1, 0, 2, 3]
    for bad in (np.zeros(12), np.zeros(14)):
        with pytest.raises(ValueError, match="scores"):
            pc.rank(bad)
