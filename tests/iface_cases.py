"""Inputs and checks shared by tests/test_iface.py (host emulation) and tests/test_gpu_iface.py (the device):
hand-made complexes on a 1/8 A grid (fp32 holds every coordinate, difference, square and sum exactly, so the kernels
must equal the float64 reference of tests/iface_ref.py in every bit), the four reference poses of 1ATN
(tests/golden/atoms_1ATN.npz) and the comparison against the graphs the reference generated from them
(tests/golden/fixture_1ATN.npz)."""
import os

import numpy as np

import iface_ref as R
from helpers import GOLDEN

STD = "ALA"
TREE_KEYS = ("nodes", "edge_index", "edge_data/dist", "internal_edge_index", "internal_edge_data/dist", "node_data/pos",
             "node_data/chain", "node_data/type", "node_data/polarity", "node_data/charge", "node_data/residue")


def table_of(residues):
    """AtomTable of [(chain, res_name, [[x, y, z], ...]), ...]; res_seq counts up within each chain"""
    from deeprank_gnn_amd.interface import AtomTable
    chain, seq, name, xyz, count = [], [], [], [], {}
    for ch, nm, atoms in residues:
        count[ch] = count.get(ch, 0) + 1
        for a in atoms:
            chain.append(ch); seq.append(count[ch]); name.append(nm); xyz.append(a)
    return AtomTable(np.array(chain), np.array(seq), np.array(name), np.array(xyz, dtype=np.float64).reshape(-1, 3))


def _blob(rng, n_atoms, centre, spread):
    """n_atoms points on the 1/8 grid within `spread` of centre"""
    return (np.round((np.asarray(centre) + rng.uniform(-spread, spread, (n_atoms, 3))) * 8) / 8).tolist()


def _random_complex(seed, n_a, n_b):
    """n_a + n_b residues of 1 - 6 atoms in two slabs 6 A apart: many interface pairs, some internal contacts"""
    rng = np.random.default_rng(seed)
    out = []
    for ch, n, x0 in (("A", n_a, -3.0), ("B", n_b, 3.0)):
        for k in range(n):
            centre = (x0, 2.5 * (k % 9), 2.5 * (k // 9))
            out.append((ch, RESNAMES[int(rng.integers(0, 20))], _blob(rng, int(rng.integers(1, 7)), centre, 1.5)))
    return out


RESNAMES = ("CYS", "HIS", "ASN", "GLN", "SER", "THR", "TYR", "TRP", "ALA", "PHE",
            "GLY", "ILE", "VAL", "MET", "PRO", "LEU", "GLU", "ASP", "LYS", "ARG")


def hand_cases():
    """[(name, residues)]"""
    rng = np.random.default_rng(5)
    big = _blob(rng, 70, (12.0, 0.0, 0.0), 3.0)                  # 70 atoms: more than a wave
    cases = [
        ("at_8.0", [("A", STD, [[0, 0, 0]]), ("B", STD, [[8.0, 0, 0]])]),
        ("at_8.5_exactly", [("A", STD, [[0, 0, 0]]), ("B", STD, [[8.5, 0, 0]])]),               # strict <: no edge
        ("no_contact", [("A", STD, [[0, 0, 0], [1, 0, 0]]), ("A", STD, [[0, 3, 0]]), ("B", STD, [[40, 0, 0]]),
                        ("B", STD, [[42.5, 1, 0]])]),
        ("chain_of_one", [("A", STD, [[0, 0, 0], [1.5, 0, 0]]), ("B", STD, [[5, 0, 0]]), ("B", STD, [[5, 2.5, 0]]),
                          ("B", STD, [[30, 0, 0]])]),
        ("one_atom_vs_70", [("A", STD, [[5.0, 0, 0]]), ("B", STD, big)]),
        ("70_vs_one_atom", [("A", STD, big), ("B", STD, [[5.0, 0, 0]]), ("B", STD, [[5.0, 1.0, 0]])]),
        # only the last atoms are within 8.5 A (7.0), every other pair is beyond
        ("last_atoms_closest", [("A", STD, [[-20, 0, 0], [-12, 5, 0], [0, 0, 0]]),
                                ("B", STD, [[30, 0, 0], [25, -5, 0], [19, 0, 0], [7, 0, 0]])]),
        # A1's only contact is the non-standard B1: A1 is no node; A2 - B2 stays
        ("non_standard", [("A", STD, [[0, 0, 0]]), ("A", "GLY", [[0, 30, 0]]), ("B", "HOH", [[4, 0, 0]]),
                          ("B", "SER", [[4, 30, 0]])]),
        # A1, A2 2.875 A apart, both within 8.5 A of B1: one internal edge
        ("internal_2.875", [("A", STD, [[0, 0, 0]]), ("A", STD, [[2.875, 0, 0]]), ("B", STD, [[8.0, 0, 0]])]),
        # the same pair with A2 beyond 8.5 A of B1 (10.875): A2 is no node, no internal edge
        ("internal_not_a_node", [("A", STD, [[0, 0, 0]]), ("A", STD, [[-2.875, 0, 0]]), ("B", STD, [[8.0, 0, 0]])]),
        ("internal_at_3.0_exactly", [("A", STD, [[0, 0, 0]]), ("A", STD, [[3.0, 0, 0]]), ("B", STD, [[8.0, 0, 0]])]),
    ]
    for n_a, n_b in ((1, 65), (63, 64), (64, 63), (65, 1), (65, 65)):
        cases.append(("random_%dx%d" % (n_a, n_b), _random_complex(100 + n_a + 7 * n_b, n_a, n_b)))
    return cases


EXPECT = {"at_8.0": (2, 1, 0), "at_8.5_exactly": (0, 0, 0), "no_contact": (0, 0, 0), "chain_of_one": (3, 2, 1),
          "one_atom_vs_70": (2, 1, 0), "70_vs_one_atom": (3, 2, 1), "last_atoms_closest": (2, 1, 0),
          "non_standard": (2, 1, 0), "internal_2.875": (3, 2, 1), "internal_not_a_node": (2, 1, 0),
          "internal_at_3.0_exactly": (3, 2, 0)}          # (nodes, interface edges, internal edges), worked out by hand


def reference_tree(table, xyz=None):
    """the reference result of one complex as the arrays the store holds (geometry only), fp32 / int64"""
    g = R.as_fp32(R.interface_graph(table.xyz if xyz is None else xyz, table.atom_ptr, table.split, table.res_type))
    return {"edge_index": g["edge_index"], "edge_data/dist": g["dist"], "internal_edge_index": g["internal_edge_index"],
            "internal_edge_data/dist": g["internal_dist"], "node_data/pos": g["pos"], "node_data/chain": g["chain"],
            "node_data/residue": g["node_residue"], "node_data/type": np.eye(20, dtype=np.float32)[g["type"]]}


def assert_tree_equals_reference(store, mol, ref):
    for k, want in ref.items():
        got = store.get(mol, k)
        assert got.dtype == want.dtype and got.shape == want.shape, (mol, k, got.dtype, got.shape, want.dtype, want.shape)
        assert got.tobytes() == want.tobytes(), (mol, k, got, want)


def assert_stores_identical(a, mols_a, b, mols_b):
    """every dataset of the listed molecules, bit for bit"""
    for ma, mb in zip(mols_a, mols_b):
        assert sorted(a._mols[ma]) == sorted(b._mols[mb]) and set(TREE_KEYS) <= set(a._mols[ma]), (ma, mb)
        for k in a._mols[ma]:
            x, y = a.get(ma, k), b.get(mb, k)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (ma, mb, k)


# ---- 1ATN ------------------------------------------------------------------------------------------------------------
_ATN = None


def atn():
    """(AtomTable of pose 1w, xyz float64 [4, T, 3] in the file's atom order, the four names)"""
    global _ATN
    if _ATN is None:
        from deeprank_gnn_amd.interface import AtomTable
        with np.load(os.path.join(GOLDEN, "atoms_1ATN.npz")) as z:
            n = np.diff(z["atom_ptr"])
            chain = np.repeat(np.array(["A", "B"])[z["res_chain"]], n)
            seq = np.repeat(z["res_seq"], n)
            name = np.repeat(z["res_names"][z["res_name_index"]], n)
            xyz = z["xyz_milli"] / 1000.0
            _ATN = (AtomTable(chain, seq, name, xyz[0]), xyz, [str(m) for m in z["mols"]])
    return _ATN


def match_by_pos(pos, fixture_pos):
    """perm with fixture_pos[i] ~ pos[perm[i]] (within 1e-4 in every coordinate), a bijection"""
    d = np.abs(fixture_pos[:, None, :] - pos[None, :, :].astype(np.float64)).max(axis=2)
    perm = d.argmin(axis=1)
    assert pos.shape[0] == fixture_pos.shape[0], (pos.shape, fixture_pos.shape)
    assert d[np.arange(len(perm)), perm].max() <= 1e-4 and len(set(perm.tolist())) == len(perm)
    return perm


def assert_matches_fixture(store, mol, fixture):
    """issue test 2: node count and both edge sets exactly, dist / pos within 1e-4, chain equal"""
    fpos = fixture.get(mol, "node_data/pos")
    pos = store.get(mol, "node_data/pos")
    perm = match_by_pos(pos, fpos)                   # fixture node i is built node perm[i]
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))                 # built node -> fixture node
    assert np.abs(pos[perm] - fpos).max() <= 1e-4
    np.testing.assert_array_equal(store.get(mol, "node_data/chain")[perm], fixture.get(mol, "node_data/chain"))
    for idx, dist in (("edge_index", "edge_data/dist"), ("internal_edge_index", "internal_edge_data/dist")):
        mine = {tuple(sorted(p)): float(d) for p, d in zip(inv[store.get(mol, idx)].tolist(), store.get(mol, dist))}
        theirs = {tuple(sorted(p)): float(d) for p, d in zip(fixture.get(mol, idx).tolist(), fixture.get(mol, dist))}
        assert len(mine) == store.get(mol, idx).shape[0] and len(theirs) == fixture.get(mol, idx).shape[0]
        assert set(mine) == set(theirs), (mol, idx, len(mine), len(theirs))
        err = max(abs(mine[p] - theirs[p]) for p in mine)
        print("%s %s: %d pairs, max |dist - fixture| = %.3g" % (mol, idx, len(mine), err))
        assert err <= 1e-4
    return perm


# ---- node feature tables (issue test 4) --------------------------------------------------------------------------------
# written out here, not read from the package: name -> (type, polarity class, charge); polarity 0 apolar, 1 polar,
# 2 negatively charged, 3 positively charged, as this reference version lists them (LYS among the negative ones).
# The committed fixture_1ATN.npz cannot serve: an older encoding wrote its `type` and `polarity` (scalars that reach
# 20 and -1).
TABLE = {"CYS": (0, 1, -0.64), "HIS": (1, 1, -0.29), "ASN": (2, 1, -1.22), "GLN": (3, 1, -1.22), "SER": (4, 1, -0.80),
         "THR": (5, 1, -0.80), "TYR": (6, 1, -0.80), "TRP": (7, 1, -0.79), "ALA": (8, 0, -0.37), "PHE": (9, 0, -0.37),
         "GLY": (10, 0, -0.37), "ILE": (11, 0, -0.37), "VAL": (12, 0, -0.37), "MET": (13, 0, -0.37), "PRO": (14, 0, 0.0),
         "LEU": (15, 0, -0.37), "GLU": (16, 2, -1.37), "ASP": (17, 2, -1.37), "LYS": (18, 2, -0.36), "ARG": (19, 3, -1.65)}


def table_complex():
    """20 one-atom residues, one of each name, ten per chain, every one a node"""
    names = sorted(TABLE)                               # (not in type order: the lookup is by name)
    res = [("A", nm, [[0.0, 1.0 * k, 0.0]]) for k, nm in enumerate(names[:10])]
    res += [("B", nm, [[4.0, 1.0 * k, 0.0]]) for k, nm in enumerate(names[10:])]
    return names, table_of(res)


def check_tables(api, device):
    from deeprank_gnn_amd.interface import interface_graphs
    names, t = table_complex()
    st = interface_graphs([t], ["all20"], api=api, device=device)
    assert st.get("all20", "node_data/residue").tolist() == list(range(20))
    typ, pol, chg = (st.get("all20", "node_data/" + k) for k in ("type", "polarity", "charge"))
    assert typ.shape == (20, 20) and pol.shape == (20, 4) and chg.shape == (20,)
    for k, nm in enumerate(names):
        want = TABLE[nm]
        assert typ[k].tolist() == [1.0 if i == want[0] else 0.0 for i in range(20)], nm
        assert pol[k].tolist() == [1.0 if i == want[1] else 0.0 for i in range(4)], nm
        assert chg[k] == want[2], nm
    assert [r.decode() for r in st.get("all20", "nodes")[:, 2]] == names


# ---- the checks both suites run ------------------------------------------------------------------------------------------
def check_hand_case(case, api, device):
    from deeprank_gnn_amd.interface import interface_graphs, build_ragged
    name, residues = case
    t = table_of(residues)
    st = interface_graphs([t], [name], api=api, device=device)
    ref = reference_tree(t)
    assert_tree_equals_reference(st, name, ref)
    if name in EXPECT:
        assert (ref["node_data/pos"].shape[0], ref["edge_index"].shape[0], ref["internal_edge_index"].shape[0]) == EXPECT[name]
    else:
        assert ref["edge_index"].shape[0] > 0 and (t.n_residues < 60 or ref["internal_edge_index"].shape[0] > 0)
    # B atoms through LDS in tiles of whole residues (6 atoms: the largest residue of the random cases), and a
    # workspace larger than needed: the same bits
    if name.startswith("random"):
        a = (t.xyz, t.atom_ptr, np.array([0, t.n_residues]), np.array([t.split]), t.res_type)
        whole = build_ragged(api, *a, device=device)
        tiled = build_ragged(api, *a, device=device, tile_atoms=6,
                             workspace_bytes=api.iface_workspace_bytes(3, 80, 90, 400))
        for k in whole:
            assert whole[k].tobytes() == tiled[k].tobytes(), (name, k)
        assert whole["dist"].tobytes() == ref["edge_data/dist"].tobytes()


def atn_batch(api, device):
    """the four poses (as AtomTable.poses) + every hand-made complex in one call: (store, names, items)"""
    from deeprank_gnn_amd.interface import AtomTable, interface_graphs
    t, xyz, mols = atn()
    cases = hand_cases()
    items = [AtomTable.poses(t, xyz)] + [table_of(r) for _, r in cases]
    names = mols + [n for n, _ in cases]
    return interface_graphs(items, names, api=api, device=device), names, items


def check_batch_independence(batch, api, device):
    """issue test 3: the batch equals each complex alone, chunk=1, and the poses given as separate tables"""
    from deeprank_gnn_amd.interface import AtomTable, interface_graphs
    store, names, items = batch
    t, xyz, mols = atn()
    one_by_one = interface_graphs(items, names, api=api, device=device, chunk=1)
    assert_stores_identical(store, names, one_by_one, names)
    for k in range(len(names)):                                    # each complex alone, through a call of its own
        it = AtomTable.poses(t, xyz[k:k + 1]) if k < 4 else items[1 + k - 4]
        alone = interface_graphs(it, [names[k]], api=api, device=device)
        assert_stores_identical(store, [names[k]], alone, [names[k]])
    # the poses as four tables of their own (grouped four times) in chunks of 3: poses must equal them
    tables = [AtomTable(*_per_atom(), xyz[m]) for m in range(4)]
    separate = interface_graphs(tables, mols, api=api, device=device, chunk=3)
    assert_stores_identical(store, mols, separate, mols)


def _per_atom():
    with np.load(os.path.join(GOLDEN, "atoms_1ATN.npz")) as z:
        n = np.diff(z["atom_ptr"])
        return (np.repeat(np.array(["A", "B"])[z["res_chain"]], n), np.repeat(z["res_seq"], n),
                np.repeat(z["res_names"][z["res_name_index"]], n))


def check_bad_input(api, device):
    """issue test 5: DRGNN_E_ARG for unsorted offset tables, DRGNN_E_CAPACITY for a small workspace; the checks are on the
    host tables, before any launch"""
    import pytest
    from deeprank_gnn_amd._lib import DrgnnError
    from deeprank_gnn_amd.interface import build_ragged
    t = table_of(hand_cases()[3][1])
    good = [t.xyz, t.atom_ptr.copy(), np.array([0, t.n_residues]), np.array([t.split]), t.res_type]
    build_ragged(api, *good, device=device)
    for which, bad in ((1, [0, 2, 1, 4, 5]), (1, [0, 2, 3, 4, 6]), (1, [1, 2, 3, 4, 5]), (2, [0, 5]), (2, [1, 4]), (3, [5])):
        a = list(good)
        a[which] = np.array(bad, dtype=np.int32)
        with pytest.raises(DrgnnError, match="bad argument"):
            build_ragged(api, *a, device=device)
    two = [np.concatenate((t.xyz, t.xyz)), np.concatenate((t.atom_ptr, t.atom_ptr[1:] + t.n_atoms)),
           np.array([0, 2 * t.n_residues + 1, 2 * t.n_residues]), np.array([1, t.n_residues + 1]), np.tile(t.res_type, 2)]
    with pytest.raises(DrgnnError, match="bad argument"):                # res_ptr not ascending
        build_ragged(api, *two, device=device)
    # an entry far beyond the tables in the middle of res_ptr (its ends are right): refused before anything is indexed
    # through it
    for mid in (2000000000, 2 * t.n_residues + 1, -1):
        far = list(two)
        far[2] = np.array([0, mid, 2 * t.n_residues])
        far[3] = np.array([1, 2 * t.n_residues])
        with pytest.raises(DrgnnError, match="bad argument"):
            build_ragged(api, *far, device=device)
    far = list(two)                                                      # the same for a split
    far[2], far[3] = np.array([0, t.n_residues, 2 * t.n_residues]), np.array([1, 2000000000])
    with pytest.raises(DrgnnError, match="bad argument"):
        build_ragged(api, *far, device=device)
    need = api.iface_workspace_bytes(1, 1, 3, 4)
    assert need > 0 and api.iface_workspace_bytes(-1, 1, 1, 1) == -1
    with pytest.raises(DrgnnError, match="capacity"):
        build_ragged(api, *good, device=device, workspace_bytes=need - 16)


# ---- end to end (issue GPU test 3) -----------------------------------------------------------------------------------------
def check_end_to_end(api, device, outdir, nn_kw=None):
    """The four poses built from atoms, put into the fixture's node order through the `pos` match and given the
    fixture's remaining node features and scores: PreCluster('mcl') must reproduce the fixture's depth_0 / depth_1, and
    the shipped regression checkpoint must score them like the fixture's own four graphs (1e-4: only the listing
    order of the edges differs)."""
    import torch
    from helpers import golden, params_of
    from deeprank_gnn_amd.clustering import PreCluster
    from deeprank_gnn_amd.dataset import GraphDataSet, GraphStore
    from deeprank_gnn_amd.ginet import GINet
    from deeprank_gnn_amd.interface import AtomTable, interface_graphs
    from deeprank_gnn_amd.NeuralNet import NeuralNet
    t, xyz, mols = atn()
    built = interface_graphs(AtomTable.poses(t, xyz), mols, api=api, device=device)
    fixture = GraphStore(os.path.join(GOLDEN, "fixture_1ATN.npz"))
    g = golden("pretrained_treg.npz")
    feats, target = [str(s) for s in g["node_feature"]], str(g["target_name"])
    mine, theirs = [], []
    for mol in mols:
        perm = match_by_pos(built.get(mol, "node_data/pos"), fixture.get(mol, "node_data/pos"))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        tree = {k: (v[perm] if k.startswith("node_data/") or k == "nodes" else v) for k, v in built._mols[mol].items()}
        tree["edge_index"] = inv[built.get(mol, "edge_index")]
        tree["internal_edge_index"] = inv[built.get(mol, "internal_edge_index")]
        other = {k: v for k, v in fixture._mols[mol].items() if not k.startswith("clustering/")}
        for k, v in other.items():
            if (k.startswith("node_data/") and k not in tree) or k.startswith("score/"):
                tree[k] = v
        # (an older encoding wrote the fixture's scalar type / polarity: both sides read the tables' one-hot rows)
        other["node_data/type"], other["node_data/polarity"] = tree["node_data/type"], tree["node_data/polarity"]
        for k in ("depth_0", "depth_1"):
            other["clustering/mcl/" + k] = fixture.get(mol, "clustering/mcl/" + k)
        mine.append(tree)
        theirs.append(other)
    a, b = GraphStore.from_trees(mols, mine), GraphStore.from_trees(mols, theirs)
    PreCluster(GraphDataSet(a, node_feature=feats, edge_feature=["dist"], target=target), method="mcl", api=api, device=device)
    for mol in mols:
        for k in ("clustering/mcl/depth_0", "clustering/mcl/depth_1"):
            np.testing.assert_array_equal(a.get(mol, k), fixture.get(mol, k), err_msg=mol + " " + k)
    ck = os.path.join(str(outdir), "treg.pth.tar")
    torch.save({'model': params_of(g), 'optimizer': {'state': {}, 'param_groups': [{'lr': 0.001, 'betas': (0.9, 0.999),
                                                                                  'eps': 1e-08, 'weight_decay': 0}]},
                'node': feats, 'edge': ['dist'], 'target': target, 'task': 'reg', 'classes': [0, 1], 'class_weight': None,
                'batch_size': 64, 'percent': [1.0, 0.0], 'lr': 0.001, 'index': None, 'shuffle': False, 'threshold': 0.3,
                'cluster_nodes': 'mcl', 'transform_sigmoid': False}, ck)
    out = []
    for st in (a, b):
        model = NeuralNet(st, GINet, pretrained_model=ck, outdir=str(outdir), **(nn_kw or {}))
        model.test(hdf5=None)
        out.append(np.asarray(model.test_out, dtype=np.float64).reshape(-1))
    print("predictions from atoms", out[0], "from the fixture", out[1])
    assert out[0].shape == (4,) and np.isfinite(out[0]).all()
    assert np.abs(out[0] - out[1]).max() <= 1e-4


def check_pose_batch(api, device):
    """issue GPU test 4: 64 poses of one topology, the four reference poses repeated, chain B of every second one
    moved rigidly by a multiple of 1/8 A.  The coordinates are first put on the 1/8 A grid, so that the moved ones
    stay exact in fp32 and the float64 reference sees the same numbers."""
    from deeprank_gnn_amd.interface import AtomTable, interface_graphs
    t, xyz, mols = atn()
    grid = np.round(xyz * 8) / 8
    in_b = np.zeros(t.n_input_atoms, dtype=bool)
    in_b[t.order[t.atom_ptr[t.split]:]] = True
    shifts = [np.array(s) for s in ((0.125, 0, 0), (0, -0.25, 0.125), (1.0, 0.5, -0.375), (-0.625, 0, 0.25))]
    poses = []
    for m in range(64):                              # poses 4 - 7, 12 - 15, ...: chain B moved
        x = grid[m % 4].copy()
        if (m // 4) % 2 == 1:
            x[in_b] += shifts[(m // 8) % 4] * (1 + m // 32)
        poses.append(x)
    names = ["pose%02d" % m for m in range(64)]
    store = interface_graphs(AtomTable.poses(t, np.stack(poses)), names, api=api, device=device)
    for m in (0, 3, 5, 30, 63):                                              # two still ones, three moved ones
        assert_tree_equals_reference(store, names[m], reference_tree(t, poses[m][t.order]))
    assert_stores_identical(store, names[0:4], store, names[8:12])          # a repeated still pose: the same graph
    for m in (5, 30, 63):                                                    # a moved copy is another graph
        still = store.get(names[m % 4], "edge_data/dist")
        got = store.get(names[m], "edge_data/dist")
        assert got.shape != still.shape or not np.array_equal(got, still), m


def check_empty_complexes(api, device):
    """complexes without a contact between others: 0 nodes, and the three offset tables do not advance"""
    from deeprank_gnn_amd.interface import build_ragged, _ragged
    cases = dict(hand_cases())
    tables = [table_of(cases[n]) for n in ("at_8.0", "no_contact", "at_8.5_exactly", "chain_of_one")]
    r = build_ragged(api, *_ragged([(t, t.xyz) for t in tables]), device=device)
    assert r["node_ptr"].tolist() == [0, 2, 2, 2, 5] and r["edge_ptr"].tolist() == [0, 1, 1, 1, 3]
    assert r["iedge_ptr"].tolist() == [0, 0, 0, 0, 1]
    assert r["edge_index"].tolist() == [[0, 1], [0, 1], [0, 2]] and r["internal_edge_index"].tolist() == [[1, 2]]
    none = build_ragged(api, *_ragged([(tables[1], tables[1].xyz)]), device=device)
    assert none["node_ptr"].tolist() == [0, 0] and none["edge_ptr"].tolist() == [0, 0] and none["iedge_ptr"].tolist() == [0, 0]
    assert none["pos"].shape == (0, 3)
