"""Inputs and checks shared by tests/test_pack.py (host emulation) and tests/test_gpu_pack.py (the device):
interface_resident_set and drgnn_iface_pack against the existing path on the same inputs,

    interface_graphs -> attach_residue_features -> GraphDataSet(same node_feature order) -> PreCluster -> ResidentGraphSet

bit for bit in every array but edge_attr with the default transform, which the store path evaluates in float32 and the
kernel in float64 (bounds below)."""
import os

import numpy as np
import torch

import iface_cases as IC
import score_cases as SC
from helpers import GOLDEN

ARRAYS = ("node_ptr", "edge_ptr", "c1_ptr", "x", "edge_index", "cluster0", "cluster1")
ALL_FEATURES = ["hse", "type", "pssm", "pos", "bsa", "chain", "ic", "polarity", "charge"]      # scrambled, every source
NO_BSA = [f for f in ALL_FEATURES if f != "bsa"]
# edge_attr, default transform.  Against np.float32(np.tanh(-d.astype(np.float64)/2 + 2) + 1): 1 ulp of float32 (the fp64
# evaluation errs by a few fp64 ulps, which can move the final rounding across one boundary at most).  Against the store
# path's float32 evaluation: 2^-21 absolute (argument off by at most 2 * 2^-23, slope of tanh at most 1, numpy's float32
# tanh within a few ulp of a value below 1, the last addition 2^-24)
ATTR_ABS = 2.0 ** -21


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.dtype, a.shape, a.tobytes()


def same(a, b):
    return bits(a) == bits(b)


def assert_sets_equal(got, want, what="", attr="bits"):
    """every array of two resident sets; attr: 'bits', 'default' (the two bounds above) or None"""
    assert got.mols == want.mols, (what, got.mols, want.mols)
    for k in ARRAYS:
        assert same(getattr(got, k), getattr(want, k)), (what, k, getattr(got, k), getattr(want, k))
    assert (got.y is None) == (want.y is None)
    if got.y is not None:
        assert same(got.y, want.y) and same(got.y_host, want.y_host), (what, got.y, want.y)
    if attr == "bits":
        assert same(got.edge_attr, want.edge_attr), what
    elif attr == "default":
        g, w = got.edge_attr.cpu().numpy(), want.edge_attr.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype == np.float32
        err = float(np.abs(g.astype(np.float64) - w).max()) if g.size else 0.0
        print("%s: max |edge_attr - store path| = %.3g (bound %.3g)" % (what, err, ATTR_ABS))
        assert err <= ATTR_ABS


def oracle(items, names, node_feature, api, device, residue_features=None, reference=None, target=None, method="mcl",
           bsa=False, hse=False, transform="default"):
    """(ResidentGraphSet of the existing path over the complexes with a node, the names of the others)"""
    from deeprank_gnn_amd.clustering import PreCluster
    from deeprank_gnn_amd.dataset import GraphDataSet, GraphStore, default_edge_transform
    from deeprank_gnn_amd.interface import attach_residue_features, interface_graphs
    from deeprank_gnn_amd.resident import ResidentGraphSet
    store = interface_graphs(items, names, api=api, device=device, reference=reference, bsa=bsa, hse=hse)
    keep = [n for n in names if store.get(n, "node_data/pos").shape[0] > 0]
    sub = GraphStore.from_trees(keep, [store._mols[n] for n in keep])
    for k, tab in (residue_features or {}).items():
        attach_residue_features(sub, k, tab)
    ds = GraphDataSet(sub, node_feature=list(node_feature), edge_feature=["dist"], target=target, clustering_method=method,
                      edge_feature_transform=default_edge_transform if transform == "default" else (lambda d: d))
    PreCluster(ds, method=method, api=api, device=device)
    return ResidentGraphSet(ds, device, api=api), [n for n in names if n not in keep], ds


# ---- 1 hand-made complexes ----------------------------------------------------------------------------------------------
def hand_batch():
    """(tables, names): the hand-made complexes of iface_cases, the two empty ones between two others"""
    cases = dict(IC.hand_cases())
    order = ["at_8.0", "no_contact", "at_8.5_exactly", "chain_of_one"] + [n for n in cases if n not in
                                                                        ("at_8.0", "no_contact", "at_8.5_exactly", "chain_of_one")]
    return [IC.table_of(cases[n]) for n in order], order


HAND_FEATURES = ["chain", "type", "pos", "w", "charge", "polarity"]


def hand_tables(tables, names):
    """a residue feature per complex: {mol: float64 [R]}"""
    rng = np.random.default_rng(11)
    return {"w": {n: rng.normal(size=t.n_residues) for t, n in zip(tables, names)}}


def check_hand(api, device):
    from deeprank_gnn_amd.interface import interface_resident_set
    tables, names = hand_batch()
    feats = hand_tables(tables, names)
    for method in ("mcl", "louvain"):
        want, skipped, _ = oracle(tables, names, HAND_FEATURES, api, device, residue_features=feats, method=method)
        got = interface_resident_set(tables, names, node_feature=HAND_FEATURES, residue_features=feats,
                                     clustering_method=method, api=api, device=device)
        assert got.skipped == skipped == ["no_contact", "at_8.5_exactly"]
        assert_sets_equal(got, want, "hand " + method, attr="default")
        k = got.mols.index("chain_of_one")                            # right after the empty ones: the offsets did not advance
        assert got.node_ptr[:3].tolist() == [0, 2, 5] and got.edge_ptr[:3].tolist() == [0, 2, 6] and k == 1
    two = got.mols.index("at_8.0")                                     # two nodes, one edge, no internal edge
    assert got.n_nodes[two] == 2 and got.n_edges[two] == 2
    raw = interface_resident_set(tables, names, node_feature=HAND_FEATURES, residue_features=feats, edge_transform=None,
                                 chunk=5, api=api, device=device)
    want_raw, _, _ = oracle(tables, names, HAND_FEATURES, api, device, residue_features=feats, transform=None)
    assert_sets_equal(raw, want_raw, "hand raw distances, chunk 5", attr="bits")
    none = interface_resident_set(tables, names, node_feature=HAND_FEATURES, residue_features=feats, edge_feature=None,
                                  api=api, device=device)
    assert none.edge_attr is None and not none.has_attr and same(none.x, got.x)
    empty = interface_resident_set(tables[1:3], names[1:3], node_feature=["type"], api=api, device=device)
    assert len(empty) == 0 and empty.skipped == names[1:3] and tuple(empty.x.shape) == (0, 20)


def raw_pack(api, device, tables, cols, edge_mode=1, **kw):
    """(built, ptrs on the host, outputs) of one direct drgnn_iface_pack call over the builder's output of ``tables``"""
    from deeprank_gnn_amd import interface as I
    xyz, atom_ptr, res_ptr, split, res_type = I._ragged([(t, t.xyz) for t in tables])
    built, ptrs = I.build_ragged_device(api, xyz, atom_ptr, res_ptr, split, res_type, device=device)
    table = torch.from_numpy(I.pack_type_table()).to(ptrs.device)
    out = I.iface_pack_raw(api, built, ptrs, cols, len(atom_ptr) - 1, type_table=table, edge_mode=edge_mode, **kw)
    return built, ptrs.cpu().numpy(), out


def check_raw_outputs(api, device):
    """the batch vector, the global internal edges and the two edge layouts of one direct call; an empty batch"""
    from deeprank_gnn_amd import _lib
    tables, names = hand_batch()
    cols = [(_lib.PACK_CHAIN, 0), (_lib.PACK_POS, 2), (_lib.PACK_TYPE, 24)]
    built, p, out = raw_pack(api, device, tables, cols, edge_mode=0)
    b = {k: v.cpu().numpy() for k, v in built.items()}
    o = {k: v.cpu().numpy() for k, v in out.items()}
    M = len(tables)
    assert o["batch"].tolist() == np.repeat(np.arange(M), np.diff(p[0])).tolist() and o["batch"].dtype == np.int64
    ei, ie, ea = [], [], []
    for k in range(M):
        pairs = b["edge_index"][p[1, k]:p[1, k + 1]]
        ei.append(np.vstack((pairs, pairs[:, ::-1])).T)
        d = b["dist"][p[1, k]:p[1, k + 1]]
        ea.append(np.concatenate((d, d)))
        pairs = b["internal_edge_index"][p[2, k]:p[2, k + 1]] + p[0, k]
        ie.append(np.vstack((pairs, pairs[:, ::-1])).T)
    assert same(o["edge_index"], np.ascontiguousarray(np.hstack(ei))) and same(o["edge_attr"], np.concatenate(ea))
    assert same(o["internal_edge_index"], np.ascontiguousarray(np.hstack(ie)))
    from deeprank_gnn_amd.interface import RESIDUE_CHARGE
    want_x = np.stack((b["chain"].astype(np.float32), b["pos"][:, 2], RESIDUE_CHARGE[b["type"]].astype(np.float32)), axis=1)
    assert same(o["x"], want_x)
    _, p0, out0 = raw_pack(api, device, tables[1:3], cols)                # nothing but empty complexes
    assert p0[:, -1].tolist() == [0, 0, 0] and all(v.numel() == 0 for v in out0.values())
    from deeprank_gnn_amd import interface as I                          # no complex at all
    dev = out["x"].device
    none = {k: torch.empty((0,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev) for k, v in built.items()}
    out1 = I.iface_pack_raw(api, none, torch.zeros((3, 1), dtype=torch.int32, device=dev), cols, 0,
                            type_table=torch.from_numpy(I.pack_type_table()).to(dev))
    assert all(v.numel() == 0 for v in out1.values())


def f64_rows(n):
    """(depth [n], bsa [n,3], hse [n,3]) float64, one row per node: values exactly halfway between two floats (round to
    nearest even takes 1 + 2^-24 down to 1 and 1 + 3 * 2^-24 up to 1 + 2^-22), a negative value, a float32 denormal, a
    float64 denormal (0 as a float) and ordinary values; one hse row whose first entry is NaN"""
    special = np.array([1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -2.5 - 2.0 ** -30, 1e-40, 1e-310, 7.25, -(1 + 2.0 ** -24), 1 / 3])
    depth = special[np.arange(n) % 8]
    bsa = special[(np.arange(3 * n).reshape(n, 3) * 5 + 1) % 8]
    hse = special[(np.arange(3 * n).reshape(n, 3) * 3 + 2) % 8]
    hse[n // 2, 0] = np.nan
    return depth, bsa, hse


def check_f64_sources(api, device):
    """depth, bsa and hse columns among chain columns, in scrambled order: every float64 is rounded once, to nearest even"""
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd import interface as I
    P = _lib
    tables, names = hand_batch()                                       # (two of the complexes have no node)
    xyz, atom_ptr, res_ptr, split, res_type = I._ragged([(t, t.xyz) for t in tables])
    built, ptrs = I.build_ragged_device(api, xyz, atom_ptr, res_ptr, split, res_type, device=device)
    n = int(built["pos"].shape[0])
    assert n > 8 and int(np.diff(ptrs[0].cpu().numpy()).max()) >= 3
    depth, bsa, hse = f64_rows(n)
    rows = {k: torch.from_numpy(v).to(ptrs.device) for k, v in (("depth", depth), ("bsa", bsa), ("hse", hse))}
    zeroed = np.where(np.isnan(hse[:, :1]), 0.0, hse)
    source = {P.PACK_DEPTH: depth[:, None], P.PACK_BSA: bsa, P.PACK_HSE: zeroed,
              P.PACK_CHAIN: built["chain"].cpu().numpy().astype(np.float64)[:, None]}
    seven = [(P.PACK_HSE, 2), (P.PACK_DEPTH, 0), (P.PACK_CHAIN, 0), (P.PACK_BSA, 2), (P.PACK_HSE, 0), (P.PACK_BSA, 0), (P.PACK_HSE, 1)]
    # 91 columns: 256 = 2 * 91 + 74, so a lane's column wraps as it steps, and a complex of three nodes takes two steps
    for cols in (seven * 13, [(P.PACK_DEPTH, 0), (P.PACK_CHAIN, 0), (P.PACK_DEPTH, 0)]):
        assert 256 % len(cols) != 0
        x = I.iface_pack_raw(api, built, ptrs, cols, len(atom_ptr) - 1, want=("x",), **rows)["x"]
        want = np.stack([source[s][:, c].astype(np.float32) for s, c in cols], axis=1)
        assert same(x, want), (len(cols), x, want)
    x = x.cpu().numpy()                                                # depth listed twice: two equal columns
    assert same(x[:, 0].copy(), x[:, 2].copy()) and same(x[:, 0].copy(), depth.astype(np.float32))
    assert np.float32(1 + 2.0 ** -24) == 1 and np.float32(1 + 3 * 2.0 ** -24) == np.float32(1 + 2.0 ** -22)
    assert 0 < abs(np.float32(1e-40)) < np.finfo(np.float32).tiny and np.float32(1e-310) == 0


def check_depth_argument(api, device):
    """a wrongly shaped ``depth=`` is refused by pack_request before any call"""
    import pytest
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd import interface as I
    cases = dict(IC.hand_cases())
    t = IC.table_of(cases["chain_of_one"])
    xyz, atom_ptr, res_ptr, split, res_type = I._ragged([(t, t.xyz)])
    built, ptrs = I.build_ragged_device(api, xyz, atom_ptr, res_ptr, split, res_type, device=device)
    n, dev = int(built["pos"].shape[0]), ptrs.device
    assert n == 3
    good = torch.zeros(n, dtype=torch.float64, device=dev)
    I.pack_request(built, ptrs, [(_lib.PACK_DEPTH, 0)], len(atom_ptr) - 1, depth=good)
    for bad in (torch.zeros(n + 1, dtype=torch.float64, device=dev), torch.zeros((n, 1), dtype=torch.float64, device=dev),
                good.to(torch.float32), torch.zeros(2 * n, dtype=torch.float64, device=dev)[::2]):
        with pytest.raises(ValueError, match="depth must be float64"):
            I.pack_request(built, ptrs, [(_lib.PACK_DEPTH, 0)], len(atom_ptr) - 1, depth=bad)


# ---- 2 1ATN ---------------------------------------------------------------------------------------------------------------
def atn_tables():
    rng = np.random.default_rng(627)
    return {"pssm": rng.normal(size=(627, 20)), "ic": rng.uniform(0.0, 3.0, size=627)}


_ORACLE = {}


def atn_sets(api, device, poses, features, method):
    """(the packed set, the oracle's set) of 1ATN poses with the bound complex as reference and irmsd as target; the
    oracle is computed once per request and left unchanged"""
    from deeprank_gnn_amd.interface import AtomTable, interface_resident_set
    case, record = SC.atn()
    mols = [record["mols"][m] for m in poses]
    batch = AtomTable.poses(case.table, np.stack([case.poses[m] for m in poses]))
    feats = atn_tables()
    assert case.table.n_residues == 627
    key = (id(api), str(device), tuple(poses), tuple(features), method)
    if key not in _ORACLE:
        _ORACLE[key] = oracle(batch, mols, features, api, device, residue_features=feats, reference=case.sref, target="irmsd",
                              method=method, bsa="bsa" in features, hse="hse" in features)
    got = interface_resident_set(batch, mols, node_feature=features, residue_features=feats, reference=case.sref,
                                 target="irmsd", clustering_method=method, api=api, device=device)
    return got, _ORACLE[key][0]


def check_atn(api, device, poses, features, method):
    from deeprank_gnn_amd.dataset import GraphStore
    got, want = atn_sets(api, device, poses, features, method)
    width = {"hse": 3, "type": 20, "pssm": 20, "pos": 3, "polarity": 4}
    assert got.skipped == [] and got.n_feat == want.n_feat == sum(width.get(f, 1) for f in features)
    assert_sets_equal(got, want, "1ATN %s %s" % (method, list(poses)), attr="default")
    assert got.y.dtype == torch.float32 and got.y.numel() == len(poses)
    if method != "mcl":
        return
    # the fixture's recorded labels.  The nodes are listed in another order there, and a cluster's number is the place of
    # its first node, so the labels are compared through the node match by pos as partitions: cluster for cluster
    fixture = GraphStore(os.path.join(GOLDEN, "fixture_1ATN.npz"))
    at = sum(width.get(f, 1) for f in features[:features.index("pos")])
    x = got.x.cpu().numpy()
    c0, c1 = got.cluster0.cpu().numpy(), got.cluster1.cpu().numpy()
    for g, mol in enumerate(got.mols):
        n0, n1 = got.node_ptr[g:g + 2]
        perm = IC.match_by_pos(x[n0:n1, at:at + 3], fixture.get(mol, "node_data/pos"))
        mine0, theirs0 = c0[n0:n1][perm], fixture.get(mol, "clustering/mcl/depth_0")
        pairs = set(zip(mine0.tolist(), theirs0.tolist()))
        assert len(pairs) == len(set(mine0.tolist())) == len(set(theirs0.tolist())), (mol, "depth_0")
        to_fixture = dict(pairs)
        mine1, theirs1 = c1[got.c1_ptr[g]:got.c1_ptr[g + 1]], fixture.get(mol, "clustering/mcl/depth_1")
        assert len(mine1) == len(theirs1) == len(pairs)
        pairs1 = {(int(mine1[a]), int(theirs1[b])) for a, b in to_fixture.items()}
        assert len(pairs1) == len(set(mine1.tolist())) == len(set(theirs1.tolist())), (mol, "depth_1")


# ---- 3 independence -------------------------------------------------------------------------------------------------------
def pose_batch(n=64):
    """the poses of iface_cases.check_pose_batch: the four reference poses on the 1/8 A grid, repeated, chain B of every
    second group of four moved rigidly; (table, xyz [n, T, 3], names)"""
    t, xyz, _ = IC.atn()
    grid = np.round(xyz * 8) / 8
    in_b = np.zeros(t.n_input_atoms, dtype=bool)
    in_b[t.order[t.atom_ptr[t.split]:]] = True
    shifts = [np.array(s) for s in ((0.125, 0, 0), (0, -0.25, 0.125), (1.0, 0.5, -0.375), (-0.625, 0, 0.25))]
    poses = []
    for m in range(n):
        x = grid[m % 4].copy()
        k = m % 64
        if (k // 4) % 2 == 1:
            x[in_b] += shifts[(k // 8) % 4] * (1 + k // 32)
        poses.append(x)
    return t, np.stack(poses), ["pose%04d" % m for m in range(n)]


INDEP_FEATURES = ["pos", "pssm", "type", "chain", "charge"]


def check_independence(api, device, n=64):
    from deeprank_gnn_amd.interface import AtomTable, interface_resident_set
    t, xyz, names = pose_batch(n)
    feats = {"pssm": atn_tables()["pssm"]}

    def run(sel=None, **kw):
        sel = list(range(n)) if sel is None else sel
        return interface_resident_set(AtomTable.poses(t, xyz[sel]), [names[m] for m in sel], node_feature=INDEP_FEATURES,
                                      residue_features=feats, api=api, device=device, **kw)
    base = run(chunk=n)
    assert len(base) == n and base.skipped == []
    # (1 MiB of Markov-clustering workspace: runs of about four of these graphs instead of all of them at once)
    for what, other in (("second run, 1 MiB of MCL workspace", run(chunk=n, mcl_budget=1 << 20)),
                        ("chunk 1, 1 MiB of MCL workspace", run(chunk=1, mcl_budget=1 << 20)), ("chunk 3", run(chunk=3))):
        assert_sets_equal(other, base, what, attr="bits")
    sel = [5, 6, 30, n - 1, 0]
    sub = run(sel)
    assert sub.mols == [names[m] for m in sel]
    for key, ptr in (("x", "node_ptr"), ("cluster0", "node_ptr"), ("cluster1", "c1_ptr"), ("edge_attr", "edge_ptr"),
                     ("edge_index", "edge_ptr")):
        a, b = getattr(sub, key).cpu().numpy(), getattr(base, key).cpu().numpy()
        if key == "edge_index":
            a, b = a.T, b.T
        sp, bp = getattr(sub, ptr), getattr(base, ptr)
        for j, m in enumerate(sel):                                    # a pose's rows: the same alone as in the full batch
            assert same(np.ascontiguousarray(a[sp[j]:sp[j + 1]]), np.ascontiguousarray(b[bp[m]:bp[m + 1]])), (key, m)
    return base


# ---- 4 edge_attr -----------------------------------------------------------------------------------------------------------
def ulps32(a, b):
    """distance in units in the last place between float32 arrays of one sign"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_edge_attr(api, device):
    from deeprank_gnn_amd.interface import AtomTable, interface_resident_set
    t, xyz, names = pose_batch(8)
    batch = AtomTable.poses(t, xyz)
    kw = dict(node_feature=["type"], api=api, device=device)
    raw = interface_resident_set(batch, names, edge_transform=None, **kw)
    default = interface_resident_set(batch, names, **kw)
    want_raw, _, _ = oracle(batch, names, ["type"], api, device, transform=None)
    want, _, _ = oracle(batch, names, ["type"], api, device)
    assert same(raw.edge_attr, want_raw.edge_attr)                       # the distances, bit for bit
    d = raw.edge_attr.cpu().numpy()
    assert d.size > 1000 and d.min() > 0.3 and d.max() < 8.5
    stated = np.float32(np.tanh(-d.astype(np.float64) / 2 + 2) + 1)
    got = default.edge_attr.cpu().numpy()
    u = int(ulps32(got, stated).max())
    err = float(np.abs(got.astype(np.float64) - want.edge_attr.cpu().numpy()).max())
    print("edge_attr: %d edges, %d ulp from the float64 statement, %.3g from the store path" % (d.size, u, err))
    assert u <= 1
    assert err <= ATTR_ABS
    called = interface_resident_set(batch, names, edge_transform=lambda w: (w * 2.0 + 1.0).to(torch.float64), **kw)
    assert same(called.edge_attr, (raw.edge_attr * 2.0 + 1.0)) and called.edge_attr.dtype == torch.float32
    return raw, default


# ---- 5 scores --------------------------------------------------------------------------------------------------------------
def states(Net, F, K, seed):
    torch.manual_seed(seed)
    return [{k: v.clone() for k, v in Net(F, 1, 1).state_dict().items()} for _ in range(K)]


def check_scores(api, device, poses, features, outdir, nn_kw):
    from deeprank_gnn_amd import Ensemble, FoutNet, GINet, sGAT
    from deeprank_gnn_amd.NeuralNet import NeuralNet
    from deeprank_gnn_amd.resident import ResidentGraphSet
    got, want = atn_sets(api, device, poses, features, "mcl")
    _, _, ds = _ORACLE[(id(api), str(device), tuple(poses), tuple(features), "mcl")]
    F = got.n_feat
    path = os.path.join(str(outdir), "set.drgn")
    got.save_native(path)
    back = ResidentGraphSet.load_native(path, device, api=api)
    assert_sets_equal(back, got, "save_native / load_native", attr="bits")
    for Net, seed, exact in ((GINet, 3, True), (FoutNet, 4, True), (sGAT, 5, False)):
        ens = Ensemble(Net, states(Net, F, 2, seed), device=device, api=api)
        a, b, c = (ens.predict(s, cached=True).cpu().numpy() for s in (got, want, back))
        assert a.shape == (2, len(poses), 1) and np.isfinite(a).all()
        print("%s: max |packed - store path| = %.3g" % (Net.__name__, np.abs(a - b).max()))
        if exact:                                                       # their launches read no edge weight
            assert a.tobytes() == b.tobytes(), Net.__name__
        else:
            assert np.abs(a - b).max() <= 1e-4
        assert a.tobytes() == c.tobytes(), Net.__name__
    ck = os.path.join(str(outdir), "ginet.pth.tar")
    sd = states(GINet, F, 1, 9)[0]
    torch.save({'model': sd, 'optimizer': {'state': {}, 'param_groups': [{'lr': 0.001, 'betas': (0.9, 0.999), 'eps': 1e-08,
                                                                         'weight_decay': 0}]},
                'node': list(features), 'edge': ['dist'], 'target': 'irmsd', 'task': 'reg', 'classes': [0, 1],
                'class_weight': None, 'batch_size': 64, 'percent': [1.0, 0.0], 'lr': 0.001, 'index': None, 'shuffle': False,
                'threshold': 0.3, 'cluster_nodes': 'mcl', 'transform_sigmoid': False}, ck)
    store = ds.stores[0]
    outs = []
    for test_on in (store, got):
        model = NeuralNet(store, GINet, pretrained_model=ck, outdir=str(outdir), **nn_kw)
        model.test(database_test=test_on, hdf5=None)
        outs.append(np.asarray(model.test_out, dtype=np.float64).reshape(-1))
    assert outs[0].shape == (len(poses),) and outs[0].tobytes() == outs[1].tobytes(), outs
    import pytest
    from deeprank_gnn_amd.interface import AtomTable, interface_resident_set
    case, record = SC.atn()
    other = interface_resident_set(AtomTable.poses(case.table, np.stack(case.poses[:1])), ["p"], node_feature=["type"],
                                   api=api, device=device)
    with pytest.raises(ValueError, match="node feature columns"):
        model.test(database_test=other, hdf5=None)


# ---- 6 refusals and errors -------------------------------------------------------------------------------------------------
def refusal_cases():
    """{name: (edit of the request, 'bad argument' or 'capacity')}"""
    from deeprank_gnn_amd import _lib

    def cols_with(row):
        def edit(q, keep):
            bad = np.array([[_lib.PACK_CHAIN, 0], list(row)], dtype=np.int32)
            keep.append(bad)
            q.host_cols, q.n_cols = bad.ctypes.data, 2
        return edit

    def setter(**kw):
        def edit(q, keep):
            for k, v in kw.items():
                setattr(q, k, v)
        return edit
    def depth_column_1(q, keep):                                       # the array is there: only the column is wrong
        keep.append(torch.zeros(int(q.n_nodes), dtype=torch.float64, device=keep[1].device))
        q.depth = keep[-1].data_ptr()
        cols_with((_lib.PACK_DEPTH, 1))(q, keep)
    P = _lib
    return {
        "depth_is_null": (cols_with((P.PACK_DEPTH, 0)), "bad argument"),
        "column_outside_depth": (depth_column_1, "bad argument"),
        "null_node_ptr": (setter(node_ptr=None), "bad argument"),
        "null_edge_ptr": (setter(edge_ptr=None), "bad argument"),
        "null_iedge_ptr": (setter(iedge_ptr=None), "bad argument"),
        "null_cols": (setter(cols=None), "bad argument"),
        "null_host_cols": (setter(host_cols=None), "bad argument"),
        "null_edge_index": (setter(edge_index=None), "bad argument"),
        "null_dist": (setter(dist=None), "bad argument"),
        "null_internal_edge_index": (setter(internal_edge_index=None), "bad argument"),
        "unknown_source": (cols_with((7, 0)), "bad argument"),
        "negative_source": (cols_with((-1, 0)), "bad argument"),
        "column_outside_pos": (cols_with((P.PACK_POS, 3)), "bad argument"),
        "column_outside_type_table": (cols_with((P.PACK_TYPE, 25)), "bad argument"),
        "column_outside_res_feat": (cols_with((P.PACK_RES, 2)), "bad argument"),
        "negative_column": (cols_with((P.PACK_HSE, -1)), "bad argument"),
        "bsa_is_null": (cols_with((P.PACK_BSA, 2)), "bad argument"),
        "hse_is_null": (cols_with((P.PACK_HSE, 0)), "bad argument"),
        "type_table_is_null": (setter(type_table=None), "bad argument"),
        "res_feat_is_null": (setter(res_feat=None), "bad argument"),
        "pos_is_null": (setter(pos=None), "bad argument"),
        "n_rows_does_not_divide": (setter(n_rows=3), "bad argument"),
        "n_rows_zero": (setter(n_rows=0), "bad argument"),
        "negative_nodes": (setter(n_nodes=-1), "bad argument"),
        "negative_edges": (setter(n_edges=-1), "bad argument"),
        "negative_complexes": (setter(n_complexes=-1), "bad argument"),
        "negative_columns": (setter(n_cols=-1), "bad argument"),
        "edge_mode_2": (setter(edge_mode=2), "bad argument"),
        "edge_mode_negative": (setter(edge_mode=-1), "bad argument"),
        "too_many_complexes": (setter(n_complexes=65536), "capacity"),
        "too_many_columns": (setter(n_cols=257), "capacity"),
        "type_table_too_wide": (setter(type_width=65), "capacity"),
    }


def check_refusal(api, device, name):
    """the request of a good call with one thing wrong: refused, and the outputs, filled with a sentinel, are untouched"""
    import pytest
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd import interface as I
    cases = dict(IC.hand_cases())
    tables = [IC.table_of(cases[n]) for n in ("chain_of_one", "internal_2.875")]
    xyz, atom_ptr, res_ptr, split, res_type = I._ragged([(t, t.xyz) for t in tables])
    built, ptrs = I.build_ragged_device(api, xyz, atom_ptr, res_ptr, split, res_type, device=device)
    dev = ptrs.device
    R = len(atom_ptr) - 1
    N, E, Ei = (int(v) for v in ptrs[:, -1].cpu())
    assert (N, E, Ei) == (6, 4, 2) and R == 7
    cols = np.array([[_lib.PACK_TYPE, 3], [_lib.PACK_POS, 1], [_lib.PACK_CHAIN, 0], [_lib.PACK_RES, 1]], dtype=np.int32)
    keep = [cols, torch.from_numpy(cols).to(dev), torch.from_numpy(I.pack_type_table()).to(dev),
            torch.arange(2 * R, dtype=torch.float32, device=dev).reshape(R, 2)]
    outs = {"x": torch.full((N, 4), -7.0, device=dev), "edge_index_out": torch.full((2, 2 * E), -7, dtype=torch.int64, device=dev),
            "edge_attr": torch.full((2 * E,), -7.0, device=dev),
            "internal_edge_index_out": torch.full((2, 2 * Ei), -7, dtype=torch.int64, device=dev),
            "batch": torch.full((N,), -7, dtype=torch.int64, device=dev)}
    q = _lib.PackRequest()
    q.node_ptr, q.edge_ptr, q.iedge_ptr = (ptrs[i].data_ptr() for i in range(3))
    for k in ("node_residue", "chain", "type", "pos", "edge_index", "dist", "internal_edge_index"):
        setattr(q, k, built[k].data_ptr())
    q.cols, q.host_cols, q.type_table, q.res_feat = keep[1].data_ptr(), cols.ctypes.data, keep[2].data_ptr(), keep[3].data_ptr()
    q.n_complexes, q.n_nodes, q.n_edges, q.n_iedges, q.n_residues, q.n_rows = 2, N, E, Ei, R, R
    q.res_width, q.type_width, q.n_cols, q.edge_mode = 2, 25, 4, 1
    for k, v in outs.items():
        setattr(q, k, v.data_ptr())
    stream = _lib.current_stream(ptrs)
    if name == "good":
        api.iface_pack(q, stream)
        assert all(not (v == -7).any() for v in outs.values())
        return
    edit, kind = refusal_cases()[name]
    edit(q, keep)
    with pytest.raises(_lib.DrgnnError, match=kind):
        api.iface_pack(q, stream)
    if device != "cpu":
        torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == -7).all()), (name, k)


def check_capacity_values(api):
    assert [api.pack_capacity(w) for w in (0, 1, 2, 3, -1)] == [256, 64, 65535, -1, -1]


def check_value_errors(api, device):
    import pytest
    from deeprank_gnn_amd.interface import interface_resident_set
    tables, names = hand_batch()
    t2, n2 = tables[:2], names[:2]
    R = t2[0].n_residues

    def run(**kw):
        kw.setdefault("node_feature", ["type"])
        return interface_resident_set(t2, n2, api=api, device=device, **kw)
    for kw, match in (({"node_feature": "all"}, "node_feature"), ({"node_feature": []}, "node_feature"),
                      ({"node_feature": ["type", "depth"]}, "unknown node feature"),
                      ({"node_feature": ["pssm"], "residue_features": {"pssm": np.zeros((R + 1, 20))}}, "one row per residue"),
                      ({"node_feature": ["pssm"], "residue_features": {"pssm": np.zeros((R, 2, 2))}}, "one row per residue"),
                      ({"node_feature": ["pssm"], "residue_features": {"pssm": {n2[0]: np.zeros(R)}}}, "no table"),
                      ({"node_feature": ["bsa"], "bsa": False}, "bsa"), ({"node_feature": ["hse"], "hse": None}, "hse"),
                      ({"node_feature": ["bsa"]}, "atom name"), ({"node_feature": ["hse"]}, "atom_name"),
                      ({"edge_feature": ("dist", "other")}, "edge_feature"), ({"edge_transform": "tanh"}, "edge_transform"),
                      ({"clustering_method": "kmeans"}, "clustering method"), ({"target": "irmsd"}, "go together"),
                      ({"residue_features": {"type": np.zeros(R)}}, "built-in")):
        with pytest.raises(ValueError, match=match):
            run(**kw)
    with pytest.raises(ValueError, match="names"):
        interface_resident_set(t2, n2[:1], node_feature=["type"], api=api, device=device)
