"""Deterministic Louvain (drgnn_louvain, host-emulation build) against the plain-Python statement of the
algorithm in tests/louvain_ref.py: labels, (levels, passes) and the bits of the modularity, one graph at a time
and all graphs in one batch; the reference itself against networkx; the package paths that take
method='louvain' (precluster, PreCluster, community_detection, NeuralNet).  CPU only."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import louvain_cases as C
import louvain_ref as R
from helpers import GOLDEN


def _run(cases, api):
    from deeprank_gnn_amd.clustering import louvain_labels
    ei, nptr, eptr = R.batch_of(cases)
    labels, info, q = louvain_labels(ei, nptr, eptr, api=api)
    return labels.numpy(), info.numpy(), q.numpy()


def check_against_reference(cases, api):
    labels, info, q = _run(cases, api)
    off = 0
    for g, (name, pairs, n) in enumerate(cases):
        lab, inf, mod = R.louvain(pairs, n)
        np.testing.assert_array_equal(labels[off:off + n], lab, err_msg=name)
        assert tuple(info[g]) == inf, name
        assert q[g:g + 1].view(np.int64)[0] == np.array([mod]).view(np.int64)[0], (name, q[g], mod)
        off += n


def all_cases():
    return R.fixture_pairs() + R.special_cases()


def _names(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("k", range(10))
def test_reference_is_a_real_louvain(k):
    nx = pytest.importorskip("networkx")
    name, pairs, n = R.fixture_pairs()[k]
    labels, _, q = R.louvain(pairs, n)
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(pairs.tolist())
    parts = {}
    for v, c in enumerate(labels):
        parts.setdefault(c, set()).add(v)
    assert abs(q - nx.community.modularity(G, list(parts.values()))) <= 1e-12
    lowest = min(nx.community.modularity(G, nx.community.louvain_communities(G, seed=s)) for s in range(8))
    assert q >= lowest - 0.005


@pytest.mark.parametrize("case", all_cases(), ids=_names(all_cases()))
def test_emulated_kernel_equals_reference_per_graph(case):
    from emu_api import emu
    check_against_reference([case], emu())


def test_emulated_kernel_equals_reference_in_one_batch():
    """a graph's result does not depend on its batch neighbours (the batch's largest graph sizes every carve)"""
    from emu_api import emu
    check_against_reference(all_cases() + R.synthetic_pairs(64), emu())


def test_known_partitions():
    from emu_api import emu
    labels, info, _ = _run(R.special_cases(), emu())
    got, off = {}, 0
    for name, _, n in R.special_cases():
        got[name] = labels[off:off + n].tolist()
        off += n
    assert got["toy6"] == [0, 0, 0, 1, 1, 1]
    assert got["edgeless"] == [0, 1, 2, 3, 4] and got["single_node"] == [0]
    assert tuple(info[1]) == (0, 0)
    assert got["K8"] == [0] * 8
    assert got["clique_ring"] == [c for c in range(6) for _ in range(5)]
    assert got["star200"] == [0] * 201


def test_carve_limit_and_capacity_error():
    """1 024 nodes with 4 096 pairs listed in both directions (as PreCluster passes them) fit the 160 KiB carve and
    equal the reference; 4 700 pairs are refused, and so is a raw list whose entry count exceeds the carve."""
    from emu_api import emu
    from deeprank_gnn_amd._lib import DrgnnError
    from deeprank_gnn_amd.clustering import louvain_labels
    pairs, n = R.limit_graph()
    assert len(pairs) == 8192
    check_against_reference([("limit", pairs, n), ("toy6",) + R.special_cases()[0][1:]], emu())
    with pytest.raises(DrgnnError, match="capacity"):
        louvain_labels(*R.batch_of([("over",) + R.limit_graph(n_pairs=4700)]), api=emu())
    ei, nptr, eptr = R.batch_of([("big", [(i, (i + 1) % 2048) for i in range(8192)], 2048)])
    labels = torch.zeros(2048, dtype=torch.int64)
    info = torch.zeros((1, 2), dtype=torch.int32)
    q = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(DrgnnError, match="capacity"):
        emu().louvain(ei, ei.size(1), nptr, eptr, 1, 2048, 8192, labels, info, q, None)


def _fixture_batch_without_clusters():
    from helpers import fixture_graphs
    from deeprank_gnn_amd.data import Batch
    graphs = fixture_graphs(count=None)
    refs = [R.louvain_precluster_ref(g.internal_edge_index.t().numpy(), g.num_nodes) for g in graphs]
    for g in graphs:
        g.cluster0 = None
        g.cluster1 = None
    return Batch.from_data_list(graphs), refs


def check_precluster(d0, d1, refs):
    np.testing.assert_array_equal(d0, np.concatenate([r[0] for r in refs]))
    np.testing.assert_array_equal(d1, np.concatenate([r[1] for r in refs]))
    off = 0
    for r in refs:                                   # consecutive, in order of first appearance
        first = list(dict.fromkeys(d0[off:off + len(r[0])].tolist()))
        assert first == list(range(len(first)))
        off += len(r[0])


def test_precluster_louvain_equals_reference():
    from emu_api import emu
    from deeprank_gnn_amd.clustering import precluster
    batch, refs = _fixture_batch_without_clusters()
    d0, d1 = precluster(batch, method='louvain', api=emu())
    check_precluster(d0.numpy(), d1.numpy(), refs)


def test_PreCluster_louvain_adds_groups_and_keeps_mcl():
    from emu_api import emu
    from deeprank_gnn_amd.clustering import PreCluster
    from deeprank_gnn_amd.dataset import GraphDataSet, GraphStore
    from helpers import NODE_FEATURES
    ds = GraphDataSet(GOLDEN + "/fixture_1ATN.npz", node_feature=NODE_FEATURES, edge_feature=["dist"],
                      target="irmsd")
    full = GraphStore(GOLDEN + "/fixture_1ATN.npz")
    PreCluster(ds, method='louvain', api=emu(), device='cpu')
    for mol in full.mols():
        for depth in ("depth_0", "depth_1"):
            old = full.get(mol, "clustering/mcl/" + depth)
            kept = ds.store.get(mol, "clustering/mcl/" + depth)
            assert kept.dtype == old.dtype and kept.tobytes() == old.tobytes()
        n = full.get(mol, "node_data/pos").shape[0]
        p = full.get(mol, "internal_edge_index")
        d0, d1 = R.louvain_precluster_ref(np.vstack((p, p[:, ::-1])), n)
        np.testing.assert_array_equal(ds.store.get(mol, "clustering/louvain/depth_0"), d0)
        np.testing.assert_array_equal(ds.store.get(mol, "clustering/louvain/depth_1"), d1)
    with pytest.raises(ValueError):
        PreCluster(ds, method='xxx', api=emu(), device='cpu')


def test_neuralnet_louvain_without_stored_clusters(tmp_path):
    import os
    from emu_api import emu
    from deeprank_gnn_amd.dataset import GraphStore
    from deeprank_gnn_amd.NeuralNet import NeuralNet
    from deeprank_gnn_amd.ginet import GINet
    from helpers import NODE_FEATURES
    bare = GraphStore(GOLDEN + "/fixture_1ATN.npz")
    for mol in bare.mols():
        for k in [k for k in bare._mols[mol] if k.startswith("clustering/")]:
            del bare._mols[mol][k]
    path = os.path.join(str(tmp_path), "bare.npz")
    bare.save_npz(path)
    nn = NeuralNet(path, GINet, node_feature=NODE_FEATURES, edge_feature=['dist'], target='irmsd', batch_size=64,
                   percent=[0.8, 0.2], outdir=str(tmp_path), cluster_nodes='louvain', _api=emu(), device='cpu')
    for mol in bare.mols():
        n = bare.get(mol, "node_data/pos").shape[0]
        p = bare.get(mol, "internal_edge_index")
        d0, d1 = R.louvain_precluster_ref(np.vstack((p, p[:, ::-1])), n)
        np.testing.assert_array_equal(nn.dataset.store.get(mol, "clustering/louvain/depth_0"), d0)
        np.testing.assert_array_equal(nn.dataset.store.get(mol, "clustering/louvain/depth_1"), d1)
    nn.train(nepoch=1, validate=False, save_model=None, hdf5=None)
    assert np.isfinite(nn.train_loss[0])


def test_community_detection_louvain_on_the_reference_toy_graph(monkeypatch):
    from emu_api import emu
    from deeprank_gnn_amd import community_pooling as cp
    monkeypatch.setattr(cp, "_API", emu())
    ei = torch.tensor([[0, 1, 1, 2, 3, 4, 4, 5], [1, 0, 2, 1, 4, 3, 5, 4]])
    assert cp.community_detection(ei, 6, method='louvain').tolist() == [0, 0, 0, 1, 1, 1]
    per_batch = cp.community_detection_per_batch(torch.cat([ei, ei + 6], 1), torch.tensor([0] * 6 + [1] * 6), 12,
                                                 method='louvain')
    assert per_batch.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2]      # the reference's shared-id offset
    with pytest.raises(NotImplementedError):
        cp.community_detection(ei, 6, edge_attr=torch.ones(8), method='louvain')
    with pytest.raises(NotImplementedError):
        cp.community_detection_per_batch(ei, torch.zeros(6, dtype=torch.int64), 6, edge_attr=torch.ones(8),
                                         method='louvain')
    with pytest.raises(ValueError):
        cp.community_detection(ei, 6, method='xxx')


# ---- beyond the fixture (tests/louvain_cases.py): raw edge lists, the gain threshold, the 64-lane edges --------------
# Every check below is written over (run, device): run(cases, ...) is louvain_cases.raw or louvain_cases.labelled bound
# to a library, so that tests/test_gpu_louvain.py runs the same checks on the device.
def _emu_kw():
    from emu_api import emu
    return dict(api=emu(), device="cpu")


def check_raw_cases_one_by_one(kw):
    for case in C.raw_cases():
        got = C.raw([case], **kw)
        C.check_batch([case], got)
        for a, b in zip(got, C.labelled([case], **kw)):              # the raw call and louvain_labels: bit for bit
            assert a.tobytes() == b.tobytes(), case[0]
    labels, info, q = C.raw([C.raw_cases()[-1]], **kw)                # nothing inside the graph
    assert labels.tolist() == [0, 1, 2, 3, 4] and info.tolist() == [[0, 0]] and q.tolist() == [0.0]


def check_ends_outside_in_a_batch(kw):
    """the middle slice of three points into both neighbours' node ranges and below node_ptr[g]"""
    cases = [C.raw_cases()[4], C.raw_cases()[7], C.raw_cases()[6]]
    ei, nptr, _ = R.batch_of(cases)
    lo, hi = int(nptr[1]), int(nptr[2])
    mid = ei[:, 8:8 + len(cases[1][1])]
    assert int(((mid >= 0) & (mid < lo)).sum()) > 0 and int((mid >= hi).sum()) > 0 and int((mid < 0).sum()) > 0
    got = C.raw(cases, **kw)
    C.check_batch(cases, got)
    for a, b in zip(got, C.labelled(cases, **kw)):
        assert a.tobytes() == b.tobytes()


def check_raw_batch(kw, with_large):
    """all raw cases in one launch; next to a 600-node graph every carve is laid out for 600 nodes"""
    cases = C.raw_cases()
    if with_large:
        cases = cases[:5] + [("modular600",) + C.modular_graph(600, seed=600)] + cases[5:]
    got = C.raw(cases, **kw)
    C.check_batch(cases, got)
    for a, b in zip(got, C.labelled(cases, **kw)):
        assert a.tobytes() == b.tobytes()


def check_refusal(kw, which):
    """capN (capE) below the middle graph: (-1, -1), modularity 0, its labels untouched; the neighbours as ever"""
    cases = C.refusal_batch()
    n_mid, e_mid = cases[1][2], len(cases[1][1])
    assert all(c[2] < n_mid and len(c[1]) < e_mid for c in (cases[0], cases[2]))
    caps = dict(cap_n=n_mid - 1) if which == "capN" else dict(cap_e=e_mid - 1)
    labels, info, q = C.raw(cases, **caps, **kw)
    n0 = cases[0][2]
    assert info[1].tolist() == [-1, -1] and q[1] == 0.0
    assert (labels[n0:n0 + n_mid] == C.FILL).all()
    C.check_batch(cases, (labels, info, q), skip=(1,))


def check_threshold(kw):
    from deeprank_gnn_amd._lib import DrgnnError
    cases = C.threshold_cases()
    for case in cases:
        name, pairs, n = case
        for run in (C.labelled, C.raw):                              # listed once: the raw carve is the same
            labels, info, q = run([case], **kw)
            C.check_case(case, labels, info[0], q[0])
            C.check_threshold_expectations(case, labels, info[0])
        twice = (name, C.both_directions(pairs), n)
        labels, info, q = C.labelled([twice], **kw)                   # as internal_edge_index lists a graph
        C.check_threshold_expectations(case, labels, info[0])
        if C.lds_bytes(n, 2 * len(pairs)) > C.LDS_LIMIT:
            with pytest.raises(DrgnnError, match="capacity"):
                C.raw([twice], **kw)
    assert sum(C.lds_bytes(n, 2 * len(p)) > C.LDS_LIMIT for _, p, n in cases) == 3


def check_lane_cases(kw):
    cases = C.lane_cases()
    for case in cases:
        C.check_batch([case], C.labelled([case], **kw))
    both = [(name, C.both_directions(pairs), n) for name, pairs, n in cases if n <= 250]
    C.check_batch(both, C.raw(both, **kw))


def check_lane_batch(kw, repeat):
    """all of the lane cases next to the threshold graph: the largest carve among the new cases"""
    cases = C.lane_cases() + C.threshold_cases()[:1]
    got = C.labelled(cases, **kw)
    C.check_batch(cases, got)
    C.check_threshold_expectations(cases[-1], got[0][-cases[-1][2]:], got[1][-1])
    if repeat:
        for a, b in zip(got, C.labelled(cases, **kw)):
            assert a.tobytes() == b.tobytes()


def check_existing_cases_invariants(kw):
    cases = all_cases() + [("limit",) + R.limit_graph()] + R.synthetic_pairs(16)
    labels, info, q = C.labelled(cases, **kw)
    off = 0
    for g, case in enumerate(cases):
        C.check_invariants(case, labels[off:off + case[2]], q[g])
        off += case[2]


def check_against_enumeration(kw):
    cases = C.tiny_cases()
    assert len(cases) >= 12 and all(c[2] <= 9 for c in cases)
    labels, info, q = C.raw(cases, **kw)
    C.check_batch(cases, (labels, info, q))
    off = 0
    for g, (name, pairs, n) in enumerate(cases):
        best, two_m = C.tiny_maxima()[name]
        got = C.exact_modularity(pairs, n, labels[off:off + n].tolist())
        assert got <= Fraction(best, two_m * two_m), name
        if name in C.REACHES_THE_MAXIMUM:
            assert got == Fraction(best, two_m * two_m), name
            assert C.bits(q[g]) == C.bits(float(Fraction(best, two_m * two_m))), name
        off += n


def check_precluster_on_lane_cases(kw):
    import types
    from deeprank_gnn_amd.clustering import precluster
    cases = [c for c in C.lane_cases() if c[0] in ("modular65", "hub64", "modular129")]
    assert len(cases) == 3
    cases = [(name, C.both_directions(pairs), n) for name, pairs, n in cases]
    ei, nptr, _ = R.batch_of(cases)
    bvec = torch.repeat_interleave(torch.arange(3), (nptr[1:] - nptr[:-1]).to(torch.int64))
    batch = types.SimpleNamespace(internal_edge_index=ei.to(kw["device"]), batch=bvec.to(kw["device"]), num_graphs=3)
    d0, d1 = precluster(batch, method='louvain', api=kw["api"])
    check_precluster(d0.cpu().numpy(), d1.cpu().numpy(), [R.louvain_precluster_ref(p, n) for _, p, n in cases])


def test_cases_sit_on_their_edges():
    """from the reference alone: ties, row lengths, community counts and level counts are what the names say"""
    C.check_lane_cases_sit_on_their_edges()
    for case in C.threshold_cases():
        lab, info, _ = C.reference(case)
        C.check_threshold_expectations(case, np.asarray(lab), info)
    for name, pairs, n in C.tiny_cases():
        best, two_m = C.tiny_maxima()[name]
        reached = C.exact_modularity(pairs, n, C.reference((name, pairs, n))[0]) == Fraction(best, two_m * two_m)
        assert reached or name not in C.REACHES_THE_MAXIMUM, name
    assert len(C.REACHES_THE_MAXIMUM) >= 5


def test_threshold_two_sites_trace():
    """thr_two_sites: level 1 gains much in its first pass and ends on a second pass that moves one node for a gain of
    2, below the threshold 2.19, and is recorded"""
    name, pairs, n = C.threshold_cases()[3]
    trace = []
    R.louvain(pairs, n, trace=trace)
    assert trace[1]["passes"] == [(2, 7872), (1, 2)] and trace[1]["recorded"] and not trace[2]["recorded"]
    assert 2 < 1e-7 * 4682 * 4682 < 7872
    name, pairs, n = C.threshold_cases()[2]
    trace = []
    R.louvain(pairs, n, trace=trace)
    assert trace[1]["passes"] == [(3, 6), (0, 0)] and 2 < 1e-7 * 7582 * 7582 < 6


def test_raw_edge_lists_one_by_one():
    check_raw_cases_one_by_one(_emu_kw())


def test_raw_ends_outside_the_graph_in_a_batch():
    check_ends_outside_in_a_batch(_emu_kw())


@pytest.mark.parametrize("with_large", [False, True], ids=["alone", "next_to_600_nodes"])
def test_raw_edge_lists_in_one_batch(with_large):
    check_raw_batch(_emu_kw(), with_large)


@pytest.mark.parametrize("which", ["capN", "capE"])
def test_graph_beyond_the_caps_is_refused_alone(which):
    check_refusal(_emu_kw(), which)


def test_gain_threshold_decides():
    check_threshold(_emu_kw())


def test_lane_edges_per_graph():
    check_lane_cases(_emu_kw())


def test_lane_edges_in_one_batch_with_the_threshold_graph():
    check_lane_batch(_emu_kw(), repeat=False)


def test_invariants_of_the_existing_cases():
    check_existing_cases_invariants(_emu_kw())


def test_modularity_against_all_set_partitions():
    check_against_enumeration(_emu_kw())


def test_precluster_louvain_on_lane_cases():
    check_precluster_on_lane_cases(_emu_kw())
