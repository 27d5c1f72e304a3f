"""Deterministic Louvain (drgnn_louvain, host-emulation build) against the plain-Python statement of the
algorithm in tests/louvain_ref.py: labels, (levels, passes) and the bits of the modularity, one graph at a time
and all graphs in one batch; the reference itself against networkx; the package paths that take
method='louvain' (precluster, PreCluster, community_detection, NeuralNet).  CPU only."""
import numpy as np
import pytest
import torch

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
