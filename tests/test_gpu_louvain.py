"""Deterministic Louvain (drgnn_louvain) on the MI355X against tests/louvain_ref.py: labels, (levels, passes) and
the bits of the modularity; repeat launches; the PreCluster path and training with cluster_nodes='louvain'."""
import numpy as np
import pytest
import torch

import louvain_ref as R
import test_louvain as T
from helpers import GOLDEN
from test_louvain import all_cases, check_precluster, _fixture_batch_without_clusters, _names

pytestmark = pytest.mark.gpu


def _device_run(cases):
    from deeprank_gnn_amd.clustering import louvain_labels
    ei, nptr, eptr = (t.cuda() for t in R.batch_of(cases))
    labels, info, q = louvain_labels(ei, nptr, eptr)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), info.cpu().numpy(), q.cpu().numpy()


def _check(cases, got):
    labels, info, q = got
    off = 0
    for g, (name, pairs, n) in enumerate(cases):
        lab, inf, mod = R.louvain(pairs, n)
        np.testing.assert_array_equal(labels[off:off + n], lab, err_msg=name)
        assert tuple(info[g]) == inf, name
        assert q[g:g + 1].view(np.int64)[0] == np.array([mod]).view(np.int64)[0], (name, q[g], mod)
        off += n


@pytest.mark.parametrize("case", all_cases(), ids=_names(all_cases()))
def test_device_equals_reference_per_graph(case):
    _check([case], _device_run([case]))


def test_device_equals_reference_in_one_batch():
    cases = all_cases() + R.synthetic_pairs(64)
    _check(cases, _device_run(cases))


def test_1024_synthetic_graphs_in_one_launch_and_repeat_launches_bit_identical():
    cases = R.synthetic_pairs(1024)
    first = _device_run(cases)
    _check(cases, first)
    second = _device_run(cases)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


def test_graph_near_the_carve_limit():
    """1 024 nodes with 4 096 pairs listed in both directions, as PreCluster passes them: a carve of ~153 KiB
    (dynamic LDS beyond 64 KiB)"""
    cases = [("limit",) + R.limit_graph()] + R.special_cases()
    _check(cases, _device_run(cases))


def test_precluster_louvain_on_device_equals_reference():
    from deeprank_gnn_amd.clustering import precluster
    batch, refs = _fixture_batch_without_clusters()
    d0, d1 = precluster(batch.to("cuda"), method='louvain')
    check_precluster(d0.cpu().numpy(), d1.cpu().numpy(), refs)


def test_neuralnet_louvain_trains_on_device(tmp_path):
    import os
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
                   percent=[0.8, 0.2], outdir=str(tmp_path), cluster_nodes='louvain')
    mol = bare.mols()[0]
    p = bare.get(mol, "internal_edge_index")
    d0, _ = R.louvain_precluster_ref(np.vstack((p, p[:, ::-1])), bare.get(mol, "node_data/pos").shape[0])
    np.testing.assert_array_equal(nn.dataset.store.get(mol, "clustering/louvain/depth_0"), d0)
    nn.train(nepoch=2, validate=True, save_model=None, hdf5=None)
    assert len(nn.train_loss) == 2 and all(np.isfinite(nn.train_loss))


# ---- beyond the fixture: the checks of tests/test_louvain.py (cases of tests/louvain_cases.py) on the device ---------
def _device_kw():
    from deeprank_gnn_amd import _lib
    return dict(api=_lib.get(), device="cuda")


def test_device_raw_edge_lists_one_by_one():
    T.check_raw_cases_one_by_one(_device_kw())


def test_device_raw_ends_outside_the_graph_in_a_batch():
    T.check_ends_outside_in_a_batch(_device_kw())


@pytest.mark.parametrize("with_large", [False, True], ids=["alone", "next_to_600_nodes"])
def test_device_raw_edge_lists_in_one_batch(with_large):
    T.check_raw_batch(_device_kw(), with_large)


@pytest.mark.parametrize("which", ["capN", "capE"])
def test_device_graph_beyond_the_caps_is_refused_alone(which):
    T.check_refusal(_device_kw(), which)


def test_device_gain_threshold_decides():
    T.check_threshold(_device_kw())


def test_device_lane_edges_per_graph():
    T.check_lane_cases(_device_kw())


def test_device_lane_edges_in_one_batch_with_the_threshold_graph_twice():
    T.check_lane_batch(_device_kw(), repeat=True)


def test_device_invariants_of_the_existing_cases():
    T.check_existing_cases_invariants(_device_kw())


def test_device_modularity_against_all_set_partitions():
    T.check_against_enumeration(_device_kw())


def test_device_precluster_louvain_on_lane_cases():
    T.check_precluster_on_lane_cases(_device_kw())
