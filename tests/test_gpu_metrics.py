"""Metrics (drgnn_metrics) on the MI355X: the golden cases of the reference's own Metrics, 10^6 and 4*10^6 fp32
predictions with ties and NaN against tests/metrics_ref.py, repeat launches bit for bit, device tensors read in place,
and the published scripts' flow NeuralNet(pretrained_model=...) -> test() -> get_metrics('test', threshold=...).
The low-digit passes of the sort (the large cases' fp32 predictions rounded to 1/64 leave the low five digits of every
key zero) and the wave, workgroup and tile boundaries are covered by the cases of tests/metrics_cases.py, against the
reference and bit for bit against the host emulation; `_large` covers scale and the saturation of G."""
import os

import numpy as np
import pytest
import torch

import metrics_cases as MC
import metrics_ref as R
from helpers import GOLDEN
from test_metrics import CASES, NAMES, attrs_of, check_attrs, run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_reference_golden(name, capsys):
    run_case(CASES[name], None, capsys)
    run_case(CASES[name], None, capsys, device="cuda")


def _large(n, seed, nan):
    rng = np.random.default_rng(seed)
    y = rng.uniform(0.0, 10.0, n)
    pred = (y + rng.normal(0.0, 2.0, n)).astype(np.float32)
    pred[rng.integers(0, n, n // 10)] = np.float32(3.5)        # a long run of ties across many tiles
    pred = np.round(pred * 64) / 64                            # and many short ones
    if nan:
        pred[rng.integers(0, n, n // 1000)] = np.nan
    return pred.astype(np.float32), y


@pytest.mark.parametrize("n", [10 ** 6, 4 * 10 ** 6])
@pytest.mark.parametrize("target,nan", [("irmsd", False), ("fnat", False), ("dockQ", True)])
def test_large_fp32_with_ties_and_nan(n, target, nan):
    from deeprank_gnn_amd.metrics import Metrics
    pred, y = _large(n, n + len(target), nan)
    thr = 4.0
    if target in ("fnat", "dockQ"):
        y, pred, thr = y / 10.0, pred / np.float32(10.0), 0.3
    m = Metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(y).cuda(), target, thr)
    p64 = pred.astype(np.float64)
    check_attrs(attrs_of(m), R.metrics(p64, y, target, thr))
    idx, gt, hits, auc = R.ranking(p64, y, target, thr)
    np.testing.assert_array_equal(m.format_score()[0], idx)
    np.testing.assert_array_equal(m.hitrate(), hits)
    assert R.same(m.auc(), auc)


def test_repeat_launches_bit_identical():
    from deeprank_gnn_amd.metrics import Metrics
    pred, y = _large(4 * 10 ** 6, 7, False)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(y).cuda()
    a, b = Metrics(p, t, "irmsd", 4.0), Metrics(p, t, "irmsd", 4.0)
    check_attrs(attrs_of(a), attrs_of(b), exact_floats=True)
    assert torch.equal(a.hitrate_tensor(), b.hitrate_tensor())
    assert a.auc() == b.auc()


def test_device_tensors_are_read_in_place():
    from deeprank_gnn_amd.metrics import Metrics
    pred, y = _large(10 ** 5, 9, False)
    p = torch.from_numpy(pred.astype(np.float64)).cuda()
    t = torch.from_numpy(y).cuda()
    m = Metrics(p, t, "lrmsd", 4.0)
    assert m._pred.data_ptr() == p.data_ptr() and m._y.data_ptr() == t.data_ptr()
    assert m.hitrate_tensor().is_cuda and m.hitrate_tensor().device == p.device
    m32 = Metrics(torch.from_numpy(pred).cuda(), t, "lrmsd", 4.0)      # fp32: converted on the device
    assert m32._pred.is_cuda
    check_attrs(attrs_of(m32), attrs_of(m), exact_floats=True)


# ---- tile, wave and digit boundaries with keys of eight varying bytes (tests/metrics_cases.py) ---------------------
@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


@pytest.mark.parametrize("target", MC.RANK_TARGETS)
@pytest.mark.parametrize("n", MC.SIZES)
def test_ranking_of_wide_keys_at_boundaries(n, target, api):
    from emu_api import emu
    MC.assert_same_results(MC.check_ranking(n, target, api, "cuda"), MC.check_ranking(n, target, emu(), None))


@pytest.mark.parametrize("target", MC.REG_TARGETS)
@pytest.mark.parametrize("n", MC.SIZES)
def test_regression_scores_and_median_at_boundaries(n, target, api):
    from emu_api import emu
    MC.assert_same_results(MC.check_regression(n, target, api, "cuda"), MC.check_regression(n, target, emu(), None))


@pytest.mark.parametrize("n", MC.CLASS_SIZES)
def test_class_matrix_ignores_outside_labels_across_tiles(n, api):
    from emu_api import emu
    MC.assert_same_results(MC.check_classes(n, api, "cuda"), MC.check_classes(n, emu(), None))


def test_boundary_ranking_twice_bit_identical(api):
    MC.check_repeat(api, "cuda")


# ---- the published scripts' flow -----------------------------------------------------------------------------------
def _checkpoint(path, g, target, task, node_feature, threshold):
    """a checkpoint in save_model's dictionary schema (reference NeuralNet.py:775-790) with the golden parameters"""
    from helpers import params_of
    state = {'model': params_of(g),
             'optimizer': {'state': {}, 'param_groups': [{'lr': 0.001, 'betas': (0.9, 0.999), 'eps': 1e-08,
                                                          'weight_decay': 0}]},
             'node': node_feature, 'edge': ['dist'], 'target': target, 'task': task, 'classes': [0, 1],
             'class_weight': None, 'batch_size': 64, 'percent': [1.0, 0.0], 'lr': 0.001, 'index': None,
             'shuffle': False, 'threshold': threshold, 'cluster_nodes': 'mcl', 'transform_sigmoid': False}
    torch.save(state, path)
    return path


def test_published_flow_pretrained_classifier(tmp_path, capsys):
    """prediction_phy_non-phy.py: test() then get_metrics('test', threshold=1.0) and the six scores it prints"""
    from helpers import golden
    from deeprank_gnn_amd.NeuralNet import NeuralNet
    from deeprank_gnn_amd.ginet import GINet
    g = golden("pretrained_class.npz")
    ck = _checkpoint(os.path.join(str(tmp_path), "tclass.pth.tar"), g, 'binclass', 'class',
                     [str(s) for s in g["node_feature"]], 1)
    model = NeuralNet(os.path.join(GOLDEN, "fixture_1ATN.npz"), GINet, pretrained_model=ck, outdir=str(tmp_path))
    model.test(hdf5=None)
    m = model.get_metrics('test', threshold=1.0)
    assert "Threshold set to 1" in capsys.readouterr().out
    ref = R.metrics(model.test_out, model.test_y, 'binclass', model.classes_to_idx[1.0])
    for a in ("accuracy", "specificity", "sensitivity", "precision", "FPR", "FNR"):
        assert R.same(getattr(m, a), ref[a]), a
    assert m.accuracy == model.test_acc
    assert len(model.test_out) == 10


def test_published_flow_pretrained_regression(tmp_path, capsys):
    """scoring_of_docking_models/test.py: get_metrics('test', threshold=t) over ten thresholds, r2_score included"""
    from helpers import golden
    from deeprank_gnn_amd.dataset import GraphStore
    from deeprank_gnn_amd.NeuralNet import NeuralNet
    from deeprank_gnn_amd.ginet import GINet
    g = golden("pretrained_treg.npz")
    st = GraphStore(os.path.join(GOLDEN, "fixture_1ATN.npz"))
    rng = np.random.default_rng(0)
    for mol in st.mols():        # the shipped model reads one-hot residue types (20) and polarities (4): 48 features
        n = st.get(mol, "node_data/pos").shape[0]
        st.set(mol, "node_data/type", np.eye(20, dtype=np.float32)[rng.integers(0, 20, n)])
        st.set(mol, "node_data/polarity", np.eye(4, dtype=np.float32)[rng.integers(0, 4, n)])
    db = os.path.join(str(tmp_path), "treg.npz")
    st.save_npz(db)
    ck = _checkpoint(os.path.join(str(tmp_path), "treg.pth.tar"), g, str(g["target_name"]), 'reg',
                     [str(s) for s in g["node_feature"]], 0.3)
    model = NeuralNet(db, GINet, pretrained_model=ck, outdir=str(tmp_path))
    model.test(hdf5=None)
    out, y = model.test_out, model.test_y
    assert len(out) == 10 and np.isfinite(out).all()
    for thr in np.linspace(0.0, 0.9, 10):
        m = model.get_metrics('test', threshold=float(thr))
        check_attrs(attrs_of(m), R.metrics(out, y, 'fnat', float(thr)))
        assert m.r2_score is not None
        np.testing.assert_array_equal(m.hitrate(), R.ranking(out, y, 'fnat', float(thr))[2])
