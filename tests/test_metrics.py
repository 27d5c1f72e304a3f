"""Metrics / NeuralNet.get_metrics (deeprank_gnn_amd.metrics, drgnn_metrics on the host-emulation build).

The numpy statement (tests/metrics_ref.py) against the reference's own Metrics (tests/golden/metrics.npz), the emulated
kernels against both: counts, ranking, hit rate, max_error and the median exactly, the other regression scores to rtol
1e-9 (sklearn's float64 sums run in another order).  Ties, NaN, the ValueError cases and get_metrics after
train / eval / test; the cases of tests/metrics_cases.py (keys of eight varying bytes at the wave, workgroup and tile
boundaries).  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

import metrics_cases as MC
import metrics_ref as R
from helpers import GOLDEN, NODE_FEATURES

RTOL = 1e-9


def golden_cases():
    with np.load(os.path.join(GOLDEN, "metrics.npz")) as z:
        d = {k: z[k] for k in z.files}
    out = {}
    for k in d:
        if k.endswith("/meta"):
            name = k[:-5]
            meta = json.loads(str(d[k]))
            attrs = {a: (None if a in meta["none"] else d["%s/attr/%s" % (name, a)])
                     for a in R.CLASS_ATTRS + R.REG_ATTRS + ("mean_abolute_error",)}
            out[name] = dict(meta, pred=d[name + "/pred"], y=d[name + "/y"], attrs=attrs,
                             hitrate=d.get(name + "/hitrate"), auc=d.get(name + "/auc"))
    return out


CASES = golden_cases()
NAMES = sorted(CASES)


def check_attrs(got, want, exact_floats=False):
    """got / want: attribute -> value.  Classification scores and max_error / median exactly, the rest to RTOL."""
    for a in R.CLASS_ATTRS + R.EXACT:
        assert R.same(got[a], want[a]), (a, got[a], want[a])
    for a in R.REG_ATTRS + ("mean_abolute_error",):
        if a not in R.EXACT:
            assert R.same(got[a], want[a], rtol=0.0 if exact_floats else RTOL), (a, got[a], want[a])


def attrs_of(m):
    return {a: getattr(m, a) for a in R.CLASS_ATTRS + R.REG_ATTRS + ("mean_abolute_error",)}


def run_case(case, api, capsys, device=None):
    """Metrics on the case's inputs; checks the printed lines, the scores and (where recorded) hit rate / AUC against the
    golden file and against metrics_ref.  Returns the Metrics."""
    from deeprank_gnn_amd.metrics import Metrics
    pred, y = case["pred"], case["y"]
    if device is not None:
        pred, y = torch.from_numpy(pred).to(device), torch.from_numpy(y).to(device)
    capsys.readouterr()
    m = Metrics(pred, y, case["target"], case["threshold"], case["binary"], api=api)
    assert capsys.readouterr().out.splitlines() == case["printed"]
    got = attrs_of(m)
    check_attrs(got, case["attrs"])
    ref = R.metrics(case["pred"], case["y"], case["target"], case["threshold"], case["binary"])
    check_attrs(got, ref)
    idx, gt, hits, auc = R.ranking(case["pred"], case["y"], case["target"], case["threshold"])
    np.testing.assert_array_equal(m.hitrate(), hits)
    assert m.hitrate().dtype == np.int64 and m.hitrate().shape == (case["pred"].size,)
    fidx, fgt = m.format_score()
    np.testing.assert_array_equal(fidx, idx)
    np.testing.assert_array_equal(fgt, gt)
    assert R.same(m.auc(), auc)
    if case["ranked"]:
        np.testing.assert_array_equal(m.hitrate(), case["hitrate"])
        assert R.same(m.auc(), case["auc"], rtol=RTOL)
    return m


@pytest.mark.parametrize("name", NAMES)
def test_numpy_statement_equals_reference_golden(name):
    c = CASES[name]
    ref = R.metrics(c["pred"], c["y"], c["target"], c["threshold"], c["binary"])
    check_attrs(ref, c["attrs"])
    assert ref["printed"] == c["printed"]
    if c["ranked"]:
        _, _, hits, auc = R.ranking(c["pred"], c["y"], c["target"], c["threshold"])
        np.testing.assert_array_equal(hits, c["hitrate"])
        assert R.same(auc, c["auc"], rtol=RTOL)


@pytest.mark.parametrize("name", NAMES)
def test_emulated_kernels_equal_reference(name, capsys):
    from emu_api import emu
    run_case(CASES[name], emu(), capsys)


def test_golden_covers_the_edge_cases():
    c = CASES
    assert c["irmsd_le_minus1"]["attrs"]["mean_squared_log_error"] is None
    assert c["dockQ"]["attrs"]["r2_score"] is None and c["dockQ"]["attrs"]["accuracy"] is not None
    assert np.isnan(c["single_class_constant_y"]["auc"]) and np.isnan(c["n1"]["attrs"]["r2_score"])
    assert np.isnan(c["all_negative"]["attrs"]["sensitivity"])
    assert c["capri_class_classes"]["attrs"]["precision"].shape == (5,)
    assert c["even_n"]["pred"].size % 2 == 0 and c["irmsd_distinct"]["pred"].size % 2 == 1


def tie_case(n, seed, target):
    rng = np.random.default_rng(seed)
    pred = np.round(rng.uniform(-3.0, 3.0, n), 1)          # ~60 distinct values: long runs of ties
    pred[rng.integers(0, n, n // 50)] = -0.0
    pred[rng.integers(0, n, n // 50)] = 0.0
    y = rng.uniform(-0.5, 3.0, n)
    return pred, y


@pytest.mark.parametrize("target", ["irmsd", "fnat", "dockQ"])
def test_ties_ranked_in_stable_order_across_tiles(target, capsys):
    """n = 9 000: three radix tiles, several reduction workgroups; -0.0 ties +0.0"""
    from emu_api import emu
    pred, y = tie_case(9000, 3, target)
    case = dict(pred=pred, y=y, target=target, threshold=1.0, binary=True, ranked=False, printed=None)
    case["attrs"] = {k: v for k, v in R.metrics(pred, y, target, 1.0).items() if k != "printed"}
    case["printed"] = R.metrics(pred, y, target, 1.0)["printed"]
    run_case(case, emu(), capsys)


def test_nan_ranks_last_and_counts_as_negative(capsys):
    from emu_api import emu
    from deeprank_gnn_amd.metrics import Metrics
    pred, y = tie_case(5000, 4, "dockQ")
    pred[::7] = np.nan
    y[::11] = np.nan
    m = Metrics(pred, y, "dockQ", 1.0, api=emu())
    ref = R.metrics(pred, y, "dockQ", 1.0)
    check_attrs(attrs_of(m), ref)
    idx, gt, hits, auc = R.ranking(pred, y, "dockQ", 1.0)
    assert np.isnan(pred[idx[-1]])
    np.testing.assert_array_equal(m.format_score()[0], idx)
    np.testing.assert_array_equal(m.hitrate(), hits)
    assert R.same(m.auc(), auc)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nonfinite_regression_input_raises(bad):
    from emu_api import emu
    from deeprank_gnn_amd.metrics import Metrics
    pred = np.linspace(0.0, 5.0, 100)
    y = pred[::-1].copy()
    pred[40] = bad
    with pytest.raises(ValueError):
        Metrics(pred, y, "irmsd", 4, api=emu())
    with pytest.raises(ValueError):
        Metrics(y, pred, "fnat", 0.3, api=emu())


def test_value_errors(capsys):
    from emu_api import emu
    from deeprank_gnn_amd.metrics import Metrics
    with pytest.raises(ValueError, match="capri_class on bin_class"):
        Metrics([1.0, 2.0], [1.0, 3.0], "irmsd", 4, binary=False, api=emu())
    with pytest.raises(ValueError):
        Metrics([0.0, 0.5], [0.0, 1.0], "bin_class", 0, binary=False, api=emu())        # continuous labels
    with pytest.raises(ValueError):
        Metrics([0.0, np.nan], [0.0, 1.0], "bin_class", 0, binary=False, api=emu())
    with pytest.raises(ValueError):
        Metrics([1.0, 2.0], [7.0, 8.0], "capri_class", 3, binary=False, api=emu())       # no y among the labels
    with pytest.raises(ValueError):
        Metrics([1.0, 2.0, 3.0], [1.0, 2.0], "irmsd", 4, api=emu())
    with pytest.raises(ValueError):
        Metrics([], [], "irmsd", 4, api=emu())


def test_inputs_as_lists_arrays_and_tensors(capsys):
    from emu_api import emu
    from deeprank_gnn_amd.metrics import Metrics
    c = CASES["fnat_negative"]
    as_list = attrs_of(Metrics(c["pred"].tolist(), c["y"].tolist(), "fnat", 0.3, api=emu()))
    as_f32 = attrs_of(Metrics(torch.from_numpy(c["pred"].astype(np.float32)), torch.from_numpy(c["y"]), "fnat", 0.3,
                              api=emu()))
    check_attrs(as_list, c["attrs"])
    check_attrs(as_f32, as_list, exact_floats=True)        # the fp32 predictions convert exactly


def test_package_exports_metrics():
    import deeprank_gnn_amd
    from deeprank_gnn_amd.metrics import Metrics, get_binary, get_comparison
    assert deeprank_gnn_amd.Metrics is Metrics
    assert get_binary([0.1, 0.5], 0.3, "fnat") == [0, 1] and get_binary([0.1, 0.5], 0.3, "irmsd") == [1, 0]
    fp, fn, tp, tn = get_comparison([1, 0, 1, 1], [1, 1, 0, 1])
    assert (fp, fn, tp, tn) == (1, 1, 2, 0)


def test_emulated_and_host_restatement_bit_identical_twice(capsys):
    from emu_api import emu
    from deeprank_gnn_amd.metrics import Metrics
    c = CASES["irmsd_distinct"]
    a = attrs_of(Metrics(c["pred"], c["y"], "irmsd", 4, api=emu()))
    b = attrs_of(Metrics(c["pred"], c["y"], "irmsd", 4, api=emu()))
    check_attrs(a, b, exact_floats=True)


# ---- tile, wave and digit boundaries with keys of eight varying bytes (tests/metrics_cases.py) ---------------------
@pytest.mark.parametrize("target", MC.RANK_TARGETS)
@pytest.mark.parametrize("n", MC.SIZES)
def test_ranking_of_wide_keys_at_boundaries(n, target, capsys):
    from emu_api import emu
    MC.check_ranking(n, target, emu(), None)


@pytest.mark.parametrize("target", MC.REG_TARGETS)
@pytest.mark.parametrize("n", MC.SIZES)
def test_regression_scores_and_median_at_boundaries(n, target, capsys):
    from emu_api import emu
    MC.check_regression(n, target, emu(), None)


@pytest.mark.parametrize("n", MC.CLASS_SIZES)
def test_class_matrix_ignores_outside_labels_across_tiles(n, capsys):
    from emu_api import emu
    MC.check_classes(n, emu(), None)


def test_boundary_ranking_twice_bit_identical(capsys):
    from emu_api import emu
    MC.check_repeat(emu(), None)


# ---- NeuralNet.get_metrics -----------------------------------------------------------------------------------------
DRGS = os.path.join(GOLDEN, "1ATN_residue.drgs")


@pytest.mark.parametrize("task,target", [(None, 'irmsd'), ('class', 'binclass')])
def test_neuralnet_get_metrics_after_train_eval_test(task, target, tmp_path, capsys):
    from emu_api import emu
    from deeprank_gnn_amd.NeuralNet import NeuralNet
    from deeprank_gnn_amd.ginet import GINet
    torch.manual_seed(0)
    np.random.seed(0)
    nn = NeuralNet(DRGS, GINet, node_feature=NODE_FEATURES, edge_feature=['dist'], target=target, task=task,
                   batch_size=64, percent=[0.7, 0.3], outdir=str(tmp_path), _api=emu(), device='cpu')
    with pytest.raises(ValueError):
        nn.get_metrics('eval', threshold=nn.threshold)
    assert "No evaluation set has been provided" in capsys.readouterr().out
    nn.train(nepoch=2, validate=True, save_model=None, hdf5=None)
    thr = nn.threshold
    for data, acc in (('train', nn.train_acc[-1]), ('eval', nn.valid_acc[-1])):
        m = nn.get_metrics(data, threshold=thr)
        assert m.accuracy == acc, (data, m.accuracy, acc)
        out, y = (nn.train_out, nn.train_y) if data == 'train' else (nn.valid_out, nn.valid_y)
        t = nn.classes_to_idx[thr] if nn.task == 'class' else thr
        check_attrs(attrs_of(m), R.metrics(out, y, nn.target, t))
    nn.test(threshold=thr, hdf5=None)
    m = nn.get_metrics('test', threshold=thr)
    assert m.accuracy == nn.test_acc
    assert len(nn.test_out) == len(nn.test_y) == len(nn.dataset)
    with pytest.raises(ValueError):
        nn.get_metrics('train', threshold=thr)       # test() replaced the pass records, as in self.data


def test_get_metrics_without_targets_says_so(tmp_path, capsys):
    from emu_api import emu
    from deeprank_gnn_amd.NeuralNet import NeuralNet
    from deeprank_gnn_amd.ginet import GINet
    nn = NeuralNet(DRGS, GINet, node_feature=NODE_FEATURES, edge_feature=['dist'], target='irmsd', batch_size=64,
                   outdir=str(tmp_path), _api=emu(), device='cpu')
    nn.test(hdf5=None)
    nn.data['test'].arrays = (nn.data['test'].arrays[0], None)     # a test set without targets
    assert nn.test_y is None and len(nn.test_out) == len(nn.dataset)
    with pytest.raises(ValueError):
        nn.get_metrics('test')
    assert "You must provide ground truth target values" in capsys.readouterr().out
