"""Ensemble (K checkpoints of one net over one resident set), kernels emulated on CPU: validation of the members, the
reference's ten fold models against ensemble_treg.npz, NeuralNet(pretrained_model=[...]) and the inference-only rule."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, NODE_FEATURES, golden, treg_graphs
from emu_api import emu
import elementwise as ew
from deeprank_gnn_amd import Ensemble, _lib
from deeprank_gnn_amd.NeuralNet import NeuralNet
from deeprank_gnn_amd.ginet import GINet
from deeprank_gnn_amd.sGAT import sGAT
from deeprank_gnn_amd.foutnet import FoutNet
from deeprank_gnn_amd.resident import ResidentGraphSet
from deeprank_gnn_amd.trainer import FusedTrainer

DB = os.path.join(GOLDEN, "fixture_1ATN.npz")


def fold_states(g):
    """the ten fold models' state dicts of ensemble_treg.npz"""
    out = []
    for k in range(1, 11):
        pre = "fold%d/" % k
        out.append({n[len(pre):]: torch.from_numpy(g[n].copy()) for n in g if n.startswith(pre)})
    return out


def random_states(Net, F, K, O=1, seed=0):
    torch.manual_seed(seed)
    return [{k: v.clone() for k, v in Net(F, O, 1).state_dict().items()} for _ in range(K)]


def test_fold_models_match_reference():
    """the reference's ten fold checkpoints on helpers.treg_graphs(): per fold under the elementwise rule, mean and
    spread against the fixture's"""
    from deeprank_gnn_amd.data import Batch
    g = golden("ensemble_treg.npz")
    graphs = treg_graphs()
    states = fold_states(g)
    ens = Ensemble(GINet, states, device="cpu", api=emu())
    assert ens.K == 10 and ens.n_feat == 48 and ens.task == "reg"
    pred = ens.predict(ResidentGraphSet(graphs, "cpu", api=emu()), batch_size=6).numpy()
    assert pred.shape == (10, 6, 1)
    batch = Batch.from_data_list(graphs)
    stats = ew.new_stats()
    for k in range(10):
        ew.check("fold%d" % (k + 1), pred[k], g["pred"][k],
                 lambda k=k: ew.oracle64("GINet", states[k], batch, batch.y)[0].numpy(), stats)
    ew.assert_arbiter_rate(stats, "ensemble folds")
    np.testing.assert_allclose(pred.mean(axis=0), g["mean"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(pred.std(axis=0), g["std"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("Net", [GINet, sGAT, FoutNet])
def test_members_equal_single_predictions(Net):
    """the emulated library has no fused K-model launch: the members' own launches, bit for bit a single model's"""
    from helpers import fixture_graphs
    graphs = fixture_graphs(NODE_FEATURES)
    F = graphs[0].num_features
    states = random_states(Net, F, 3, seed=1)
    rs = ResidentGraphSet(graphs, "cpu", api=emu())
    ens = Ensemble(Net, states, device="cpu", api=emu())
    pred = ens.predict(rs, batch_size=4)
    assert ens.last_path == "separate" and ens.last_reason
    assert tuple(pred.shape) == (3, len(graphs), 1)
    for k, sd in enumerate(states):
        net = Net(F, 1, 1)
        net.load_state_dict(sd)
        tr = FusedTrainer(net, task="reg", api=emu())
        ref = tr.predict_epoch(rs, list(range(len(graphs))), 4, cached=ens._cached_ok(rs))
        assert torch.equal(pred[k], ref.reshape(len(graphs), 1)), k
    # a subset, in another order
    idx = [5, 1, 7]
    sub = ens.predict(rs, indices=idx, batch_size=2)
    assert torch.equal(sub, pred[:, idx])
    # the K parameter sets live in one [K, P] buffer
    assert tuple(ens.params.shape) == (3, ens.trainers[0].flat_p.numel())
    assert ens.nets[2].fc2.bias.data_ptr() == ens.params[2].data_ptr() + 4 * ens.trainers[2].offset["fc2.bias"]


def _ckpt(tmp_path, name, sd, **over):
    state = {'model': sd, 'optimizer': None, 'node': NODE_FEATURES, 'edge': ['dist'], 'target': 'irmsd', 'task': 'reg',
             'classes': [0, 1], 'class_weight': None, 'batch_size': 64, 'percent': [1.0, 0.0], 'lr': 0.01, 'index': None,
             'shuffle': True, 'threshold': 0.3, 'cluster_nodes': 'mcl', 'transform_sigmoid': False}
    state.update(over)
    path = os.path.join(str(tmp_path), name)
    torch.save(state, path)
    return path


def test_mismatched_members_raise(tmp_path):
    a, b = random_states(GINet, 28, 2)
    with pytest.raises(ValueError, match="'F'"):
        Ensemble(GINet, [a, random_states(GINet, 20, 1)[0]], device="cpu", api=emu())
    with pytest.raises(ValueError, match="'transform_sigmoid'"):
        Ensemble(GINet, [_ckpt(tmp_path, "a.pt", a), _ckpt(tmp_path, "b.pt", b, transform_sigmoid=True)],
                 device="cpu", api=emu())
    c = random_states(GINet, 28, 1, O=2)[0]
    with pytest.raises(ValueError, match="'task'"):
        Ensemble(GINet, [_ckpt(tmp_path, "a.pt", a), _ckpt(tmp_path, "c.pt", c, task='class')], device="cpu", api=emu())
    d = random_states(GINet, 28, 1, O=2)[0]
    with pytest.raises(ValueError, match="'classes'"):
        Ensemble(GINet, [_ckpt(tmp_path, "c.pt", c, task='class'), _ckpt(tmp_path, "d.pt", d, task='class', classes=[1, 2])],
                 device="cpu", api=emu())
    with pytest.raises(ValueError):
        Ensemble(GINet, [], device="cpu", api=emu())
    # a layer of another width (F and the head alike): the parameter is named, before any state dict is loaded
    e = dict(b)
    e["conv1.fc_attention.weight"] = torch.zeros(1, 40)
    with pytest.raises(ValueError, match="'conv1.fc_attention.weight'"):
        Ensemble(GINet, [a, e], device="cpu", api=emu())


def test_emulated_plan_is_none():
    """the host emulation has no ensemble launch: its plan answers NONE and predict takes the members' launches"""
    p = emu().ens_step_plan(3, _lib.GINET, 28, 60, 200, 30, 64, 128, 1, 16, _lib.TOPO_HIER | _lib.TOPO_TILES)
    assert p.family == _lib.STEP_FAMILY_NONE


def _nn(path, tmp_path):
    return NeuralNet(DB, GINet, pretrained_model=path, outdir=str(tmp_path), _api=emu(), device='cpu')


def test_neuralnet_ensemble_regression(tmp_path):
    states = random_states(GINet, 28, 3, seed=2)
    paths = [_ckpt(tmp_path, "m%d.pt" % k, sd, batch_size=4) for k, sd in enumerate(states)]
    singles = [_nn(p, tmp_path).test(hdf5=None) for p in paths]
    ens_nn = _nn(paths, tmp_path)
    assert ens_nn.ensemble is not None and ens_nn.ensemble.K == 3
    store = ens_nn.test(hdf5='ens.drgs')
    per = np.array([s['raw_outputs'] for s in singles]).T                  # [n, K]
    got = np.asarray(store['ensemble_raw_outputs'])
    assert got.shape == (10, 3)
    np.testing.assert_array_equal(got, per)
    np.testing.assert_allclose(store['outputs'], per.mean(axis=1), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(store['raw_outputs'], store['outputs'])
    assert store['mol'] == singles[0]['mol'] and store['targets'] == singles[0]['targets']
    assert np.isfinite(ens_nn.test_loss)
    m = ens_nn.get_metrics('test', threshold=4.0)
    assert m is not None
    # the export carries the members' outputs too
    from deeprank_gnn_amd.container import read_container
    _, exp = read_container(ens_nn.exported[-1])
    assert exp['tree/epoch_0000/test/ensemble_raw_outputs'].shape == (10, 3)
    # a single checkpoint: no ensemble, today's record
    assert _nn(paths[0], tmp_path).ensemble is None and 'ensemble_raw_outputs' not in dict(singles[0].items())
    # inference only
    with pytest.raises(_lib.DrgnnError, match="inference only"):
        ens_nn.train(nepoch=1)


def test_neuralnet_ensemble_classification(tmp_path):
    states = random_states(GINet, 28, 2, O=2, seed=3)
    paths = [_ckpt(tmp_path, "c%d.pt" % k, sd, task='class', target='binclass', batch_size=4, threshold=1)
             for k, sd in enumerate(states)]
    singles = [_nn(p, tmp_path).test(hdf5=None) for p in paths]
    store = _nn(paths, tmp_path).test(hdf5=None)
    prob = np.stack([np.asarray(s['raw_outputs']) for s in singles], axis=1)        # [n, K, O]
    got = np.asarray(store['ensemble_raw_outputs'])
    assert got.shape == (10, 2, 2)
    np.testing.assert_allclose(got, prob, rtol=1e-6, atol=1e-7)
    mean = prob.mean(axis=1)
    np.testing.assert_allclose(store['raw_outputs'], mean, rtol=1e-6, atol=1e-7)
    assert store['outputs'] == [[0, 1][i] for i in mean.argmax(axis=1)]
