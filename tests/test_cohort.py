"""Cohort (K members of one net trained over one resident set), kernels emulated on CPU.  The emulated library has no cohort
launch: its plan answers NONE and every member runs its own step (the separate path, which is what a user gets for graphs the
fused kernels do not take) -- with the trajectory of a FusedTrainer of its own, bit for bit."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, NODE_FEATURES, fixture_graphs
from emu_api import emu
from deeprank_gnn_amd import Cohort, Ensemble, _lib, kfold_indices
from deeprank_gnn_amd.NeuralNet import NeuralNet
from deeprank_gnn_amd.ginet import GINet
from deeprank_gnn_amd.sGAT import sGAT
from deeprank_gnn_amd.foutnet import FoutNet
from deeprank_gnn_amd.resident import ResidentGraphSet
from deeprank_gnn_amd.trainer import FusedTrainer

DB = os.path.join(GOLDEN, "fixture_1ATN.npz")
NETS = {"GINet": GINet, "sGAT": sGAT, "FoutNet": FoutNet}


def random_states(Net, F, K, O=1, seed=0):
    torch.manual_seed(seed)
    return [{k: v.clone() for k, v in Net(F, O, 1).state_dict().items()} for _ in range(K)]


def schedule(n, K, T, B):
    """[T][K] mini-batches over n graphs, different per member: a short last mini-batch, and the last member has none in the
    last step"""
    rng = np.random.RandomState(3)
    rows = []
    for s in range(T):
        row = []
        for m in range(K):
            size = B if s < T - 1 else max(1, B - 1 - m % 2)
            if s == T - 1 and m == K - 1 and K > 1:
                size = 0
            row.append(rng.permutation(n)[:size].tolist())
        rows.append(row)
    return rows


def single_trajectory(Net, sd, rs, batches, lr, seed, api, task="reg", class_weights=None, O=1, dropout=None,
                      betas=(0.9, 0.999), eps=1e-8):
    """a FusedTrainer of its own over one member's mini-batches: (trainer, losses per step with None where it had none)"""
    net = Net(rs.n_feat, O, 1)
    net.load_state_dict(sd)
    if dropout is not None:
        net.dropout = dropout
    tr = FusedTrainer(net.to(rs.device), lr=lr, task=task, class_weights=class_weights, seed=seed, api=api, betas=betas,
                      eps=eps)
    tr.plan_overrides = {"force_wgs": 1}
    cache = rs.topology_cache(need_weights=Net is sGAT)
    losses = []
    for ids in batches:
        losses.append(tr.train_step_cached(cache, ids).clone() if len(ids) else None)
    return tr, losses


def assert_member_equals(coh, m, tr, losses, got_losses, words=False):
    """``words``: got_losses are the loss words after each step (unchanged where the member had no mini-batch), else the
    record of an epoch (NaN there)"""
    assert torch.equal(coh.params[m], tr.flat_p), m
    assert torch.equal(coh.exp_avg[m], tr.exp_avg) and torch.equal(coh.exp_avg_sq[m], tr.exp_avg_sq), m
    assert torch.equal(coh.step2[m, :2], tr.step2[:2]), m
    for s, want in enumerate(losses):
        if want is None:
            assert torch.equal(got_losses[s, m], got_losses[s - 1, m]) if words else torch.isnan(got_losses[s, m])
        else:
            assert torch.equal(got_losses[s, m:m + 1], want), (m, s)


@pytest.mark.parametrize("n,k", [(n, k) for n in (10, 11, 103) for k in (2, 5, 10)])
def test_kfold_indices(n, k):
    folds = kfold_indices(n, k, shuffle=True, seed=4)
    assert len(folds) == k
    allv = np.concatenate(folds)
    assert sorted(allv.tolist()) == list(range(n))                       # disjoint and covering
    sizes = [len(f) for f in folds]
    assert max(sizes) - min(sizes) <= 1
    again = kfold_indices(n, k, shuffle=True, seed=4)
    assert all(np.array_equal(a, b) for a, b in zip(folds, again))
    plain = kfold_indices(n, k, shuffle=False)
    assert np.array_equal(np.concatenate(plain), np.arange(n))
    with pytest.raises(ValueError):
        kfold_indices(n, n + 1)


def test_mismatched_members_raise():
    a, b = random_states(GINet, 28, 2)
    with pytest.raises(ValueError, match="'F'"):
        Cohort(GINet, [a, random_states(GINet, 20, 1)[0]], device="cpu", api=emu())
    e = dict(b)
    e["conv1.fc_attention.weight"] = torch.zeros(1, 40)
    with pytest.raises(ValueError, match="'conv1.fc_attention.weight'"):
        Cohort(GINet, [a, e], device="cpu", api=emu())
    with pytest.raises(ValueError):
        Cohort(GINet, [], device="cpu", api=emu())
    with pytest.raises(ValueError, match="lr"):
        Cohort(GINet, [a, b], lr=[0.1, 0.2, 0.3], device="cpu", api=emu())


def test_emulated_plan_is_none():
    p = emu().cohort_step_plan(3, _lib.GINET, 28, 60, 200, 30, 64, 128, 1, 16, _lib.TOPO_HIER | _lib.TOPO_TILES)
    assert p.family == _lib.STEP_FAMILY_NONE


@pytest.mark.parametrize("name", sorted(NETS))
def test_member_equals_single_trainer(name):
    """test 1 in its separate-path form: different mini-batches per member, a short last one, a member without one"""
    Net = NETS[name]
    graphs = fixture_graphs(NODE_FEATURES)
    rs = ResidentGraphSet(graphs, "cpu", api=emu())
    K, T, B = 3, 6, 4
    sds = random_states(Net, rs.n_feat, K, seed=5)
    lrs, seeds = [0.01, 0.02, 0.005], [11, 12, 13]
    coh = Cohort(Net, sds, lr=lrs, seeds=seeds, device="cpu", api=emu())
    rows = schedule(len(graphs), K, T, B)
    # (train_step returns the members' loss words: a member without a mini-batch keeps its last one)
    got = torch.stack([coh.train_step(rs, row).clone() for row in rows])
    assert coh.last_path == "separate" and coh.last_reason
    for m in range(K):
        tr, losses = single_trajectory(Net, sds[m], rs, [row[m] for row in rows], lrs[m], seeds[m], emu())
        assert_member_equals(coh, m, tr, losses, got, words=True)
        if len(rows[-1][m]):
            assert torch.equal(coh.last_pred[m], tr.last_pred)
    assert int(coh.step2[K - 1, 0]) == T - 1 and int(coh.step2[0, 0]) == T
    assert coh.faults().tolist() == [0] * K
    coh.raise_on_faults()


@pytest.mark.parametrize("name", ["GINet", "sGAT"])
def test_member_hyper_parameters(name):
    """non-default betas / eps and a learning rate per member: 3 steps of 4 graphs, every member bit-equal to a trainer of its
    own with those hyper-parameters (itself pinned to float64 by test_adam.py)"""
    Net = NETS[name]
    graphs = fixture_graphs(NODE_FEATURES)
    rs = ResidentGraphSet(graphs, "cpu", api=emu())
    K, betas, eps = 3, (0.5, 0.9), 1e-3
    sds = random_states(Net, rs.n_feat, K, seed=8)
    lrs, seeds = [0.1, 0.01, 0.001], [21, 22, 23]
    coh = Cohort(Net, sds, lr=lrs, seeds=seeds, device="cpu", api=emu(), betas=betas, eps=eps)
    rows = schedule(len(graphs), K, 3, 4)
    got = torch.stack([coh.train_step(rs, row).clone() for row in rows])
    for m in range(K):
        tr, losses = single_trajectory(Net, sds[m], rs, [row[m] for row in rows], lrs[m], seeds[m], emu(), betas=betas, eps=eps)
        assert (tr.lr, tuple(tr.betas), tr.eps) == (lrs[m], betas, eps)
        assert_member_equals(coh, m, tr, losses, got, words=True)
    assert not torch.equal(coh.exp_avg_sq[0], torch.zeros_like(coh.exp_avg_sq[0]))


def test_learning_rates_and_seeds():
    """test 5: equal starts and mini-batches, different lr -> the members diverge, each equal to its single trainer; members
    equal in everything stay bit-identical"""
    graphs = fixture_graphs(NODE_FEATURES)
    rs = ResidentGraphSet(graphs, "cpu", api=emu())
    sd = random_states(GINet, rs.n_feat, 1, seed=2)[0]
    lrs, seeds = [0.01, 0.03, 0.01, 0.01], [5, 5, 5, 9]
    coh = Cohort(GINet, [sd] * 4, lr=lrs, seeds=seeds, device="cpu", api=emu())
    orders = [list(range(len(graphs)))] * 4
    losses = torch.cat([coh.train_epoch(rs, orders, 4) for _ in range(2)])
    assert torch.equal(coh.params[0], coh.params[2]) and torch.equal(losses[:, 0], losses[:, 2])
    assert not torch.equal(coh.params[0], coh.params[1])
    assert not torch.equal(coh.params[0], coh.params[3])                  # (another dropout stream)
    batches = [orders[0][lo:lo + 4] for lo in range(0, len(graphs), 4)] * 2
    for m in range(4):
        tr, want = single_trajectory(GINet, sd, rs, batches, lrs[m], seeds[m], emu())
        assert_member_equals(coh, m, tr, want, losses)


def test_hand_over(tmp_path):
    """test 8: save -> NeuralNet(pretrained_model=paths) scores as an ensemble with the members' own outputs; ensemble()
    shares the parameters"""
    graphs = fixture_graphs(NODE_FEATURES)
    rs = ResidentGraphSet(graphs, "cpu", api=emu())
    coh = Cohort(GINet, 3, n_feat=rs.n_feat, device="cpu", api=emu())
    coh.train_epoch(rs, [list(range(10)), list(range(2, 10)), list(range(8))], 4)
    paths = coh.save([os.path.join(str(tmp_path), "fold%d.pt" % m) for m in range(3)], node=NODE_FEATURES, target='irmsd',
                     batch_size=4)
    nn = NeuralNet(DB, GINet, pretrained_model=paths, outdir=str(tmp_path), _api=emu(), device='cpu')
    store = nn.test(hdf5=None)
    got = np.asarray(store['ensemble_raw_outputs'])
    assert got.shape == (10, 3)
    ens = coh.ensemble()
    assert ens.params.data_ptr() == coh.params.data_ptr()
    shared = ens.predict(rs, batch_size=4)
    fresh = Ensemble(GINet, coh.state_dicts(), device="cpu", api=emu()).predict(rs, batch_size=4)
    assert torch.equal(shared, fresh)
    np.testing.assert_array_equal(got, shared.reshape(3, 10).t().numpy())
    # ... and it follows the cohort: one more epoch changes what the shared ensemble scores
    coh.train_epoch(rs, [list(range(10))] * 3, 4)
    assert not torch.equal(ens.predict(rs, batch_size=4), fresh)
    sd = torch.load(paths[1], map_location="cpu", weights_only=False)
    assert sd['optimizer']['state'] and sd['lr'] == 0.01 and sd['task'] == 'reg'


@pytest.mark.parametrize("name", ["GINet", "sGAT"])
def test_cross_validate(name, tmp_path):
    """test 9 in its separate-path form: fixture, k = 5, 3 epochs"""
    Net = NETS[name]
    nn = NeuralNet(DB, Net, node_feature=NODE_FEATURES, target='irmsd', batch_size=4, lr=0.01, outdir=str(tmp_path),
                   _api=emu(), device='cpu')
    if name == "GINet":
        nn.model.dropout = 0.0
    torch.manual_seed(21)
    res = nn.cross_validate(k=5, nepoch=3, validate=True, save_model=os.path.join(str(tmp_path), "cv"), seed=1)
    folds = res['folds']
    assert sorted(np.concatenate(folds).tolist()) == list(range(10)) and len(folds) == 5
    coh = res['cohort']
    assert coh.last_path == "separate"
    assert len(res['train_loss']) == 5 and all(len(v) == 3 for v in res['train_loss'])
    assert len(res['valid_loss']) == 5 and all(len(v) == 3 for v in res['valid_loss'])
    rs = res['set']
    for m in range(5):
        batches = [o[lo:lo + 4] for o in (ep[m] for ep in res['orders']) for lo in range(0, len(o), 4)]
        tr, _ = single_trajectory(Net, res['start'][m], rs, batches, 0.01, coh.seeds[m], emu(), dropout=0.0)
        assert torch.equal(coh.params[m], tr.flat_p), m
        # the fold's validation loss = that model's own evaluation of its held-out graphs
        held = folds[m].tolist()
        pred = tr.predict_cached(rs.topology_cache(need_weights=Net is sGAT), held).reshape(-1)
        want = float(torch.nn.functional.mse_loss(pred, rs.y[held]))
        assert res["valid_loss"][m][-1] == want, m
        assert res['metrics'][m] is not None
    assert len(res['paths']) == 5 and all(os.path.exists(p) for p in res['paths'])
    loaded = NeuralNet(DB, Net, pretrained_model=res['paths'], outdir=str(tmp_path), _api=emu(), device='cpu')
    assert loaded.ensemble is not None and loaded.ensemble.K == 5
