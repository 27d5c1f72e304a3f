"""Cohort on the MI355X: the two cohort launches per step (K members over one resident set and its cached topology) give,
member by member, the bits of a FusedTrainer of its own with the one-workgroup-per-graph layout stepped on that member's
mini-batches alone -- parameters, both Adam moments, step words, last predictions and every step's loss -- for every net,
every feature-width class, K = 1 / 3 / 10, with different mini-batches per member, a short last one and a member that has none
in the last step; beyond one launch's resident workgroups; on from-memory graphs; for classification; per-member learning
rates and seeds; existing launches unchanged; reference parity directly; the hand-over to Ensemble / NeuralNet; and
cross-validation end to end."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLDEN, NODE_FEATURES
import deeprank_gnn_amd.synthetic as synth
from deeprank_gnn_amd import Cohort, Ensemble
from deeprank_gnn_amd.NeuralNet import NeuralNet
from deeprank_gnn_amd.ginet import GINet
from deeprank_gnn_amd.sGAT import sGAT
from deeprank_gnn_amd.foutnet import FoutNet
from deeprank_gnn_amd.resident import ResidentGraphSet
from deeprank_gnn_amd.trainer import FusedTrainer
from oracle import cpu_ref
from test_gpu_ensemble import WIDTHS, graphs_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NETS = {"GINet": GINet, "sGAT": sGAT, "FoutNet": FoutNet}
DB = os.path.join(GOLDEN, "fixture_1ATN.npz")


def states(Net, F_, K, seed, O=1):
    torch.manual_seed(seed)
    return [{k: v.clone() for k, v in Net(F_, O, 1).state_dict().items()} for _ in range(K)]


def schedule(n, K, T, B, seed=3):
    """[T][K] mini-batches over n graphs, different per member: a short last mini-batch, and (K > 1) the last member has none
    in the last step"""
    rng = np.random.RandomState(seed)
    rows = []
    for s in range(T):
        row = []
        for m in range(K):
            size = B if s < T - 1 else max(1, B - 1 - m % 3)
            if s == T - 1 and m == K - 1 and K > 1:
                size = 0
            row.append(rng.permutation(n)[:size].tolist())
        rows.append(row)
    return rows


def single(Net, sd, rs, batches, lr, seed, task="reg", class_weights=None, O=1, dropout=None, overrides={"force_wgs": 1},
           betas=(0.9, 0.999), eps=1e-8):
    """a FusedTrainer of its own over one member's mini-batches: (trainer, its loss per step, None where it had none)"""
    net = Net(rs.n_feat, O, 1)
    net.load_state_dict(sd)
    if dropout is not None:
        net.dropout = dropout
    tr = FusedTrainer(net.to(DEV), lr=lr, task=task, class_weights=class_weights, seed=seed, betas=betas, eps=eps)
    tr.plan_overrides = dict(overrides)
    cache = rs.topology_cache(need_weights=Net is sGAT)
    losses = [tr.train_step_cached(cache, ids).clone() if len(ids) else None for ids in batches]
    tr.check_faults()
    return tr, losses


def check_cohort(Net, sds, graphs, rows, lrs=0.01, seeds=None, task="reg", class_weights=None, O=1, y=None,
                 betas=(0.9, 0.999), eps=1e-8):
    """cohort steps over ``rows`` ([T][K] mini-batches) == per member a single trainer on that member's mini-batches"""
    K = len(sds)
    rs = ResidentGraphSet(graphs, DEV)
    if y is not None:
        rs.set_targets(y)
    seeds = list(range(40, 40 + K)) if seeds is None else seeds
    lrs = [lrs] * K if not isinstance(lrs, list) else lrs
    coh = Cohort(Net, sds, lr=lrs, seeds=seeds, task=task, class_weights=class_weights, device=DEV, betas=betas, eps=eps)
    cache = rs.topology_cache(need_weights=Net is sGAT)
    got = torch.stack([coh.train_step(cache, row).clone() for row in rows])
    assert coh.last_path == "fused", coh.last_reason
    p, _, _, _ = coh.plan(cache, sorted({i for row in rows for b in row for i in b}), max(len(b) for b in rows[0]))
    assert p.family != 0 and p.wgs_per_graph == 1
    assert coh.faults().cpu().tolist() == [0] * K
    coh.raise_on_faults()
    for m in range(K):
        tr, losses = single(Net, sds[m], rs, [row[m] for row in rows], lrs[m], seeds[m], task, class_weights, O,
                            betas=betas, eps=eps)
        assert torch.equal(coh.params[m], tr.flat_p), (Net.__name__, m, "parameters")
        assert torch.equal(coh.exp_avg[m], tr.exp_avg) and torch.equal(coh.exp_avg_sq[m], tr.exp_avg_sq), (Net.__name__, m)
        assert torch.equal(coh.step2[m, :2], tr.step2[:2]), (Net.__name__, m, "step words")
        assert torch.isfinite(coh.params[m]).all()
        for s, want in enumerate(losses):
            if want is not None:
                assert torch.equal(got[s, m:m + 1], want), (Net.__name__, m, s, "loss")
            elif s > 0:
                assert torch.equal(got[s, m], got[s - 1, m])              # (not stepped: the loss word is unchanged)
        last = max(s for s, b in enumerate(r[m] for r in rows) if len(b))
        if last == len(rows) - 1:
            assert torch.equal(coh.last_pred[m], tr.last_pred), (Net.__name__, m, "pred")
    return coh, rs


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("width", sorted(WIDTHS))
@pytest.mark.parametrize("name", sorted(NETS))
def test_member_equals_single_trainer(name, width, K):
    """GINet runs with its default dropout 0.4: every member has its own dropout stream and step index"""
    F_ = WIDTHS[width]
    coh, _ = check_cohort(NETS[name], states(NETS[name], F_, K, seed=K * 100 + width), graphs_of(24, F_),
                          schedule(24, K, 6, 16))
    if K > 1:
        assert int(coh.step2[K - 1, 0]) == 5 and int(coh.step2[0, 0]) == 6


@pytest.mark.parametrize("name", ["GINet", "sGAT"])
def test_member_hyper_parameters(name):
    """non-default betas / eps and a learning rate per member reach the member table: 3 steps of 4 graphs, every member
    bit-equal to a trainer of its own with those hyper-parameters (itself pinned to float64 by test_gpu_adam.py)"""
    coh, _ = check_cohort(NETS[name], states(NETS[name], 28, 3, seed=17), graphs_of(8, 28), schedule(8, 3, 3, 4),
                          lrs=[0.1, 0.01, 0.001], betas=(0.5, 0.9), eps=1e-3)
    assert not torch.equal(coh.exp_avg_sq[0], torch.zeros_like(coh.exp_avg_sq[0]))


# 2 -------------------------------------------------------------------------------------------------------------------------
def test_cohort_past_resident_count():
    """GINet, K = 10 at batch 64: 640 workgroups per launch, more than stay resident at once at this LDS size; no workgroup
    waits for another, no fault bits, same bits"""
    coh = Cohort(GINet, states(GINet, 32, 2, seed=7), device=DEV)
    p = coh.api.cohort_step_plan(10, coh.kind, 32, 70, 200, 64, coh.R, coh.H, 1, 64, 1 | 4)
    assert p.family != 0 and p.wgs_per_graph == 1
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    # (1024-lane workgroups: at most two per CU by waves, fewer by LDS)
    assert 10 * 64 > cu * min(2, max(1, (160 * 1024) // int(p.lds_bytes)))
    check_cohort(GINet, states(GINet, 32, 10, seed=7), graphs_of(128, 32), schedule(128, 10, 6, 64))


# 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NETS))
def test_cohort_from_memory_graphs(name):
    """~350-node graphs: the from-memory forms of the fused kernels"""
    g = graphs_of(6, 28, n_nodes=345, n_pairs=700, n_internal=330, seed=50)
    check_cohort(NETS[name], states(NETS[name], 28, 3, seed=11), g, schedule(6, 3, 6, 3))


# 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NETS))
def test_cohort_classification(name):
    graphs = graphs_of(24, 28)
    y = torch.tensor([i % 2 for i in range(24)], dtype=torch.int64)
    check_cohort(NETS[name], states(NETS[name], 28, 3, seed=13, O=2), graphs, schedule(24, 3, 6, 16), task="class",
                 class_weights=[0.3, 0.7], O=2, y=y)


# 5 -------------------------------------------------------------------------------------------------------------------------
def test_learning_rates_and_seeds():
    """equal starts and equal mini-batches (the launch then carries the host-known sizes): different lr or seed -> the members
    diverge and each equals its single trainer; members equal in everything stay bit-identical to each other"""
    sd = states(GINet, 28, 1, seed=2)[0]
    rows = [[b] * 4 for b in (r[0] for r in schedule(24, 1, 6, 16))]
    coh, _ = check_cohort(GINet, [sd] * 4, graphs_of(24, 28), rows, lrs=[0.01, 0.03, 0.01, 0.01], seeds=[5, 5, 5, 9])
    assert torch.equal(coh.params[0], coh.params[2]) and torch.equal(coh.exp_avg_sq[0], coh.exp_avg_sq[2])
    assert not torch.equal(coh.params[0], coh.params[1])
    assert not torch.equal(coh.params[0], coh.params[3])


# 6 -------------------------------------------------------------------------------------------------------------------------
def test_existing_launches_unchanged():
    """a plain FusedTrainer (default plan) gives the same parameter bits whether or not a Cohort was built and stepped in the
    same process before it: the shared update body and the launch set-up changed nothing for it"""
    graphs = [synth.make_graph(i) for i in range(16)]
    sd = states(GINet, 32, 1, seed=3)[0]
    rs = ResidentGraphSet(graphs, DEV)
    batches = [list(range(16)), list(range(8)), list(range(4, 16)), list(range(16)), list(range(2, 14))]
    before, _ = single(GINet, sd, rs, batches, 0.01, 17, overrides={})
    coh = Cohort(GINet, states(GINet, 32, 3, seed=4), device=DEV)
    coh.train_epoch(rs, [list(range(16))] * 3, 8)
    assert coh.last_path == "fused", coh.last_reason
    after, _ = single(GINet, sd, rs, batches, 0.01, 17, overrides={})
    assert torch.equal(before.flat_p, after.flat_p) and torch.equal(before.exp_avg_sq, after.exp_avg_sq)


# 7 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net_name", ["GINet", "sGAT", "FoutNet"])
def test_five_cohort_steps_match_oracle_training(net_name):
    """tests/test_gpu_trainer.py::test_five_native_steps_match_oracle_training for a cohort of 3: member 0 is that test's case
    (16 graphs, seed 9); members 1 and 2 take seeds 10 and 11 and step graphs 0 - 11 and 4 - 15.  Each member against its own
    oracle + torch.optim.Adam loop on the collated batch of its graphs, with that test's tolerances."""
    from deeprank_gnn_amd.data import Batch
    graphs = [synth.make_graph(i, n_nodes=120, n_pairs=260) for i in range(16)]
    member_ids = [list(range(16)), list(range(12)), list(range(4, 16))]
    params = [cpu_ref.init_params(net_name, 32, 1, 1, seed=9 + m) for m in range(3)]
    coh = Cohort(NETS[net_name], params, lr=0.01, device=DEV)
    for net in coh.nets:
        if hasattr(net, "dropout"):
            net.dropout = 0.0                      # dropout forced to 0 for parity
    rs = ResidentGraphSet(graphs, DEV)
    got = torch.stack([coh.train_step(rs, member_ids).clone() for _ in range(5)]).cpu().numpy()
    assert coh.last_path == "fused", coh.last_reason
    coh.raise_on_faults()
    kw = {"looped": False} if net_name == "FoutNet" else {}
    sds = coh.state_dicts()
    for m in range(3):
        batch_cpu = Batch.from_data_list([graphs[i] for i in member_ids[m]])
        leaves = {k: v.clone().requires_grad_(True) for k, v in params[m].items()}
        opt = torch.optim.Adam(list(leaves.values()), lr=0.01)
        for it in range(5):
            opt.zero_grad()
            pred = cpu_ref.FORWARD[net_name](leaves, batch_cpu, **kw)
            loss = F.mse_loss(pred.reshape(-1), batch_cpu.y)
            loss.backward()
            opt.step()
            print("member %d step %d: cohort loss %.8g oracle %.8g" % (m, it, got[it, m], float(loss.detach())))
            np.testing.assert_allclose(got[it, m], float(loss.detach()), rtol=1e-4)
        for k, v in leaves.items():
            np.testing.assert_allclose(sds[m][k].numpy(), v.detach().numpy(), rtol=1e-4, atol=1e-5, err_msg="%d %s" % (m, k))


# 8 -------------------------------------------------------------------------------------------------------------------------
def test_hand_over(tmp_path):
    from helpers import fixture_graphs
    graphs = fixture_graphs(NODE_FEATURES)
    rs = ResidentGraphSet(graphs, DEV)
    coh = Cohort(GINet, 3, n_feat=rs.n_feat, device=DEV)
    coh.train_epoch(rs, [list(range(10)), list(range(2, 10)), list(range(8))], 4)
    assert coh.last_path == "fused", coh.last_reason
    paths = coh.save([os.path.join(str(tmp_path), "fold%d.pt" % m) for m in range(3)], node=NODE_FEATURES, target='irmsd',
                     batch_size=4)
    nn = NeuralNet(DB, GINet, pretrained_model=paths, outdir=str(tmp_path))
    store = nn.test(hdf5=None)
    got = np.asarray(store['ensemble_raw_outputs'])
    assert got.shape == (10, 3)
    for m, tr in enumerate(coh.trainers):
        own = tr.predict_cached(rs.topology_cache(), list(range(10))).reshape(-1).cpu().numpy()
        np.testing.assert_array_equal(got[:, m], own)
    ens = coh.ensemble()
    assert ens.params.data_ptr() == coh.params.data_ptr()
    shared = ens.predict(rs, batch_size=4)
    assert ens.last_path == "fused", ens.last_reason
    fresh = Ensemble(GINet, coh.state_dicts(), device=DEV).predict(rs, batch_size=4)
    assert torch.equal(shared, fresh)


# 9 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["GINet", "sGAT"])
def test_cross_validate(name, tmp_path):
    Net = NETS[name]
    nn = NeuralNet(DB, Net, node_feature=NODE_FEATURES, target='irmsd', batch_size=4, lr=0.01, outdir=str(tmp_path))
    if name == "GINet":
        nn.model.dropout = 0.0
    torch.manual_seed(21)
    res = nn.cross_validate(k=5, nepoch=3, validate=True, save_model=os.path.join(str(tmp_path), "cv"), seed=1)
    folds, coh, rs = res['folds'], res['cohort'], res['set']
    assert len(folds) == 5 and sorted(np.concatenate(folds).tolist()) == list(range(10))
    assert coh.last_path == "fused", coh.last_reason
    assert all(len(v) == 3 for v in res['train_loss']) and all(len(v) == 3 for v in res['valid_loss'])
    cache = rs.topology_cache(need_weights=Net is sGAT)
    for m in range(5):
        batches = [o[lo:lo + 4] for o in (ep[m] for ep in res['orders']) for lo in range(0, len(o), 4)]
        tr, _ = single(Net, res['start'][m], rs, batches, 0.01, coh.seeds[m], dropout=0.0)
        assert torch.equal(coh.params[m], tr.flat_p), m
        held = folds[m].tolist()
        pred = tr.predict_cached(cache, held).reshape(-1)
        want = float(F.mse_loss(pred, rs.y[held]))
        assert res['valid_loss'][m][-1] == want, m
        assert res['metrics'][m] is not None
    assert len(res['paths']) == 5 and all(os.path.exists(p) for p in res['paths'])
    loaded = NeuralNet(DB, Net, pretrained_model=res['paths'], outdir=str(tmp_path))
    assert loaded.ensemble is not None and loaded.ensemble.K == 5
