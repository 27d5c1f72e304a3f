"""Ensemble on the MI355X: the fused ensemble launch (K members per launch over one resident set and its cached topology)
gives, member by member, the bits of FusedTrainer.predict_cached with the one-workgroup-per-graph layout on the same mini-batches (every net, every feature-width class, K = 1 / 3 / 10), also at K x B
beyond one launch's resident workgroups (K = 10, batch 64) and on graphs beyond the staged LDS layout; the reference's ten fold models against
ensemble_treg.npz; NeuralNet(pretrained_model=[...]) on the fixture."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, NODE_FEATURES, golden, treg_graphs
import elementwise as ew
import deeprank_gnn_amd.synthetic as synth
from deeprank_gnn_amd import Ensemble
from deeprank_gnn_amd.ginet import GINet
from deeprank_gnn_amd.sGAT import sGAT
from deeprank_gnn_amd.foutnet import FoutNet
from deeprank_gnn_amd.resident import ResidentGraphSet
from deeprank_gnn_amd.trainer import FusedTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NETS = {"GINet": GINet, "sGAT": sGAT, "FoutNet": FoutNet}
# padded feature width -> a feature count of that class
WIDTHS = {16: 12, 32: 28, 48: 44, 64: 52}


def states(Net, F, K, seed):
    torch.manual_seed(seed)
    return [{k: v.clone() for k, v in Net(F, 1, 1).state_dict().items()} for _ in range(K)]


def graphs_of(n, F, n_nodes=60, n_pairs=120, n_internal=40, seed=0):
    return [synth.make_graph(seed + i, n_nodes=n_nodes + (i % 5), n_pairs=n_pairs, n_feat=F, n_c1=5, n_internal=n_internal)
            for i in range(n)]


def check_against_separate(Net, sds, graphs, B):
    """Ensemble.predict == per member FusedTrainer.predict_cached on the same mini-batches, bit for bit"""
    F = graphs[0].num_features
    rs = ResidentGraphSet(graphs, DEV)
    ens = Ensemble(Net, sds, device=DEV)
    got = ens.predict(rs, batch_size=B, cached=True)
    ens.raise_on_faults()
    assert ens.last_path == "fused", ens.last_reason
    cache = rs.topology_cache(need_weights=Net is sGAT)
    n = len(graphs)
    p, _, _, _ = ens.plan(cache, list(range(min(n, B))))
    assert p.family != 0 and p.wgs_per_graph == 1
    for k, sd in enumerate(sds):
        net = Net(F, 1, 1)
        net.load_state_dict(sd)
        tr = FusedTrainer(net.to(DEV), task="reg")
        tr.plan_overrides = {"force_wgs": 1}
        want = torch.cat([tr.predict_cached(cache, list(range(lo, min(n, lo + B)))).clone() for lo in range(0, n, B)])
        tr.check_faults()
        assert torch.isfinite(want).all()
        assert torch.equal(got[k], want), (Net.__name__, k)
    return got


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("width", sorted(WIDTHS))
@pytest.mark.parametrize("name", sorted(NETS))
def test_ensemble_equals_separate(name, width, K):
    F = WIDTHS[width]
    check_against_separate(NETS[name], states(NETS[name], F, K, seed=K * 100 + width), graphs_of(24, F), B=16)


def test_ensemble_past_resident_count():
    """GINet, K = 10 at batch 64: 640 workgroups per launch, more than stay resident at once at this LDS size -- the plan
    takes the one-workgroup-per-graph form (no workgroup waits for another); no fault bits, same bits.  Below the line
    (K = 1, batch 64) the single-model plan would take two workgroups per graph, the ensemble plan still one."""
    ens = Ensemble(GINet, states(GINet, 32, 2, seed=7), device=DEV)
    p = ens.api.ens_step_plan(10, ens.kind, 32, 70, 200, 64, ens.R, ens.H, 1, 64, 1 | 4)
    assert p.family != 0 and p.wgs_per_graph == 1
    single = ens.api.step_plan(ens.kind, 32, 70, 200, 64, ens.R, ens.H, 1, 64, 0, False, 1 | 4)
    assert single.wgs_per_graph == 2
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    # (1024-lane workgroups: at most two per CU by waves, fewer by LDS)
    assert 10 * 64 > cu * min(2, max(1, (160 * 1024) // int(p.lds_bytes)))
    check_against_separate(GINet, states(GINet, 32, 10, seed=7), graphs_of(128, 32), B=64)


@pytest.mark.parametrize("name", sorted(NETS))
def test_ensemble_from_memory_graphs(name):
    """~350-node graphs: the from-memory forms of the fused kernels"""
    g = graphs_of(6, 28, n_nodes=345, n_pairs=700, n_internal=330, seed=50)
    check_against_separate(NETS[name], states(NETS[name], 28, 3, seed=11), g, B=3)


def test_fold_models_match_reference():
    from deeprank_gnn_amd.data import Batch
    g = golden("ensemble_treg.npz")
    graphs = treg_graphs()
    sds = []
    for k in range(1, 11):
        pre = "fold%d/" % k
        sds.append({n[len(pre):]: torch.from_numpy(g[n].copy()) for n in g if n.startswith(pre)})
    ens = Ensemble(GINet, sds, device=DEV)
    pred = ens.predict(ResidentGraphSet(graphs, DEV), batch_size=6).cpu().numpy()
    ens.raise_on_faults()
    assert ens.last_path == "fused", ens.last_reason
    batch = Batch.from_data_list(graphs)
    stats = ew.new_stats()
    for k in range(10):
        ew.check("fold%d" % (k + 1), pred[k], g["pred"][k],
                 lambda k=k: ew.oracle64("GINet", sds[k], batch, batch.y)[0].numpy(), stats)
    ew.assert_arbiter_rate(stats, "ensemble folds")
    np.testing.assert_allclose(pred.mean(axis=0), g["mean"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(pred.std(axis=0), g["std"], rtol=1e-4, atol=1e-4)


def test_neuralnet_ensemble(tmp_path):
    from deeprank_gnn_amd.NeuralNet import NeuralNet
    db = os.path.join(GOLDEN, "fixture_1ATN.npz")
    paths = []
    for k, sd in enumerate(states(GINet, 28, 10, seed=5)):
        paths.append(os.path.join(str(tmp_path), "m%d.pt" % k))
        torch.save({'model': sd, 'optimizer': None, 'node': NODE_FEATURES, 'edge': ['dist'], 'target': 'irmsd',
                    'task': 'reg', 'classes': [0, 1], 'class_weight': None, 'batch_size': 4, 'percent': [1.0, 0.0],
                    'lr': 0.01, 'index': None, 'shuffle': True, 'threshold': 0.3, 'cluster_nodes': 'mcl',
                    'transform_sigmoid': False}, paths[-1])
    singles = [NeuralNet(db, GINet, pretrained_model=p, outdir=str(tmp_path)).test(hdf5=None) for p in paths]
    nn = NeuralNet(db, GINet, pretrained_model=paths, outdir=str(tmp_path))
    store = nn.test(hdf5=None)
    assert nn.ensemble.last_path == "fused", nn.ensemble.last_reason
    per = np.array([s['raw_outputs'] for s in singles]).T
    got = np.asarray(store['ensemble_raw_outputs'])
    assert got.shape == (10, 10)
    np.testing.assert_array_equal(got, per)
    np.testing.assert_allclose(store['outputs'], per.mean(axis=1), rtol=1e-6, atol=1e-7)
    assert nn.get_metrics('test', threshold=4.0) is not None
    assert 'ensemble_raw_outputs' not in dict(singles[0].items())
