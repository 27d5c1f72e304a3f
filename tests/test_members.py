"""The one definition of "K members of one net over packed storage" (members.py) and FusedTrainer.adopt_storage under it,
kernels emulated on CPU: a trainer on caller-owned buffers is the trainer it would have been on its own, the cohort's and its
ensemble's member tables name the same parameter rows, Cohort.save writes NeuralNet.save_model's dictionary."""
import ctypes
import os

import pytest
import torch

from helpers import GOLDEN, NODE_FEATURES, fixture_graphs
from emu_api import emu
from deeprank_gnn_amd import Cohort, _lib
from deeprank_gnn_amd.NeuralNet import NeuralNet
from deeprank_gnn_amd.ginet import GINet
from deeprank_gnn_amd.sGAT import sGAT
from deeprank_gnn_amd.foutnet import FoutNet
from deeprank_gnn_amd.resident import ResidentGraphSet
from deeprank_gnn_amd.trainer import FusedTrainer

DB = os.path.join(GOLDEN, "fixture_1ATN.npz")


def conv_pointers(desc):
    """the non-null parameter addresses of a drgnn_net_desc"""
    out = []
    for conv in (desc.conv1, desc.conv2):
        for b in range(desc.n_branch):
            out += [p for p in (conv[b].w_nbr, conv[b].w_self, conv[b].bias) if p]
    return out


def inside(ptr, t):
    return t.data_ptr() <= ptr < t.data_ptr() + 4 * t.numel()


def check_adopt_storage(Net, graphs, device, api, B=4, steps=3, wgs=None):
    """A trainer put on external rows by adopt_storage (descriptor cache warm) against a fresh trainer of the same seed over
    the same ``steps`` cached mini-batches of ``B`` graphs; then the inference-only form on the trained parameters.  Returns
    the trainers (fresh, adopted, inference-only)."""
    rs = ResidentGraphSet(graphs, device, api=api)
    cache = rs.topology_cache(need_weights=Net is sGAT)
    F, n = rs.n_feat, len(graphs)

    def make():
        torch.manual_seed(3)
        return FusedTrainer(Net(F, 1, 1).to(device), lr=0.01, task="reg", seed=17, api=api)
    fresh, tr, inf = make(), make(), make()
    old_desc = tr._descs(F)[2]
    assert all(inside(p, tr.flat_p) for p in conv_pointers(old_desc))
    own = {"p": tr.flat_p, "m": tr.exp_avg, "v": tr.exp_avg_sq, "step2": tr.step2, "loss": tr.loss}
    start = tr.flat_p.clone()
    ext_p = torch.stack([tr.flat_p])                                      # [1, P]: the values are in place, as a pack's
    ext_g, ext_m, ext_v = (torch.zeros_like(ext_p) for _ in range(3))
    ext_step2 = torch.zeros((1, 4), dtype=torch.int32, device=device)
    ext_loss = torch.zeros(1, dtype=torch.float32, device=device)
    tr.adopt_storage(ext_p[0], ext_g[0], ext_m[0], ext_v[0], ext_step2[0], ext_loss)
    desc = tr._descs(F)[2]
    assert conv_pointers(desc) and all(inside(p, ext_p) for p in conv_pointers(desc))
    assert all(inside(p.data_ptr(), ext_p) and inside(p.grad.data_ptr(), ext_g) for p in tr.net.parameters())
    assert all(inside(g.data_ptr(), ext_g) for g in tr.live_grads)
    for s in range(steps):
        ids = [(s * B + j) % n for j in range(B)]
        if wgs is not None:
            assert tr._cached_prepare(cache, ids)["plan"].wgs_per_graph == wgs
        want = fresh.train_step_cached(cache, ids).clone()
        got = tr.train_step_cached(cache, ids)
        assert got.data_ptr() == ext_loss.data_ptr() and torch.equal(got, want), s
        assert torch.equal(tr.last_pred, fresh.last_pred), s
    assert torch.equal(ext_p[0], fresh.flat_p) and not torch.equal(ext_p[0], start)
    assert torch.equal(ext_m[0], fresh.exp_avg) and torch.equal(ext_v[0], fresh.exp_avg_sq)
    assert torch.equal(ext_step2[0, :2], fresh.step2[:2]) and int(tr.step) == steps
    assert torch.equal(ext_loss, fresh.loss)
    # the adopted buffers are the trainer's, its former ones are left as they were
    assert (tr.flat_p.data_ptr(), tr.flat_g.data_ptr(), tr.exp_avg.data_ptr(), tr.exp_avg_sq.data_ptr(), tr.step2.data_ptr()) == \
        (ext_p.data_ptr(), ext_g.data_ptr(), ext_m.data_ptr(), ext_v.data_ptr(), ext_step2.data_ptr())
    assert torch.equal(own["p"], start) and not own["m"].any() and not own["v"].any()
    assert not own["step2"].any() and not own["loss"].any()
    # inference only: the trained parameters alone
    inf.adopt_storage(ext_p[0])
    assert inf.flat_g is None and inf.exp_avg is None and inf.exp_avg_sq is None
    assert all(p.grad is None and inside(p.data_ptr(), ext_p) for p in inf.net.parameters())
    ids = list(range(B))
    assert torch.equal(inf.predict_cached(cache, ids), fresh.predict_cached(cache, ids))
    with pytest.raises(_lib.DrgnnError):
        inf.train_step_cached(cache, ids)
    return fresh, tr, inf


@pytest.mark.parametrize("Net", [GINet, sGAT])
def test_adopt_storage(Net):
    check_adopt_storage(Net, fixture_graphs(NODE_FEATURES), "cpu", emu())


def test_adopt_storage_needs_both_moments():
    tr = FusedTrainer(GINet(28, 1, 1), api=emu())
    with pytest.raises(ValueError):
        tr.adopt_storage(tr.flat_p, tr.flat_g, tr.exp_avg)
    with pytest.raises(ValueError):
        tr.adopt_storage(tr.flat_p, exp_avg=tr.exp_avg, exp_avg_sq=tr.exp_avg_sq)


@pytest.mark.parametrize("Net", [GINet, sGAT])
def test_ensemble_without_cached_topology(Net):
    """predict(cached=False): every member's own native inference loop, on trainers without gradient or Adam buffers (the
    members of an Ensemble are inference only) -- the outputs of the cached path"""
    from deeprank_gnn_amd import Ensemble
    rs = ResidentGraphSet(fixture_graphs(NODE_FEATURES), "cpu", api=emu())
    torch.manual_seed(1)
    ens = Ensemble(Net, [{k: v.clone() for k, v in Net(rs.n_feat, 1, 1).state_dict().items()} for _ in range(2)],
                   device="cpu", api=emu())
    assert all(tr.flat_g is None for tr in ens.trainers)
    plain = ens.predict(rs, batch_size=4, cached=False)
    assert ens.last_path == "separate" and "no cached topology" in ens.last_reason
    assert torch.equal(plain, ens.predict(rs, batch_size=4, cached=True))


def test_member_tables_name_the_same_rows():
    """entry m of the cohort's table and of its ensemble's: the same net descriptor and head pointers, inside params[m]"""
    rs = ResidentGraphSet(fixture_graphs(NODE_FEATURES), "cpu", api=emu())
    coh = Cohort(FoutNet, 3, n_feat=rs.n_feat, device="cpu", api=emu())
    ens = coh.ensemble()
    size = ctypes.sizeof(_lib.EnsMember)

    def entries(table, Member):
        return (Member * 3).from_buffer_copy(table.numpy().tobytes())
    coh._ensure(4)
    prefix = [bytes(e)[:size] for e in entries(coh._table, _lib.CohortMember)]
    ens_entries = entries(ens.table, _lib.EnsMember)
    for m in range(3):
        e = ens_entries[m]
        assert bytes(e) == prefix[m], m
        ptrs = conv_pointers(e.net) + [e.w1, e.b1, e.w2, e.b2]
        assert len(ptrs) > 4 and all(inside(p, coh.params[m]) for p in ptrs), m
    coh._ensure(8)
    grown = entries(coh._table, _lib.CohortMember)
    assert coh._cap == 8 and [bytes(e)[:size] for e in grown] == prefix
    assert all(grown[m].flat_param == coh.params[m].data_ptr() for m in range(3))


def test_cohort_save_has_save_model_keys(tmp_path):
    coh = Cohort(GINet, 2, n_feat=fixture_graphs(NODE_FEATURES)[0].num_features, device="cpu", api=emu())
    paths = coh.save([os.path.join(str(tmp_path), "m%d.pt" % m) for m in range(2)])
    nn = NeuralNet(DB, GINet, node_feature=NODE_FEATURES, target='irmsd', batch_size=4, outdir=str(tmp_path), _api=emu(),
                   device='cpu')
    single = os.path.join(str(tmp_path), "single.pth.tar")
    nn.save_model(single)
    keys = set(torch.load(single, map_location="cpu", weights_only=False))
    assert {"model", "optimizer", "node", "transform_sigmoid"} <= keys
    for p in paths:
        assert set(torch.load(p, map_location="cpu", weights_only=False)) == keys
