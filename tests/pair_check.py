"""The launch pair -- k_net forward / backward with head_graph inside, train_update, k_head for inference -- at the shapes
ONLY it serves: more than 64 node features, a head other than the reference's fc1 128 / 64, ``x.requires_grad``.  Shared by
the emulated (test_emu_launch_pair.py) and the MI355X test (test_gpu_launch_pair.py).

Every number is compared with oracle/cpu_ref.py under tests/elementwise.py: |got - ref| <= 1e-4 + 1e-4 |ref| per element, the
float64 oracle as arbiter for at most 0.1 % of the elements.  Each case prints its arbiter count (``PAIR ...`` lines).

On the device the checker asserts, before a launch, that the launch is the pair by itself (``_can_fuse`` False, plan family
NONE) and which scratch regime of k_net it is (``regime``, from drgnn_net_lds_bytes against the LDS limit).  The emulation
build's plan answers with its stand-in step for some of these shapes; there the trainer is told to take the pair
(``fused_step = False``), whose per-graph routines are the device's own source.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from deeprank_gnn_amd import _lib
from deeprank_gnn_amd.data import Batch
from deeprank_gnn_amd.topology import Topology
from deeprank_gnn_amd.trainer import FusedTrainer
from elementwise import Lazy64, assert_arbiter_rate, check, check_step, new_stats
from oracle import cpu_ref

KIB = 1024
KINDS = {"GINet": _lib.GINET, "sGAT": _lib.SGAT, "FoutNet": _lib.FOUT}
CLASS_W = [0.2, 0.5, 0.3]


def nets():
    from deeprank_gnn_amd.ginet import GINet
    from deeprank_gnn_amd.sGAT import sGAT
    from deeprank_gnn_amd.foutnet import FoutNet
    return {"GINet": GINet, "sGAT": sGAT, "FoutNet": FoutNet}


def fw_of(net_name):
    return {"looped": False} if net_name == "FoutNet" else {}


def sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def shape_of(n_nodes):
    """synthetic.make_graph proportions of tests/test_gpu_width_classes.py"""
    return dict(n_nodes=n_nodes, n_pairs=(5 * n_nodes) // 2, n_c1=max(4, n_nodes // 12), n_internal=(7 * n_nodes) // 4)


@functools.lru_cache(maxsize=None)
def _graphs(n_feat, n_nodes, B):
    import deeprank_gnn_amd.synthetic as synth
    return tuple(synth.make_graph(i, n_feat=n_feat, **shape_of(n_nodes)) for i in range(B))


def syn_batch(n_feat, n_nodes, B):
    return Batch.from_data_list(list(_graphs(n_feat, n_nodes, B)))


def ragged(n_feat, seed=5):
    from step_check import ragged_batch
    batch = ragged_batch(seed, n_feat)
    batch.y = torch.arange(batch.num_graphs, dtype=torch.float32) * 0.3 - 1.0
    return batch


def make_params(net_name, n_feat, H=None, O=1, seed=41):
    """Oracle parameters; ``H``: a head of that many hidden units instead of the reference's (nn.Linear's init bounds)."""
    params = cpu_ref.init_params(net_name, n_feat, O, 1, seed=seed)
    if H is not None:
        R = params["fc1.weight"].shape[1]
        gen = torch.Generator().manual_seed(seed + 1000 * H + O)
        params["fc1.weight"] = cpu_ref._uniform((H, R), R, gen)
        params["fc1.bias"] = cpu_ref._uniform((H,), R, gen)
        params["fc2.weight"] = cpu_ref._uniform((O, H), H, gen)
        params["fc2.bias"] = cpu_ref._uniform((O,), H, gen)
    return params


def build_net(net_name, params, device):
    """The model class with the head's layers replaced to the parameters' shapes, loaded strict, dropout 0."""
    n_feat = {"GINet": lambda: params["conv1.fc.weight"].shape[1], "sGAT": lambda: params["conv1.weight"].shape[0] // 2,
              "FoutNet": lambda: params["conv1.Wc"].shape[0]}[net_name]()
    H, R = params["fc1.weight"].shape
    O = params["fc2.weight"].shape[0]
    net = nets()[net_name](n_feat, O, 1)
    if net.fc1.out_features != H:
        net.fc1 = torch.nn.Linear(R, H)
        net.fc2 = torch.nn.Linear(H, O)
    net.load_state_dict(params, strict=True)
    if hasattr(net, "dropout"):
        net.dropout = 0.0
    return net.to(device)


def targets(batch_cpu, task):
    if task == "class":
        batch_cpu.y = torch.tensor([k % 3 for k in range(batch_cpu.num_graphs)])
    return batch_cpu


def regime(api, net_name, n_feat, topo, head):
    """(regime, forward bytes, backward bytes, head staged) of a launch on ``topo``: which instance of k_net the forward / the
    backward is -- (i) both from LDS with >= 40 KiB to spare, (ii) both from LDS, the backward within 8 KiB of the limit,
    (iii) forward from LDS, backward from global scratch, (iv) both from global scratch, else 'other' -- and whether the
    backward keeps the head's weights in LDS (net_launch: when drgnn_net_head_stage_bytes more still fit; the reference heads do
    in (i) and do not in (ii))."""
    fwd, bwd = (api.net_lds_bytes(KINDS[net_name], n_feat, topo.max_nodes, topo.max_edges, topo.max_c0, b) for b in (False, True))
    R, H, O = head
    stage = api.net_head_stage_bytes(R, H, O)
    spare = _lib.LDS_LIMIT - bwd
    staged = 0 <= stage <= spare
    if fwd > _lib.LDS_LIMIT:
        assert bwd > _lib.LDS_LIMIT
        return "iv", fwd, bwd, staged
    if bwd > _lib.LDS_LIMIT:
        return "iii", fwd, bwd, staged
    if spare >= 40 * KIB:
        return "i", fwd, bwd, staged
    if spare <= 8 * KIB:
        return "ii", fwd, bwd, staged
    return "other", fwd, bwd, staged


def grads_of(net):
    return {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters()}


def check_pair_step(net_name, batch_cpu, device, api=None, params=None, task="reg", want_regime=None, co_build=False,
                    dropout=None, want_passes=False, where=""):
    """One mini-batch through compute_gradients / predict / compute_gradients again: loss, predictions, every gradient against
    the oracle; inference against the training launch's predictions; the second step gives the first one's bits.
    ``want_passes``: the head is too wide for k_head to stage whole, so inference must go over the hidden units in passes
    (asserted from drgnn_head_pass_units).  Returns the element statistics."""
    on_device = api is None
    kw = {} if on_device else {"api": api}
    n_feat = int(batch_cpu.x.shape[1])
    if params is None:
        params = make_params(net_name, n_feat, None, 1 if task == "reg" else 3)
    H, R = params["fc1.weight"].shape
    O = params["fc2.weight"].shape[0]
    batch_cpu = targets(batch_cpu, task)
    fw = dict(fw_of(net_name))
    fw64 = dict(fw)
    cw = None
    if task == "class":
        cw = torch.tensor(CLASS_W)
        fw["class_weights"] = fw64["class_weights"] = cw
    mask = None
    if dropout is not None:
        gen = torch.Generator().manual_seed(77)
        mask = (torch.rand((batch_cpu.num_graphs, H), generator=gen) >= dropout).float()      # seeded keep decisions
        fw.update(dropout=dropout, drop_mask=mask)
        fw64.update(dropout=dropout, drop_mask=mask.double())
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, task=task, **fw)
    lazy = Lazy64(net_name, params, batch_cpu, task=task, **fw64)
    net = build_net(net_name, params, device)
    tr = FusedTrainer(net, lr=0.01, task=task, class_weights=None if cw is None else cw.to(device), **kw)
    assert (tr.R, tr.H, tr.O) == (R, H, O)
    if mask is not None:
        net.dropout = dropout
        tr.drop_mask = mask.to(device).contiguous()
    if not on_device:
        tr.fused_step = False
    batch = batch_cpu.clone().to(device)
    need_w = net_name == "sGAT"
    topo = Topology.from_batch(batch, need_weights=need_w, **kw)
    nxt = Topology.from_batch(batch, need_weights=need_w, build=False, **kw) if co_build else None
    assert not tr._can_fuse(topo, n_feat, nxt, True, batch.x), (where, "a fused kernel serves this shape")
    assert not tr._can_fuse(topo, n_feat, None, False, batch.x), (where, "a fused inference kernel serves this shape")
    if on_device:
        assert tr._plan_for(topo, n_feat, nxt, True, batch.x).family == _lib.STEP_FAMILY_NONE, where
        assert tr._plan_for(topo, n_feat, None, False, batch.x).family == _lib.STEP_FAMILY_NONE, where
    got_regime, fwd, bwd, staged = regime(tr.api, net_name, n_feat, topo, (R, H, O))
    units = tr.api.head_pass_units(R, H, O, batch_cpu.num_graphs)      # hidden units k_head stages at a time for predict()
    assert 0 < units <= H and (units < H) == want_passes, "%s: k_head stages %d of %d hidden units at a time" % (where, units, H)
    if want_regime is not None:
        assert got_regime == want_regime, "%s: regime %s, not %s (k_net LDS need %d / %d bytes forward / backward)" % (
            where, got_regime, want_regime, fwd, bwd)
        assert staged == (want_regime == "i"), (where, got_regime, staged)
    loss = tr.compute_gradients(batch, topo=topo, next_topo=nxt)
    sync(device)
    assert tr.faults() == 0
    first = (float(loss), tr.last_pred.cpu().numpy().copy(), tr.flat_g.cpu().numpy().copy())
    stats = new_stats()
    check_step(where, lazy, first[0], first[1], grads_of(net), ref_loss, ref_pred.numpy(), {k: v.numpy() for k, v in ref_grads.items()},
               stats)
    if mask is None:
        # inference (k_net forward + k_head): the oracle's predictions, and the training launch's (head_graph) under the same
        # rule.  Equal bits are not expected of the two: k_head forms fc1 on the MFMA (one chain over R per element) and fc2
        # from 8 interleaved sums per pass, head_graph forms fc1 from 8 split sums per hidden unit on the VALU -- the same
        # products added in another order, so they agree to rounding, which is what the element-wise rule admits.
        pred = tr.predict(batch, topo=topo).cpu().numpy()
        sync(device)
        check(where + " inference", pred, ref_pred.numpy(), lazy.pred, stats)
        check(where + " inference vs training launch", pred, first[1], lazy.pred, stats)
    else:
        off_pred, _, _ = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, task=task, **fw_of(net_name))
        assert float((off_pred - ref_pred).abs().max()) > 1e-3          # the mask really bit
    if co_build:
        from topo_check import check_against_oracle
        assert nxt.status()[0] == 0
        check_against_oracle(nxt, batch_cpu, weights=need_w)
    loss2 = tr.compute_gradients(batch, topo=topo if nxt is None else nxt)
    sync(device)
    assert tr.faults() == 0
    assert float(loss2) == first[0] or (np.isnan(first[0]) and np.isnan(float(loss2)))
    np.testing.assert_array_equal(tr.last_pred.cpu().numpy(), first[1])
    np.testing.assert_array_equal(tr.flat_g.cpu().numpy(), first[2])
    assert_arbiter_rate(stats, where)
    print("PAIR %-52s regime=%-5s lds=%3d/%3d KiB head %-10s k_head units/pass=%d/%d elements=%-6d arbiter=%d" % (
        where, got_regime, fwd // KIB, bwd // KIB, "staged" if staged else "not staged", units, H, stats["elements"],
        stats["arbiter"]))
    return stats


# ---- a. width sweep ------------------------------------------------------------------------------------------------------
# (net, features, nodes per graph, graphs, regime).  Every net meets every regime at some width; the regime is asserted from
# drgnn_net_lds_bytes at run time.
WIDTHS = (65, 72, 100, 129, 200, 256, 300)
WIDTH_CASES = [("GINet", 65, 120, "i"), ("GINet", 72, 170, "i"), ("GINet", 100, 200, "ii"), ("GINet", 129, 180, "iii"),
               ("GINet", 200, 130, "iii"), ("GINet", 256, 200, "iv"), ("GINet", 300, 90, "iii"),
               ("sGAT", 65, 200, "iii"), ("sGAT", 72, 160, "ii"), ("sGAT", 100, 100, "i"), ("sGAT", 129, 120, "ii"),
               ("sGAT", 200, 200, "iv"), ("sGAT", 256, 120, "iv"), ("sGAT", 300, 70, "iii"),
               ("FoutNet", 65, 190, "ii"), ("FoutNet", 72, 130, "i"), ("FoutNet", 100, 160, "iii"), ("FoutNet", 129, 200, "iv"),
               ("FoutNet", 200, 100, "iii"), ("FoutNet", 256, 80, "iii"), ("FoutNet", 300, 200, "iv")]
assert {(n, r) for n, _, _, r in WIDTH_CASES} == {(n, r) for n in KINDS for r in ("i", "ii", "iii", "iv")}
assert {(n, f) for n, f, _, _ in WIDTH_CASES} == {(n, f) for n in KINDS for f in WIDTHS}
CO_BUILD_CASE = ("GINet", 100, 120, "i")         # the next mini-batch's topology built inside the backward launch


def check_width(net_name, n_feat, n_nodes, want_regime, device, api=None, co_build=False, B=3):
    where = "%s F=%d %dx%d nodes" % (net_name, n_feat, B, n_nodes)
    return check_pair_step(net_name, syn_batch(n_feat, n_nodes, B), device, api, want_regime=want_regime, co_build=co_build, where=where)


def check_ragged(net_name, n_feat, device, api=None):
    return check_pair_step(net_name, ragged(n_feat), device, api, where="%s F=%d ragged" % (net_name, n_feat))


# ---- b. three Adam steps ---------------------------------------------------------------------------------------------------
def check_three_adam_steps(net_name, device, api=None, n_feat=100, n_nodes=120, B=5):
    """train_step with ping-ponged topologies against torch.optim.Adam on the oracle (the tolerances of
    test_fused_step_syn64_three_adam_steps_match_oracle): train_update on slabs of a wide conv1."""
    on_device = api is None
    kw = {} if on_device else {"api": api}
    batch_cpu = syn_batch(n_feat, n_nodes, B)
    params = make_params(net_name, n_feat, seed=12)
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(leaves.values()), lr=0.01)
    net = build_net(net_name, params, device)
    tr = FusedTrainer(net, lr=0.01, task="reg", **kw)
    if not on_device:
        tr.fused_step = False
    batch = batch_cpu.clone().to(device)
    need_w = net_name == "sGAT"
    topos = [Topology.from_batch(batch, need_weights=need_w, **kw), Topology.from_batch(batch, need_weights=need_w, **kw)]
    assert not tr._can_fuse(topos[0], n_feat, topos[1], True, batch.x)
    if on_device:
        assert tr._plan_for(topos[0], n_feat, topos[1], True, batch.x).family == _lib.STEP_FAMILY_NONE
    for it in range(3):
        opt.zero_grad()
        pred = cpu_ref.FORWARD[net_name](leaves, batch_cpu, **fw_of(net_name))
        loss = F.mse_loss(pred.reshape(-1), batch_cpu.y)
        loss.backward()
        opt.step()
        got = tr.train_step(batch, topo=topos[it & 1], next_topo=topos[1 - (it & 1)])
        sync(device)
        np.testing.assert_allclose(float(got), float(loss.detach()), rtol=1e-4)
        np.testing.assert_allclose(tr.last_pred.cpu().numpy(), pred.detach().numpy(), rtol=1e-4, atol=1e-4)
    assert tr.faults() == 0 and int(tr.step) == 3
    sd = net.state_dict()
    for k, v in leaves.items():
        np.testing.assert_allclose(sd[k].cpu().numpy(), v.detach().numpy(), rtol=1e-4, atol=1e-4, err_msg=k)


# ---- c. heads --------------------------------------------------------------------------------------------------------------
HEADS = (("GINet", 16), ("FoutNet", 96), ("sGAT", 128), ("GINet", 129), ("sGAT", 147), ("FoutNet", 200), ("GINet", 257), ("sGAT", 512),
         ("GINet", 512))
# GINet's readout is 64 wide (sGAT's and FoutNet's 32): its 512-unit head is the one k_head cannot stage whole even for 16
# graphs per workgroup, so predict() takes it in passes (416 + 96 units at one output, 400 + 112 at three)
HEADS_IN_PASSES = {("GINet", 512)}


def check_head(net_name, H, O, n_feat, device, api=None, dropout=None):
    """A head of H hidden units, O outputs (O = 3: classification with class weights).  At 32 features the head alone sends the
    launch to the pair."""
    task = "reg" if O == 1 else "class"
    batch_cpu = syn_batch(n_feat, 90, 5)
    params = make_params(net_name, n_feat, H, O)
    where = "%s head H=%d O=%d F=%d%s" % (net_name, H, O, n_feat, "" if dropout is None else " dropout %.1f" % dropout)
    return check_pair_step(net_name, batch_cpu, device, api, params=params, task=task, dropout=dropout,
                           want_passes=(net_name, H) in HEADS_IN_PASSES, where=where)


def check_head_too_wide(device, api=None):
    """H = 513: the trainer raises DrgnnError before anything is launched (parameters, gradient buffer and step counter keep
    what they held), and the library's own entry point of the backward launch returns DRGNN_E_WIDTH (-3, "unsupported width")
    with its outputs untouched."""
    import pytest
    from deeprank_gnn_amd.functional import H1, H2, _describe
    kw = {} if api is None else {"api": api}
    batch_cpu = syn_batch(32, 90, 5)
    params = make_params("sGAT", 32, 513, 1)
    net = build_net("sGAT", params, device)
    tr = FusedTrainer(net, lr=0.01, task="reg", **kw)
    batch = batch_cpu.clone().to(device)
    topo = Topology.from_batch(batch, need_weights=True, **kw)
    assert not tr._can_fuse(topo, 32, None, True, batch.x)
    before = tr.flat_p.clone()
    tr.flat_g.fill_(7.0)
    with pytest.raises(_lib.DrgnnError, match="unsupported width"):
        tr.train_step(batch, topo=topo)
    sync(device)
    assert torch.equal(tr.flat_p, before) and bool((tr.flat_g == 7.0).all()) and int(tr.step) == 0
    # the library itself: the backward entry point with valid buffers of a 513-unit head
    B, n_nodes = topo.n_graphs, batch.x.shape[0]
    new = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=device)
    xp, arg0, arg1 = new((1, n_nodes, H1)), new((1, n_nodes, H1), torch.int32), new((1, n_nodes, H2), torch.int32)
    readout, pred = new((B, H2)), torch.full((B, 1), 7.0, device=device)
    hp = torch.full((B, tr.api.head_partial_elems(tr.R, tr.H, tr.O)), 7.0, device=device)
    partials = torch.full((B, tr.api.net_partial_elems(tr.kind, 32)), 7.0, device=device)
    scratch = new(tr.api.net_scratch_elems(tr.kind, 32, n_nodes, topo.n_edges, B))
    desc = _describe(tr.kind, 32, tr.live, 1)
    with pytest.raises(_lib.DrgnnError, match="unsupported width"):
        tr.api.net_backward_fused_head(desc, tr._head_desc(True), batch.x, readout, batch.y, tr.step, topo.ws_i32, topo.ws_f32,
                                       n_nodes, topo.n_edges, B, topo.max_nodes, topo.max_edges, topo.max_c0, xp, arg0, arg1,
                                       pred, hp, None, partials, scratch, _lib.current_stream(batch.x))
    sync(device)
    assert bool((pred == 7.0).all()) and bool((hp == 7.0).all()) and bool((partials == 7.0).all())
    assert tr.faults() == 0


# (graphs, R, H, O, inference in passes).  More than 512 graphs: 64 per workgroup.
#   520, 32, 64, 12   fc2's 8 split sums per graph and output need 8 * 64 * O floats of LDS, more than the K-split area used to hold
#   530, 64, 300, 3   too wide to stage whole beside 64 graphs: passes of 224 + 76 units (a tail that is no multiple of the MFMA tile)
#   530, 32, 300, 12  both at once, passes of 272 + 28
#    20, 64, 500, 1   16 graphs per workgroup, passes of 416 + 84
HEAD_STEP_CASES = [(520, 32, 64, 12, False), (530, 64, 300, 3, True), (530, 32, 300, 12, True), (20, 64, 500, 1, True)]


def check_head_step(device, api=None, B=520, R=32, H=64, O=12, passes=False):
    """k_head called by itself (drgnn_head_step) against torch in float64, element-wise: inference, and the training launch
    where the head fits LDS whole -- a training launch takes no passes, so where inference needs them (asserted from
    drgnn_head_pass_units) it must refuse with DRGNN_E_WIDTH and leave its outputs alone."""
    import pytest
    from deeprank_gnn_amd.launch import head_desc
    api = api or _lib.get()
    units = api.head_pass_units(R, H, O, B)
    assert 0 < units <= H and (units < H) == passes, (units, H)
    gen = torch.Generator().manual_seed(5)
    lin1, lin2 = torch.nn.Linear(R, H), torch.nn.Linear(H, O)
    net = torch.nn.Module()
    net.fc1, net.fc2 = lin1, lin2
    net = net.to(device)
    readout = torch.randn((B, R), generator=gen)
    y = torch.randint(0, O, (B,), generator=gen)
    p64 = [t.detach().cpu().double() for t in (lin1.weight, lin1.bias, lin2.weight, lin2.bias)]
    x64 = readout.double().requires_grad_(True)
    ref = F.linear(F.relu(F.linear(x64, p64[0], p64[1])), p64[2], p64[3])
    F.cross_entropy(ref, y).backward()
    rd, yd = readout.to(device), y.to(device)
    step = torch.zeros(1, dtype=torch.int32, device=device)
    stream = _lib.current_stream(rd)
    pred = torch.full((B, O), 7.0, device=device)
    api.head_step(head_desc(net, _lib.TASK_CLASS, False, 0.0, 1), rd, None, B, step, pred, None, None, stream)
    sync(device)
    stats = new_stats()
    where = "k_head %d graphs R=%d H=%d O=%d" % (B, R, H, O)
    check(where + " inference", pred.cpu().numpy(), ref.detach().float().numpy(), lambda: ref.detach().numpy(), stats)
    pred2 = torch.full((B, O), 7.0, device=device)
    gr = torch.full((B, R), 7.0, device=device)
    partials = torch.full((api.head_num_slabs(B), api.head_partial_elems(R, H, O)), 7.0, device=device)
    train = head_desc(net, _lib.TASK_CLASS, True, 0.0, 1)
    if passes:
        with pytest.raises(_lib.DrgnnError, match="unsupported width"):
            api.head_step(train, rd, yd, B, step, pred2, gr, partials, stream)
        sync(device)
        assert bool((pred2 == 7.0).all()) and bool((gr == 7.0).all()) and bool((partials == 7.0).all())
    else:
        api.head_step(train, rd, yd, B, step, pred2, gr, partials, stream)
        sync(device)
        assert torch.equal(pred2, pred)
        check(where + " d readout", gr.cpu().numpy(), x64.grad.float().numpy(), lambda: x64.grad.numpy(), stats)
    assert_arbiter_rate(stats, where)
    print("PAIR %-52s k_head units/pass=%d/%d elements=%-6d arbiter=%d" % (where, units, H, stats["elements"], stats["arbiter"]))


# ---- d. drop-in boundary ---------------------------------------------------------------------------------------------------
def check_dropin_wide(net_name, device, api=None, n_feat=100):
    """``model(batch)`` beyond 64 features: outside the fused kernels (the reason names the feature count), the launch pair's
    body + torch's head, loss.backward(): the oracle's numbers."""
    from deeprank_gnn_amd.fused_autograd import engine_for
    kw = {} if api is None else {"api": api}
    batch_cpu = syn_batch(n_feat, 120, 5)
    params = make_params(net_name, n_feat)
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, **fw_of(net_name))
    lazy = Lazy64(net_name, params, batch_cpu, **fw_of(net_name))
    net = build_net(net_name, params, device)
    net.train()
    batch = batch_cpu.clone().to(device)
    topo = Topology.from_batch(batch, need_weights=(net_name == "sGAT"), **kw)
    out = net(batch, topo=topo)
    eng = engine_for(net)
    assert eng.last_path is None and eng.last_reason
    if api is None:
        assert "%d features" % n_feat in eng.last_reason, eng.last_reason
    loss = F.mse_loss(out.reshape(-1), batch.y)
    loss.backward()
    sync(device)
    where = "%s model(batch) F=%d" % (net_name, n_feat)
    stats = check_step(where, lazy, float(loss.detach()), out.detach().cpu().numpy(), grads_of(net), ref_loss, ref_pred.numpy(),
                       {k: v.numpy() for k, v in ref_grads.items()})
    print("PAIR %-52s elements=%-6d arbiter=%d" % (where, stats["elements"], stats["arbiter"]))


def _oracle_grad_x(net_name, params, batch_cpu, double):
    b = batch_cpu.clone()
    p = params
    if double:
        p = {k: v.double() for k, v in params.items()}
        for key in ("x", "edge_attr", "pos", "y", "internal_edge_attr"):
            v = getattr(b, key, None)
            if torch.is_tensor(v) and v.is_floating_point():
                setattr(b, key, v.double())
    x = b.x.clone().requires_grad_(True)
    b.x = x
    pred = cpu_ref.FORWARD[net_name](p, b, **fw_of(net_name))
    F.mse_loss(pred.reshape(-1), b.y).backward()
    return pred.detach().numpy(), x.grad.numpy()


def check_grad_x(net_name, n_feat, device, api=None):
    """``batch.x.requires_grad_(True)``: always the launch pair (the dX GEMM, written back through the xs tile with stride
    F + 1); x.grad against the oracle's autograd with respect to x."""
    from deeprank_gnn_amd.fused_autograd import engine_for
    kw = {} if api is None else {"api": api}
    batch_cpu = syn_batch(n_feat, 120, 4)
    params = make_params(net_name, n_feat, seed=43)
    ref_pred, ref_gx = _oracle_grad_x(net_name, params, batch_cpu, False)
    net = build_net(net_name, params, device)
    net.train()
    batch = batch_cpu.clone().to(device)
    topo = Topology.from_batch(batch, need_weights=(net_name == "sGAT"), **kw)
    batch.x.requires_grad_(True)
    out = net(batch, topo=topo)
    eng = engine_for(net)
    assert eng.last_path is None and eng.last_reason
    if api is None:
        assert "without gradient" in eng.last_reason, eng.last_reason
    F.mse_loss(out.reshape(-1), batch.y).backward()
    sync(device)
    stats = new_stats()
    where = "%s x.grad F=%d" % (net_name, n_feat)
    r64 = []

    def ref64(i):
        if not r64:
            r64.append(_oracle_grad_x(net_name, params, batch_cpu, True))
        return r64[0][i]
    check(where + " pred", out.detach().cpu().numpy().reshape(-1), ref_pred.reshape(-1), lambda: ref64(0).reshape(-1), stats)
    check(where, batch.x.grad.cpu().numpy(), ref_gx, lambda: ref64(1), stats)
    assert float(np.abs(ref_gx).max()) > 0.0
    assert_arbiter_rate(stats, where)
    print("PAIR %-52s elements=%-6d arbiter=%d" % (where, stats["elements"], stats["arbiter"]))


# ---- e. resident set with 72 features ------------------------------------------------------------------------------------
def check_resident_set(net_name, device, api=None, n_feat=72, n_nodes=60, n_graphs=8, batch_size=4, big=None):
    """A resident set beyond 64 features.  The native epoch loop either leaves the epoch to the per-batch path (None; then the
    cached single step refuses too, and the per-batch steps run) or gives the bits of stepping the same mini-batches one by
    one.  The set's topology cache has aggregation tiles exactly when the builder forms them for the set's largest graph
    (drgnn_topology_tiles_ok: up to 256 features where an x tile fits its LDS); ``big``: one graph of that many nodes, beyond
    what the builder forms tiles for -- at 64 features or fewer resident.TopologyCache then forms them in a launch of their
    own, beyond 64 features the cache stays without tiles."""
    import copy
    import pytest
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd.resident import ResidentGraphSet
    kw = {} if api is None else {"api": api}
    graphs = list(_graphs(n_feat, n_nodes, n_graphs))
    if big is not None:
        graphs[-1] = synth.make_graph(n_graphs - 1, n_feat=n_feat, **shape_of(big))
    rs = ResidentGraphSet(graphs, device, **kw)
    need_w = net_name == "sGAT"
    cache = rs.topology_cache(need_weights=need_w)
    tiles = rs.api.topology_tiles_ok(cache.max_nodes, cache.max_edges, n_feat)
    assert tiles == (big is None), "%d nodes, %d edges" % (cache.max_nodes, cache.max_edges)
    assert (cache.topo.tiles is not None) == tiles and bool(cache.topo.flags & _lib.TOPO_TILES) == tiles
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    for cached in (False, True):
        net = build_net(net_name, make_params(net_name, n_feat, seed=9), device)
        tr_a = FusedTrainer(net, lr=0.01, task="reg", seed=7, **kw)
        tr_b = FusedTrainer(copy.deepcopy(net), lr=0.01, task="reg", seed=7, **kw)
        done = tr_a.train_epoch(rs, order, batch_size, cached=cached)
        sync(device)
        if api is None:
            assert done is None, "no fused kernel takes %d features: the epoch is the per-batch path's" % n_feat
        if done is None:
            assert int(tr_a.step) == 0
            if cached:
                with pytest.raises(_lib.DrgnnError):
                    tr_a.train_step_cached(cache, order[:batch_size])
            else:
                for lo in range(0, len(order), batch_size):
                    loss = tr_a.train_step(Batch.from_data_list([graphs[i] for i in order[lo:lo + batch_size]]).to(device))
                    assert np.isfinite(float(loss))
                assert int(tr_a.step) == len(order) // batch_size and tr_a.faults() == 0
            continue
        losses, pred = done
        want_l, want_p = [], []
        cache = rs.topology_cache(need_weights=need_w) if cached else None
        for lo in range(0, len(order), batch_size):
            ids = order[lo:lo + batch_size]
            if cached:
                want_l.append(float(tr_b.train_step_cached(cache, ids)))
            else:
                want_l.append(float(tr_b.train_step(Batch.from_data_list([graphs[i] for i in ids]).to(device))))
            want_p.append(tr_b.last_pred.detach().cpu().clone())
        assert losses.cpu().tolist() == want_l
        assert torch.equal(pred.cpu(), torch.cat(want_p))
        assert torch.equal(tr_a.flat_p.cpu(), tr_b.flat_p.cpu())


def check_neuralnet_wide(net_name, tmp_path, device=None, api=None, n_feat=72):
    """NeuralNet.train for two epochs over a graph file of 72 features == the per-batch loop's losses (each mini-batch from the
    resident set, its own topology build, train_step), bit for bit: the epoch loss is the float32 sum of the mini-batch losses
    in visiting order, formed here the way NeuralNet._epoch forms it."""
    import os
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd.NeuralNet import NeuralNet
    db = synth.save_store(os.path.join(str(tmp_path), "wide.npz"), 8, n_feat=n_feat, **shape_of(60))
    kw = dict(node_feature=["feat"], edge_feature=["dist"], target="irmsd", batch_size=3, percent=[1.0, 0.0], shuffle=False,
              outdir=str(tmp_path))
    if api is not None:
        kw.update(_api=api, device="cpu")
    runs = []
    for loop in ("train", "per batch"):
        torch.manual_seed(0)
        np.random.seed(0)
        nn = NeuralNet(db, nets()[net_name], **kw)
        if hasattr(nn.model, "dropout"):
            nn.model.dropout = 0.0
        assert nn.trainer.layout is not None and int(nn._resident(nn.dataset).n_feat) == n_feat
        if loop == "train":
            nn.train(nepoch=2, validate=False, save_model=None, hdf5=None)
            runs.append([float(v) for v in nn.train_loss])
        else:
            total = []
            for _ in range(2):
                run = torch.zeros((), dtype=torch.float32)
                for batch in nn._batches(nn.dataset, nn.train_index, False):
                    run += nn.trainer.train_step(batch).detach().reshape(()).cpu()
                total.append(float(run))
            runs.append(total)
        assert nn.trainer.faults() == 0
    assert np.isfinite(runs[0]).all() and runs[0][1] < runs[0][0]
    assert runs[0] == runs[1], (runs[0], runs[1])
