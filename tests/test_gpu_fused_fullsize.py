"""The BENCHMARKED kernel instance against the oracle at the BENCHMARKED shape.

bench.py times ``k_step3_co_topo`` / ``k_step2_co_topo`` at width 32 (the width-specialised fused training step, launched
through ``FusedTrainer.compute_gradients`` / ``train_step`` with the next batch's topology co-built by
the same launch) on ``synthetic.make_batch(0, 64)`` = BASELINE.json configs[1..3].  These tests run
exactly that launch on exactly that batch and compare predictions, loss and EVERY gradient with
``oracle/cpu_ref.py`` element by element:  |got - ref| <= 1e-4 + 1e-4 |ref|  (north_star: 1e-4 fp32),
no scaling by the tensor's maximum.  Reference path: ginet.py:99-141, sGAT.py:114-138,
foutnet.py:103-125 + MSELoss + loss.backward() + Adam (NeuralNet.py:489-506).

fp32 caveat, stated rather than hidden: a gradient element is a sum of ~10^4 products; the oracle
(torch CPU fp32) and the kernel associate that sum differently.  Where an element is a cancellation
residue the two fp32 results may differ by more than 1e-4 of the ELEMENT while both sit within fp32
round-off of the exact value.  For any element that misses the strict test we therefore evaluate the
oracle in float64 as the arbiter and require the kernel to be at least as close to the float64 value as
1e-4 + 1e-4|ref| OR as close as the fp32 oracle itself is (x4): never looser than what fp32 arithmetic
of the reference can resolve (tests/elementwise.py).  The number of elements needing the arbiter is ASSERTED to stay
below 0.1 %.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from elementwise import Lazy64, check_step, new_stats, assert_arbiter_rate

pytestmark = pytest.mark.gpu
TOL = 1e-4
NETS = ["GINet", "sGAT", "FoutNet"]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _fw_kwargs(net_name):
    return {"looped": False} if net_name == "FoutNet" else {}


def _grads_of(net):
    return {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}


def _trainer(net_name, params, lr=0.01):
    from test_gpu_parity import build
    from deeprank_gnn_amd.trainer import FusedTrainer
    net = build(net_name, params, 1)                      # dropout forced to 0 for parity
    return net, FusedTrainer(net, lr=lr, task="reg")


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("net_name", NETS)
def test_fused_step_syn64_gradients_match_oracle_elementwise(net_name, pipelined):
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.topology import Topology
    dev = _dev()
    batch_cpu = synth.make_batch(0, 64)
    params = cpu_ref.init_params(net_name, 32, 1, 1, seed=11)
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y,
                                                           **_fw_kwargs(net_name))
    lazy = Lazy64(net_name, params, batch_cpu, **_fw_kwargs(net_name))
    net, tr = _trainer(net_name, params)
    batch = batch_cpu.clone().to(dev)
    need_w = net_name == "sGAT"
    topo = Topology.from_batch(batch, need_weights=need_w)
    # the launch bench.py times: the width-specialised fused kernel (F16 = 32) ...
    assert tr._can_fuse(topo, 32), "SYN64 must take the fused-step path"
    assert tr.api.step_is_specialised(tr.kind, batch.x, 32, topo.max_nodes, topo.max_edges, topo.max_c0,
                                      tr.H, tr.O), "SYN64 must take the width-specialised instantiation"
    nxt = Topology.from_batch(batch, need_weights=need_w, build=False) if pipelined else None
    loss = tr.compute_gradients(batch, topo=topo, next_topo=nxt)
    torch.cuda.synchronize()
    stats = new_stats()
    check_step("%s SYN64" % net_name, lazy, loss, tr.last_pred.cpu().numpy(), _grads_of(net), ref_loss, ref_pred.numpy(),
               {k: v.numpy() for k, v in ref_grads.items()}, stats)
    # the escape clause is bounded: at most 0.1 % of the elements may need the float64 arbiter (round 2: none did)
    assert_arbiter_rate(stats, "%s pipelined=%s" % (net_name, pipelined))
    if pipelined:
        # ... and the topology the same launch built for the NEXT step is the one a plain build gives
        from topo_check import check_against_oracle
        assert nxt.status()[0] == 0
        check_against_oracle(nxt, batch_cpu, weights=need_w)
        loss2 = tr.compute_gradients(batch, topo=nxt)
        assert float(loss2) == float(loss)


@pytest.mark.parametrize("net_name", NETS)
def test_fused_step_syn128_gradients_match_oracle_elementwise(net_name):
    """The reference's shipped training batch size (128 graphs) in the launches it takes by itself: beyond the
    resident workgroup count GINet runs both branches of a graph in ONE workgroup from the aggregation tiles
    (k_step3b_co_topo, drgnn_step3.h: net_step3_graph_both), sGAT / FoutNet one workgroup per graph (k_step2_co_topo<.., 1>),
    and the co-launched builder one workgroup per graph (rows chain, then clusters chain).  Element-wise against the oracle,
    and the topology that launch built for the next step is the one a plain build gives."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd.topology import Topology
    from topo_check import check_against_oracle
    dev = _dev()
    batch_cpu = synth.make_batch(0, 128)
    params = cpu_ref.init_params(net_name, 32, 1, 1, seed=13)
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, **_fw_kwargs(net_name))
    lazy = Lazy64(net_name, params, batch_cpu, **_fw_kwargs(net_name))
    net, tr = _trainer(net_name, params)
    batch = batch_cpu.clone().to(dev)
    need_w = net_name == "sGAT"
    topo = Topology.from_batch(batch, need_weights=need_w)
    assert tr._can_fuse(topo, 32)
    nxt = Topology.from_batch(batch, need_weights=need_w, build=False)
    loss = tr.compute_gradients(batch, topo=topo, next_topo=nxt)
    torch.cuda.synchronize()
    stats = new_stats()
    check_step("%s SYN128" % net_name, lazy, loss, tr.last_pred.cpu().numpy(), _grads_of(net), ref_loss, ref_pred.numpy(),
               {k: v.numpy() for k, v in ref_grads.items()}, stats)
    assert_arbiter_rate(stats, "%s batch 128" % net_name)
    assert nxt.status()[0] == 0
    check_against_oracle(nxt, batch_cpu, weights=need_w)
    loss2 = tr.compute_gradients(batch, topo=nxt)          # (the co-built, lean workspace under the same kind of launch)
    assert float(loss2) == float(loss)
    tr.check_faults()


@pytest.mark.parametrize("layout", ["two", "one"])
def test_fused_step_syn64_dropout_on_matches_oracle_elementwise(layout):
    """The launch bench.py times runs GINet with dropout = 0.4 (ginet.py:97,138); the product's Bernoulli draw is a counter
    hash, not torch's Philox, so the dropout-on code path is compared through an EXPLICIT mask: the kernels take a [B, 128]
    0 / 1 mask (drgnn_head_desc.drop_mask) instead of the hash decision, the oracle applies F.dropout's arithmetic
    hid * mask / (1 - p) with the same mask.  Everything else is the benchmarked launch (k_step3_co_topo at width 32, p_drop =
    0.4, keep_scale = 1 / 0.6 in the forward and in d hid).  Both GINet layouts (two branch workgroups / one per graph)."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.topology import Topology
    dev = _dev()
    batch_cpu = synth.make_batch(0, 64)
    params = cpu_ref.init_params("GINet", 32, 1, 1, seed=21)
    gen = torch.Generator().manual_seed(77)
    mask = (torch.rand((64, 128), generator=gen) >= 0.4).float()          # keep-rate 0.6, seeded
    assert 0.5 < float(mask.mean()) < 0.7
    fw = dict(dropout=0.4, drop_mask=mask)
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads("GINet", params, batch_cpu, batch_cpu.y, **fw)
    lazy = Lazy64("GINet", params, batch_cpu, dropout=0.4, drop_mask=mask.double())
    net, tr = _trainer("GINet", params)
    net.dropout = 0.4
    tr.drop_mask = mask.to(dev).contiguous()
    batch = batch_cpu.clone().to(dev)
    topo = Topology.from_batch(batch, need_weights=False)
    assert tr._can_fuse(topo, 32)
    tr.plan_overrides = {"force_wgs": 1} if layout == "one" else {}
    nxt = Topology.from_batch(batch, need_weights=False, build=False)
    loss = tr.compute_gradients(batch, topo=topo, next_topo=nxt)
    torch.cuda.synchronize()
    # the mask really bit: the dropout-off prediction differs
    off_pred, _, _ = cpu_ref.loss_and_grads("GINet", params, batch_cpu, batch_cpu.y)
    assert float((off_pred - ref_pred).abs().max()) > 1e-3
    stats = new_stats()
    check_step("GINet SYN64 dropout 0.4 (%s)" % layout, lazy, loss, tr.last_pred.cpu().numpy(), _grads_of(net), ref_loss,
               ref_pred.numpy(), {k: v.numpy() for k, v in ref_grads.items()}, stats)
    assert_arbiter_rate(stats, "GINet dropout on, layout %s" % layout)
    tr.check_faults()


@pytest.mark.parametrize("net_name", NETS)
def test_fused_step_syn64_three_adam_steps_match_oracle(net_name):
    """Three optimiser steps through the benchmarked launches (k_step3_co_topo + k_update, topologies
    ping-ponging as in bench.py) vs the oracle trained with torch.optim.Adam."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd.topology import Topology
    dev = _dev()
    batch_cpu = synth.make_batch(0, 64)
    params = cpu_ref.init_params(net_name, 32, 1, 1, seed=12)
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(leaves.values()), lr=0.01)
    net, tr = _trainer(net_name, params, lr=0.01)
    batch = batch_cpu.clone().to(dev)
    need_w = net_name == "sGAT"
    topos = [Topology.from_batch(batch, need_weights=need_w), Topology.from_batch(batch, need_weights=need_w)]
    kw = _fw_kwargs(net_name)
    for it in range(3):
        opt.zero_grad()
        pred = cpu_ref.FORWARD[net_name](leaves, batch_cpu, **kw)
        loss = F.mse_loss(pred.reshape(-1), batch_cpu.y)
        loss.backward()
        opt.step()
        got = tr.train_step(batch, topo=topos[it & 1], next_topo=topos[1 - (it & 1)])
        np.testing.assert_allclose(float(got), float(loss.detach()), rtol=TOL)
        np.testing.assert_allclose(tr.last_pred.cpu().numpy(), pred.detach().numpy(), rtol=TOL, atol=TOL)
    sd = net.state_dict()
    for k, v in leaves.items():
        # Adam's first steps move every weight by ~lr regardless of the gradient's size: the parameters
        # agree to 1e-4 element-wise wherever the gradient is resolved by fp32 (all but exact zeros)
        np.testing.assert_allclose(sd[k].cpu().numpy(), v.detach().numpy(), rtol=TOL, atol=TOL, err_msg=k)


@pytest.mark.parametrize("net_name,n_graphs", [("GINet", 80), ("GINet", 96), ("sGAT", 80), ("sGAT", 128), ("FoutNet", 200), ("GINet", 200)])
def test_fused_step_batches_beyond_the_argument_table(net_name, n_graphs):
    """More than 64 graphs: the per-graph offsets no longer travel in the kernel arguments (workspace tables instead), and
    beyond 160 graphs the topology builder runs one workgroup per graph -- same numbers as the oracle either way."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd.topology import Topology
    dev = _dev()
    batch_cpu = synth.make_batch(0, n_graphs, n_nodes=48, n_pairs=90, n_c1=4, n_internal=20)
    params = cpu_ref.init_params(net_name, 32, 1, 1, seed=3)
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, **_fw_kwargs(net_name))
    net, tr = _trainer(net_name, params)
    batch = batch_cpu.clone().to(dev)
    need_w = net_name == "sGAT"
    topo = Topology.from_batch(batch, need_weights=need_w)
    nxt = Topology.from_batch(batch, need_weights=need_w, build=False)
    assert tr._can_fuse(topo, 32)
    # beyond the resident size (2 B + builder workgroups > CUs) a GINet graph is ONE workgroup running both branches: no
    # workgroup ever waits for another one, whatever the dispatch order
    wgs, _ = tr.api.net_step_plan(tr.kind, 32, topo.max_nodes, topo.max_edges, topo.max_c0, tr.R, tr.H, tr.O, n_graphs, n_graphs)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # two workgroups per graph ONLY if they and the co-launched builder (then one workgroup per graph) are all resident:
    # GINet's branch workgroups, and the half-graph workgroups of the node-split layout of sGAT / FoutNet (drgnn_step2.h)
    assert wgs == (2 if 2 * n_graphs + n_graphs <= cus else 1), (wgs, n_graphs, cus)
    loss = tr.compute_gradients(batch, topo=topo, next_topo=nxt)
    torch.cuda.synchronize()
    assert tr.faults() == 0
    check_step(net_name, Lazy64(net_name, params, batch_cpu, **_fw_kwargs(net_name)), loss, tr.last_pred.cpu().numpy(),
               _grads_of(net), ref_loss, ref_pred.numpy(), {k: v.numpy() for k, v in ref_grads.items()})
    from topo_check import check_against_oracle
    check_against_oracle(nxt, batch_cpu, weights=need_w)
    assert float(tr.compute_gradients(batch, topo=nxt)) == float(loss)


def test_ginet_one_workgroup_step_at_syn_size_matches_oracle_and_two_workgroup_step():
    """BASELINE-shaped graphs (200 nodes, ~1000 edges, 32 features), 130 of them: past the resident size, so the launch
    is one workgroup per graph (both branches in sequence: drgnn_step3.h's net_step3_graph_both, from the aggregation tiles).  Element-wise against the oracle; the first 64
    graphs' predictions equal what the two-workgroup layout gives on them alone (same arithmetic per branch)."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.topology import Topology
    dev = _dev()
    n_graphs = 130
    batch_cpu = synth.make_batch(0, n_graphs)
    params = cpu_ref.init_params("GINet", 32, 1, 1, seed=21)
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads("GINet", params, batch_cpu, batch_cpu.y)
    net, tr = _trainer("GINet", params)
    batch = batch_cpu.clone().to(dev)
    topo = Topology.from_batch(batch, need_weights=False)
    assert tr._can_fuse(topo, 32)
    assert tr.api.net_step_plan(tr.kind, 32, topo.max_nodes, topo.max_edges, topo.max_c0, tr.R, tr.H, tr.O, n_graphs)[0] == 1
    assert tr.api.step_is_specialised(tr.kind, batch.x, 32, topo.max_nodes, topo.max_edges, topo.max_c0, tr.H, tr.O)
    loss = tr.compute_gradients(batch, topo=topo)
    torch.cuda.synchronize()
    assert tr.faults() == 0
    check_step("GINet one workgroup per graph", Lazy64("GINet", params, batch_cpu), loss, tr.last_pred.cpu().numpy(),
               _grads_of(net), ref_loss, ref_pred.numpy(), {k: v.numpy() for k, v in ref_grads.items()})
    pred_one = tr.last_pred[:64].cpu().numpy().copy()
    small = synth.make_batch(0, 64).to(dev)
    t64 = Topology.from_batch(small, need_weights=False)
    assert tr.api.net_step_plan(tr.kind, 32, t64.max_nodes, t64.max_edges, t64.max_c0, tr.R, tr.H, tr.O, 64)[0] == 2
    tr.compute_gradients(small, topo=t64)                  # (no update in between: same parameters)
    pred_af = tr.last_pred.cpu().numpy().copy()            # the two-workgroup kernel of the same family (drgnn_step3.h)
    np.testing.assert_array_equal(pred_one, pred_af)       # forward arithmetic is the same code in both layouts
    tr.plan_overrides = {"no_aggregate": 1}                # ... and the launch pair (family NONE: drgnn_net.h): same numbers to rounding
    assert tr._plan_for(t64, 32).family == _lib.STEP_FAMILY_NONE
    tr.compute_gradients(small, topo=t64)
    pred_two = tr.last_pred.cpu().numpy()
    tr.plan_overrides = {}
    np.testing.assert_allclose(pred_one, pred_two, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("cached", [True, False])
@pytest.mark.parametrize("n_feat,task", [(32, "reg"), (5, "class"), (40, "reg"), (16, "reg")])
def test_ginet_one_workgroup_layout_matches_two_workgroup_layout(n_feat, task, cached):
    """cached: the one-workgroup launches read the batch's graphs out of a resident set's topology cache, in reversed order"""
    from step_check import check_one_workgroup_layout
    check_one_workgroup_layout(n_feat, task, "cuda:0", seed=3 + n_feat, cached=cached)


@pytest.mark.parametrize("net_name,n_nodes,n_pairs", [("GINet", 272, 320), ("FoutNet", 264, 300)])
def test_fused_step_offset_tables_longer_than_one_staging_pass(net_name, n_nodes, n_pairs):
    """More than 255 nodes: the per-wave staging jobs of the offset tables (N + 1 words) take a second 128-bit pass, the
    member lists too -- still the width-specialised fused kernel (8 features -> the 16-wide instantiation), same numbers as
    the oracle."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd.topology import Topology
    dev = _dev()
    batch_cpu = synth.make_batch(0, 12, n_nodes=n_nodes, n_pairs=n_pairs, n_feat=8, n_c1=6, n_internal=300)
    params = cpu_ref.init_params(net_name, 8, 1, 1, seed=4)
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, **_fw_kwargs(net_name))
    from test_gpu_parity import build
    from deeprank_gnn_amd.trainer import FusedTrainer
    net = build(net_name, params, 1)                      # (feature width taken from the parameters)
    tr = FusedTrainer(net, lr=0.01, task="reg")
    batch = batch_cpu.clone().to(dev)
    topo = Topology.from_batch(batch, need_weights=False)
    assert topo.max_nodes > 255
    assert tr._can_fuse(topo, 8), "this shape must take the fused-step path"
    assert tr.api.step_is_specialised(tr.kind, batch.x, 8, topo.max_nodes, topo.max_edges, topo.max_c0, tr.H, tr.O)
    loss = tr.compute_gradients(batch, topo=topo)
    torch.cuda.synchronize()
    check_step(net_name, Lazy64(net_name, params, batch_cpu, **_fw_kwargs(net_name)), loss, tr.last_pred.cpu().numpy(),
               _grads_of(net), ref_loss, ref_pred.numpy(), {k: v.numpy() for k, v in ref_grads.items()})


@pytest.mark.parametrize("net_name", NETS)
def test_fused_step_random_shapes_match_oracle(net_name):
    """A seeded sweep of mini-batches whose graphs differ in size inside the batch (4 .. 230 nodes, sparse to dense
    contacts, 4 .. 64 features, few to many clusters): loss, predictions and every gradient of the fused step vs the
    oracle.  Exercises the per-wave staging jobs at every array length, odd feature widths (generic kernel) and the
    width-specialised instantiations alike."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd.data import Batch
    from deeprank_gnn_amd.topology import Topology
    from deeprank_gnn_amd.trainer import FusedTrainer
    from test_gpu_parity import build
    dev = _dev()
    rng = np.random.default_rng(20260928)
    ran = 0
    sweep_stats = new_stats()
    for case in range(10):
        n_feat = int(rng.choice([4, 7, 16, 20, 32, 48, 64]))
        n_graphs = int(rng.integers(1, 9))
        graphs = []
        for k in range(n_graphs):
            n_nodes = int(rng.integers(4, 231))
            half = n_nodes // 2
            n_pairs = int(rng.integers(1, max(2, min(4 * n_nodes, half * (n_nodes - half)))))
            n_int = int(rng.integers(1, max(2, min(3 * n_nodes, half * (half - 1) // 2 + 1))))
            graphs.append(synth.make_graph(1000 * case + k, n_nodes=n_nodes, n_pairs=n_pairs, n_feat=n_feat,
                                           n_c1=int(rng.integers(1, 12)), n_internal=n_int))
        batch_cpu = Batch.from_data_list(graphs)
        params = cpu_ref.init_params(net_name, n_feat, 1, 1, seed=100 + case)
        ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, **_fw_kwargs(net_name))
        net = build(net_name, params, 1)
        tr = FusedTrainer(net, lr=0.01, task="reg")
        batch = batch_cpu.clone().to(dev)
        need_w = net_name == "sGAT"
        topo = Topology.from_batch(batch, need_weights=need_w)
        if not tr._can_fuse(topo, n_feat):
            continue                                  # (a shape beyond LDS takes the three-launch path: tested elsewhere)
        ran += 1
        loss = tr.compute_gradients(batch, topo=topo)
        torch.cuda.synchronize()
        where = "case %d: F=%d, %d graphs, nodes %s" % (case, n_feat, n_graphs, [int(g.x.shape[0]) for g in graphs])
        check_step(where, Lazy64(net_name, params, batch_cpu, **_fw_kwargs(net_name)), loss, tr.last_pred.cpu().numpy(),
                   _grads_of(net), ref_loss, ref_pred.numpy(), {k: v.numpy() for k, v in ref_grads.items()}, sweep_stats)
    assert ran >= 6
    assert_arbiter_rate(sweep_stats, "%s sweep" % net_name)


@pytest.mark.parametrize("net_name", NETS)
def test_fused_step_random_shapes_with_a_large_graph_match_oracle(net_name):
    """The same kind of sweep with ONE graph of 280 .. 400 nodes in every mini-batch (the others 4 .. 260): the launch takes
    the from-memory instance for all of them (counted: a sparse large graph may still fit the staged layout) -- tiny graphs next to the large one, every width, rows shorter than
    the padded width, the tiles formed by the stand-alone launch where the builder stages none -- against the oracle.  The
    trainer is handed the Batch only (it builds the workspace itself)."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.data import Batch
    from deeprank_gnn_amd.trainer import FusedTrainer
    from test_gpu_parity import build
    dev = _dev()
    rng = np.random.default_rng(20260930)
    sweep_stats = new_stats()
    from_memory = 0
    for case in range(7):
        n_feat = int(rng.choice([7, 20, 32, 44, 48, 64]))
        n_graphs = int(rng.integers(2, 8))
        big = int(rng.integers(0, n_graphs))
        graphs = []
        for k in range(n_graphs):
            n_nodes = int(rng.integers(280, 401)) if k == big else int(rng.integers(4, 261))
            half = n_nodes // 2
            n_pairs = int(rng.integers(1, max(2, min(1000, 3 * n_nodes, half * (n_nodes - half)))))      # (<= 2000 directed edges)
            n_int = int(rng.integers(1, max(2, min(3 * n_nodes, half * (half - 1) // 2 + 1))))
            graphs.append(synth.make_graph(5000 + 100 * case + k, n_nodes=n_nodes, n_pairs=n_pairs, n_feat=n_feat,
                                           n_c1=int(rng.integers(1, 20)), n_internal=n_int))
        batch_cpu = Batch.from_data_list(graphs)
        params = cpu_ref.init_params(net_name, n_feat, 1, 1, seed=300 + case)
        ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, **_fw_kwargs(net_name))
        net = build(net_name, params, 1)
        tr = FusedTrainer(net, lr=0.01, task="reg")
        batch = batch_cpu.clone().to(dev)
        topo = tr._topology_of(batch, True)
        where = "case %d: F=%d, nodes %s" % (case, n_feat, [int(g.x.shape[0]) for g in graphs])
        plan = tr._plan_for(topo, n_feat, None, True, batch.x)
        assert plan.family == _lib.STEP_FAMILY_AGGREGATE, (where, plan.family, topo.max_edges)
        from_memory += int(plan.from_memory)          # (a sparse 300-node graph still fits the staged layout)
        loss = tr.compute_gradients(batch, topo=topo)
        torch.cuda.synchronize()
        assert tr.faults() == 0
        check_step(where, Lazy64(net_name, params, batch_cpu, **_fw_kwargs(net_name)), loss, tr.last_pred.cpu().numpy(),
                   _grads_of(net), ref_loss, ref_pred.numpy(), {k: v.numpy() for k, v in ref_grads.items()}, sweep_stats)
    assert from_memory >= 4, from_memory
    assert_arbiter_rate(sweep_stats, "%s large-graph sweep" % net_name)


@pytest.mark.parametrize("net_name", NETS)
def test_benchmark_schedule_is_reproducible_and_graph_replays_equal_eager_launches(net_name):
    """Size-independent property of the benchmarked schedule (pipelined topology build, dropout ON for GINet): 240 steps run
    (a) launch by launch, (b) launch by launch again, (c) as hipGraph replays of 20 recorded steps give the same parameters,
    Adam moments, loss and step counter BIT FOR BIT -- fixed-order reductions everywhere, the readout exchange and the
    double-buffered topology workspaces have no timing-dependent outcome; no fault bit is raised."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd.foutnet import FoutNet
    from deeprank_gnn_amd.ginet import GINet
    from deeprank_gnn_amd.sGAT import sGAT
    from deeprank_gnn_amd.topology import Topology
    from deeprank_gnn_amd.trainer import FusedTrainer
    dev = _dev()
    Net = {"GINet": GINet, "sGAT": sGAT, "FoutNet": FoutNet}[net_name]
    batch = synth.make_batch(0, 64).to(dev)
    need_w = net_name == "sGAT"
    STEPS, CHUNK = 240, 20

    def fresh():
        torch.manual_seed(11)
        tr = FusedTrainer(Net(32, 1, 1).to(dev), lr=1e-3, task="reg", seed=77)      # (GINet keeps its dropout of 0.4)
        topos = [Topology.from_batch(batch, need_weights=need_w), Topology.from_batch(batch, need_weights=need_w)]
        return tr, topos

    def step(tr, topos, k):
        tr.train_step(batch, topo=topos[k & 1], next_topo=topos[1 - (k & 1)])

    def state(tr):
        torch.cuda.synchronize()
        assert tr.faults() == 0
        return [t.detach().cpu().numpy().copy() for t in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.loss, tr.step2[:2])]

    runs = []
    for _ in range(2):                                   # (a), (b): eager
        tr, topos = fresh()
        for k in range(STEPS):
            step(tr, topos, k)
        runs.append(state(tr))
    tr, topos = fresh()                                  # (c): recorded
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in range(CHUNK):                           # the first chunk eagerly (warm-up of the capture)
            step(tr, topos, k)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(CHUNK):
            step(tr, topos, k)
    # (the capture itself does not execute: 20 eager steps so far, 220 to go = 11 replays)
    for _ in range((STEPS - CHUNK) // CHUNK):
        g.replay()
    runs.append(state(tr))
    assert int(runs[0][4][0]) == STEPS
    for other in runs[1:]:
        for a, b, name in zip(runs[0], other, ("parameters", "exp_avg", "exp_avg_sq", "loss", "counters")):
            np.testing.assert_array_equal(a, b, err_msg=name)
    assert np.isfinite(runs[0][0]).all() and np.isfinite(runs[0][3]).all()


@pytest.mark.parametrize("net_name,cached,n_graphs,n_feat", [(n, c, 64, 32) for n in NETS for c in (False, True)] +
                         [("GINet", False, 136, 32), ("GINet", True, 136, 32), ("sGAT", False, 136, 32)] +
                         [(n, c, 64, 48) for n in NETS for c in (False, True)] +
                         [("GINet", False, 128, 48), ("GINet", True, 128, 44), ("sGAT", False, 128, 48), ("FoutNet", False, 128, 48),
                          ("GINet", False, 136, 48), ("GINet", True, 136, 48)])
def test_capacity_class_kernels_equal_the_runtime_layout_bit_for_bit(net_name, cached, n_graphs, n_feat):
    """A batch inside the capacity class (200 nodes / 1024 edges / 52 clusters per graph, 32 features -- or up to 48, the feature
    count of the reference's shipped regression models, for the aggregation-first kernels) is stepped by kernels
    whose LDS layout is a compile-time constant (drgnn_step.h: CLS); the layout moves arrays, not arithmetic: three training
    steps give the same bits with the class kernels (default) and without (plan override no_class), rebuilt and cached;
    136 graphs: GINet's one-workgroup layout and the other kinds beyond one round of workgroups."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.foutnet import FoutNet
    from deeprank_gnn_amd.ginet import GINet
    from deeprank_gnn_amd.resident import ResidentGraphSet
    from deeprank_gnn_amd.sGAT import sGAT
    from deeprank_gnn_amd.trainer import FusedTrainer
    dev = _dev()
    api = _lib.get()
    Net = {"GINet": GINet, "sGAT": sGAT, "FoutNet": FoutNet}[net_name]
    batch = synth.make_batch(0, n_graphs, n_feat=n_feat).to(dev)
    rs = ResidentGraphSet([synth.make_graph(i, n_feat=n_feat) for i in range(n_graphs)], dev) if cached else None
    cache = rs.topology_cache(need_weights=(net_name == "sGAT")) if cached else None
    out = []
    for no_class in (0, 1):
        torch.manual_seed(3)
        tr = FusedTrainer(Net(n_feat, 1, 1).to(dev), lr=1e-2, task="reg", seed=5)
        tr.plan_overrides = {"no_class": no_class}
        if cached:
            assert tr._cached_prepare(cache, list(range(n_graphs)))["plan"].cls == 1 - no_class
        else:
            from deeprank_gnn_amd.topology import Topology
            plan = tr._plan_for(Topology.from_batch(batch, need_weights=(net_name == "sGAT")), n_feat)
            assert plan.cls == 1 - no_class
            if net_name == "GINet" and n_graphs > 128:
                # beyond the resident batch size GINet steps both branches in ONE workgroup; its 32- and 48-wide class instances
                # work them off side by side on the two halves of the workgroup (drgnn_step3.h: STEP3B_DUAL, per-branch Z1 / XP /
                # dS) -- compared here bit for bit with the branch-after-branch run-time layout
                assert plan.wgs_per_graph == 1, (plan.wgs_per_graph, plan.lds_bytes)
        for _ in range(3):
            if cached:
                tr.train_step_cached(cache, list(range(n_graphs)))
            else:
                tr.train_step(batch)
        last_pred = tr.last_pred.detach().clone()
        # the inference launch of the same graphs (GINet: class instances too, one workgroup per graph side by side)
        inf = tr.predict_cached(cache, list(range(n_graphs))) if cached else tr.predict(batch)
        torch.cuda.synchronize()
        assert tr.faults() == 0
        out.append([t.detach().cpu().numpy().copy() for t in (tr.flat_p, tr.exp_avg_sq, tr.loss, last_pred, inf)])
    for a, b, name in zip(out[0], out[1], ("parameters", "exp_avg_sq", "loss", "predictions", "inference predictions")):
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert np.isfinite(out[0][0]).all()


# ---- sGAT / FoutNet: the three kernel families (round-3 kernel / aggregation first, one workgroup / node split) --------------
AF_LAYOUTS = {"old": {"no_aggregate": 1}, "af1": {"no_split": 1}, "af2": {}}


def _check_family(tr, c, layout):
    """the plan a prepared step carries is the family / layout the test means to exercise"""
    from deeprank_gnn_amd import _lib
    plan = c["plan"]
    if layout == "old":      # (round 6: the product-first family is not in the device library -- the launch pair steps it)
        assert plan.family == _lib.STEP_FAMILY_NONE, plan.family
        return
    assert plan.family == _lib.STEP_FAMILY_AGGREGATE, (layout, plan.family)
    assert c["slabs"] == plan.slabs_per_graph == (2 if layout == "af2" else 1), (layout, plan.slabs_per_graph)
    assert plan.wgs_per_graph == (2 if layout == "af2" else 1)


@pytest.mark.parametrize("layout", ["old", "af1", "af2"])
@pytest.mark.parametrize("net_name", ["sGAT", "FoutNet"])
def test_single_branch_step_families_syn64_match_oracle_elementwise(net_name, layout):
    """sGAT / FoutNet at the benchmarked shape through every kernel family: the round-3 kernel (drgnn_step.h), the
    aggregation-first kernel with one workgroup per graph and with the graph split between two workgroups that exchange
    pooled rows (drgnn_step2.h; sGAT.py:62-93,114-138, foutnet.py:56-82,103-125).  Loss, predictions and EVERY gradient
    element vs the oracle; three Adam steps through the ping-ponged launches vs torch.optim.Adam; the split launch is
    bit-reproducible."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.topology import Topology
    dev = _dev()
    api = _lib.get()
    batch_cpu = synth.make_batch(0, 64)
    params = cpu_ref.init_params(net_name, 32, 1, 1, seed=11)
    kw = _fw_kwargs(net_name)
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, **kw)
    lazy = Lazy64(net_name, params, batch_cpu, **kw)
    batch = batch_cpu.clone().to(dev)
    need_w = net_name == "sGAT"
    if True:
        net, tr = _trainer(net_name, params)
        tr.plan_overrides = dict(AF_LAYOUTS[layout])
        topo = Topology.from_batch(batch, need_weights=need_w)
        nxt = Topology.from_batch(batch, need_weights=need_w, build=False)
        _check_family(tr, tr._fused_prepare(batch, topo, True, nxt), layout)
        loss = tr.compute_gradients(batch, topo=topo, next_topo=nxt)
        torch.cuda.synchronize()
        stats = new_stats()
        check_step("%s SYN64 %s" % (net_name, layout), lazy, loss, tr.last_pred.cpu().numpy(), _grads_of(net), ref_loss,
                   ref_pred.numpy(), {k: v.numpy() for k, v in ref_grads.items()}, stats)
        assert_arbiter_rate(stats, "%s %s" % (net_name, layout))
        assert tr.faults() == 0
        g1 = {k: v.copy() for k, v in _grads_of(net).items()}
        loss2 = tr.compute_gradients(batch, topo=nxt)          # the co-built topology, same launch layout: bit-identical
        assert float(loss2) == float(loss)
        for k, v in _grads_of(net).items():
            assert np.array_equal(v, g1[k]), k
        # three optimiser steps
        leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        opt = torch.optim.Adam(list(leaves.values()), lr=0.01)
        net, tr = _trainer(net_name, params, lr=0.01)
        tr.plan_overrides = dict(AF_LAYOUTS[layout])
        topos = [topo, nxt]
        for it in range(3):
            opt.zero_grad()
            pred = cpu_ref.FORWARD[net_name](leaves, batch_cpu, **kw)
            lref = F.mse_loss(pred.reshape(-1), batch_cpu.y)
            lref.backward()
            opt.step()
            got = tr.train_step(batch, topo=topos[it & 1], next_topo=topos[1 - (it & 1)])
            np.testing.assert_allclose(float(got), float(lref.detach()), rtol=TOL)
        sd = net.state_dict()
        for k, v in leaves.items():
            np.testing.assert_allclose(sd[k].cpu().numpy(), v.detach().numpy(), rtol=TOL, atol=TOL, err_msg=k)


@pytest.mark.parametrize("layout", ["old", "af1", "af2"])
@pytest.mark.parametrize("net_name", ["sGAT", "FoutNet", "GINet"])
def test_step_families_ragged_batches_vs_oracle(net_name, layout):
    """Every kernel family on ragged batches (tests/step_check.py: graphs of 1 .. 49 nodes, a single-node graph that leaves
    one half of the split EMPTY, isolated nodes -> FoutNet's NaN rows / sGAT's bias rows (sGAT.py:62-93, foutnet.py:71-73),
    self loops, duplicate edges, non-consecutive cluster ids), classification and regression, feature widths 32 / 20 / 28 /
    12 / 44 / 60 / 7 / 26 / 33 (padded 32, 32, 32, 16, 48, 64, 16, 32, 48): loss, predictions and EVERY gradient element vs the ORACLE on the same
    inputs (tests/elementwise.py: 1e-4 + 1e-4 |ref|, float64 arbiter), NaN pattern equal.  GINet: the product-first family
    ("old"), the aggregation-first one-workgroup ("af1") and two-workgroup ("af2") layouts."""
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.topology import Topology
    from deeprank_gnn_amd.trainer import FusedTrainer
    from test_gpu_parity import build
    dev = _dev()
    rng = np.random.default_rng(5)
    from step_check import ragged_batch
    kw = _fw_kwargs(net_name)
    # (7 / 26 / 33: feature counts that are not multiples of 4 -- the aggregation-first kernels read padded tile rows)
    for seed, (n_feat, task) in enumerate(((32, "reg"), (20, "class"), (28, "reg"), (12, "reg"), (44, "class"), (60, "reg"),
                                           (7, "reg"), (26, "class"), (33, "reg"))):
        batch_cpu = ragged_batch(seed, n_feat)          # 7 graphs: 1 .. 49 nodes, a single-node graph, isolated nodes, self loops, duplicates
        batch_cpu.y = torch.arange(batch_cpu.num_graphs, dtype=torch.float32) * 0.3 - 1.0
        n_out = 1 if task == "reg" else 3
        params = cpu_ref.init_params(net_name, n_feat, n_out, 1, seed=4)
        if task == "class":
            batch_cpu.y = torch.from_numpy(rng.integers(0, 3, size=int(batch_cpu.y.shape[0]))).long()
        ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, task=task, **kw)
        lazy = Lazy64(net_name, params, batch_cpu, task=task, **kw)
        batch = batch_cpu.clone().to(dev)
        need_w = net_name == "sGAT"
        net = build(net_name, params, n_out)
        tr = FusedTrainer(net, lr=0.01, task=task)
        if net_name == "GINet":
            tr.plan_overrides = {"old": {"no_aggregate": 1}, "af1": {"force_wgs": 1}, "af2": {}}[layout]
        else:
            tr.plan_overrides = dict(AF_LAYOUTS[layout])
        topo = Topology.from_batch(batch, need_weights=need_w)
        assert tr._can_fuse(topo, n_feat, None, True, batch.x) == (layout != "old")
        c = tr._fused_prepare(batch, topo)
        if layout == "old":      # (the launch pair: drgnn_net_forward + drgnn_net_backward_fused_head)
            assert c["plan"].family == _lib.STEP_FAMILY_NONE
        elif net_name == "GINet":
            assert c["plan"].family == _lib.STEP_FAMILY_AGGREGATE
            assert c["plan"].wgs_per_graph == (1 if layout == "af1" else 2)
        else:
            _check_family(tr, c, layout)
        if layout != "old":
            assert c["plan"].width == ((n_feat + 15) // 16) * 16
        loss = tr.compute_gradients(batch, topo=topo)
        torch.cuda.synchronize()
        assert tr.faults() == 0
        stats = new_stats()
        check_step("%s ragged F=%d %s %s" % (net_name, n_feat, task, layout), lazy, float(loss), tr.last_pred.cpu().numpy(),
                   _grads_of(net), ref_loss.detach(), ref_pred.detach().numpy(), {k: v.numpy() for k, v in ref_grads.items()}, stats)
        # (ragged batches are a few thousand elements: the 0.1 % arbiter budget would be a handful)
        assert stats["arbiter"] <= max(3, stats["elements"] // 200), stats
