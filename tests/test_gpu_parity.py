"""Parity tests proper: the HIP library on a real MI355X vs golden vectors / the CPU oracle.
All calls go through the C ABI (deeprank-gnn_amd/csrc/libdrgnn.so).  Tolerance 1e-4 fp32
(BASELINE.json north_star); integer topology is compared exactly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import CASES, golden, params_of, fixture_batch, fixture_graphs, syn4_batch
from topo_check import check_against_oracle
from oracle import cpu_ref
from elementwise import (SWEEP_SEEDS, Lazy64, assert_arbiter_rate, check, check_step, check_step_kinks, describe, kink_line,
                         new_stats)

pytestmark = pytest.mark.gpu
TOL = 1e-4


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nets():
    from deeprank_gnn_amd.ginet import GINet
    from deeprank_gnn_amd.sGAT import sGAT
    from deeprank_gnn_amd.foutnet import FoutNet
    return {"GINet": GINet, "sGAT": sGAT, "FoutNet": FoutNet}


def build(net_name, params, n_out):
    n_feat = {"GINet": lambda: params["conv1.fc.weight"].shape[1],
              "sGAT": lambda: params["conv1.weight"].shape[0] // 2,
              "FoutNet": lambda: params["conv1.Wc"].shape[0]}[net_name]()
    net = nets()[net_name](n_feat, n_out, 1)
    net.load_state_dict(params, strict=True)
    if hasattr(net, "dropout"):
        net.dropout = 0.0
    return net.to(dev())


def test_library_is_the_hip_build():
    from deeprank_gnn_amd import _lib
    api = _lib.get()
    assert api.path.endswith("csrc/libdrgnn.so")
    assert api.lib.drgnn_abi_version() == 5
    mapped = [ln.split()[-1] for ln in open("/proc/self/maps") if "libdrgnn" in ln]
    assert any(m.endswith("csrc/libdrgnn.so") for m in mapped), mapped
    # the package's API object must be bound to the gfx950 build, not to the host-emulation build of the CPU suite
    assert "libdrgnn_emu" not in api.path


@pytest.mark.parametrize("which", ["fix8", "fix10", "syn4", "syn3_full", "derived"])
def test_topology_vs_oracle(which):
    from deeprank_gnn_amd.topology import Topology
    import deeprank_gnn_amd.synthetic as synth
    batch = {"fix8": lambda: fixture_batch(8), "fix10": lambda: fixture_batch(10), "syn4": syn4_batch,
             "syn3_full": lambda: synth.make_batch(0, 3), "derived": lambda: fixture_batch(8)}[which]()
    if which == "derived":
        for k in ("_node_ptr", "_edge_ptr", "_c1_ptr", "_max_nodes", "_max_edges", "_max_c0"):
            batch.__dict__.pop(k, None)
    gb = batch.clone().to(dev())
    for weights in (True, False):        # False: pooled graph through the bitmap path
        topo = Topology.from_batch(gb, need_weights=weights)
        assert topo.status()[0] == 0
        check_against_oracle(topo, batch, weights=weights)


def test_topology_random_ragged_and_global_scratch():
    from test_emu_topology import random_graph
    from deeprank_gnn_amd.data import Batch
    from deeprank_gnn_amd.topology import Topology
    for seed in range(4):
        rng = np.random.default_rng(100 + seed)
        graphs = []
        for k in range(9):
            n = int(rng.integers(1, 60))
            e = int(rng.integers(0, 5 * n))
            graphs.append(random_graph(rng, n, e, int(rng.integers(1, n + 1)), int(rng.integers(1, 5)),
                                       sym=bool(k % 2), self_loops=(k == 3), dup=(k == 4)))
        batch = Batch.from_data_list(graphs)
        if seed == 3:
            batch.__dict__["_max_nodes"] = 100000      # LDS estimate too large -> global scratch
            batch.__dict__["_max_edges"] = 100000
        for weights in (True, False):
            topo = Topology.from_batch(batch.clone().to(dev()), need_weights=weights)
            assert topo.status()[0] == 0
            check_against_oracle(topo, batch, weights=weights)


def test_topology_flags_bad_input():
    from deeprank_gnn_amd.topology import Topology
    from deeprank_gnn_amd import _lib
    batch = syn4_batch()
    batch.edge_index[1, 3] = batch.x.size(0) - 1
    topo = Topology.from_batch(batch.to(dev()))
    assert topo.status()[0] & 1
    with pytest.raises(_lib.DrgnnError):
        topo.check()


@pytest.mark.parametrize("fname", sorted(CASES))
def test_net_vs_reference_golden(fname):
    from deeprank_gnn_amd.topology import Topology
    net_name, make_batch, task = CASES[fname]
    g = golden(fname)
    batch = make_batch().to(dev())
    net = build(net_name, params_of(g), g["out"].shape[1])
    net.train()
    topo = Topology.from_batch(batch, check=True)
    # every float is compared ELEMENT-WISE with the reference-generated golden (|got - ref| <= 1e-4 + 1e-4 |ref|); an
    # element that misses it is arbitrated by the oracle in float64 on the same inputs, and at most 0.1 % may (elementwise.py)
    target_cpu = torch.from_numpy(g["target"])
    lazy = Lazy64(net_name, params_of(g), make_batch(), target=target_cpu, task=task, want_trace=True)
    stats = new_stats()
    readout = net.body(batch, topo)
    check(fname + " readout", readout.detach().cpu().numpy(), g["readout"], lambda: lazy.traced("readout"), stats)
    out = net(batch)                                   # default path: builds its own topology
    # ... and runs on the aggregation-first step kernels (fused_autograd), like test_fused_step_vs_reference_golden's launches
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.fused_autograd import engine_for
    eng = engine_for(net)
    assert eng.last_path == ("jacobian" if out.shape[1] == 1 else "two-launch") and eng.last_plan.family == _lib.STEP_FAMILY_AGGREGATE, \
        eng.last_reason
    target = target_cpu.to(dev())
    loss = F.mse_loss(out.reshape(-1), target) if task == "reg" else F.cross_entropy(out, target)
    loss.backward()
    grads = {}
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        grads[name] = p.grad.cpu().numpy()
    check_step(fname, lazy, loss.item(), out.detach().cpu().numpy(), grads, g["loss"], g["out"],
               {name: g["grad/" + name] for name in grads}, stats)
    assert_arbiter_rate(stats, fname)


@pytest.mark.parametrize("path", ["fused", "pair"])
@pytest.mark.parametrize("net_name", ["GINet", "sGAT", "FoutNet"])
def test_full_size_batch_vs_oracle_and_determinism(net_name, path):
    """BASELINE configs[1..3]: 64 synthetic graphs (200 nodes, ~1000 edges, 32 features) through model(batch) / loss.backward(),
    on the fused step kernels (fused_autograd) and on the launch pair (functional.net_body + the head in torch).

    The two paths are pinned on different parameter seeds for a reason worth stating: with seed 5 GINet's conv2_ext has ONE
    pre-activation of 7.8e-7 (float64; 6.0e-7 in the fp32 reference) that is also the maximum of its depth-1 cluster.  ReLU'
    of that element is 1 on one side of fp32 round-off and 0 on the other, and the whole gradient of that readout channel
    goes through it: the aggregation-first kernels, which associate conv1 as (A x) W, land on the other side of zero than
    torch's A (x W) does, and 180 elements of d conv1_ext.fc.weight move by up to 2e-4 of the tensor's maximum while the
    predictions agree to 8e-7 (tools/r06/jacobian_fullsize_check.py; tools/r06/relu_kink_seed5.py reproduces the kernels'
    value in float64 by moving that one element across zero).  No evaluation order is "the" fp32 answer at a kink,
    so that seed stays with the launch pair (product first, the reference's order), and the fused kernels take seed 11, the
    seed test_gpu_fused_fullsize.py pins FusedTrainer's step on.  test_syn64_kink_sweep runs both paths on the same seeds,
    seed 5 included, through the kink arbiter that resolves such a decision."""
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.fused_autograd import engine_for
    from deeprank_gnn_amd.topology import Topology
    batch_cpu = synth.make_batch(0, 64)
    params = cpu_ref.init_params(net_name, 32, 1, 1, seed=(11 if path == "fused" else 5))
    kw = {"looped": False} if net_name == "FoutNet" else {}
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, **kw)
    net = build(net_name, params, 1)
    eng = engine_for(net)
    if path == "pair":
        eng.plan_overrides = {"no_aggregate": 1}
    batch = batch_cpu.clone().to(dev())

    def run():
        net.zero_grad(set_to_none=True)
        # (tiles of the net's flavour: edge-weighted sums are sGAT's)
        topo = Topology.from_batch(batch, need_weights=(net_name == "sGAT"))
        out = net(batch, topo=topo)
        loss = F.mse_loss(out.reshape(-1), batch.y)
        loss.backward()
        return out.detach().clone(), loss.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    out1, loss1, g1 = run()
    if path == "fused":
        assert eng.last_path == "jacobian" and eng.last_plan.family == _lib.STEP_FAMILY_AGGREGATE, eng.last_reason
    else:
        assert eng.last_path is None and "no fused kernel" in eng.last_reason
    out2, loss2, g2 = run()
    assert torch.equal(out1, out2) and torch.equal(loss1, loss2)      # bit-reproducible: no float atomics
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    check_step("%s SYN64 (autograd path, %s)" % (net_name, path), Lazy64(net_name, params, batch_cpu, **kw), loss1.item(),
               out1.cpu().numpy(), {k: v.cpu().numpy() for k, v in g1.items()}, ref_loss, ref_pred.numpy(),
               {k: v.numpy() for k, v in ref_grads.items()})


_SYN64 = {}


def _syn64():
    if "batch" not in _SYN64:
        import deeprank_gnn_amd.synthetic as synth
        _SYN64["batch"] = synth.make_batch(0, 64)
    return _SYN64["batch"]


SWEEP = [(net_name, seed) for net_name, seeds in SWEEP_SEEDS.items() for seed in seeds]


@pytest.mark.parametrize("path", ["fused", "pair"])
@pytest.mark.parametrize("net_name,seed", SWEEP)
def test_syn64_kink_sweep(net_name, seed, path):
    """SYN64, regression, through model(batch) / loss.backward(), on the SAME parameter seeds for both paths (the fused step
    kernels and the launch pair), checked with the kink arbiter (elementwise.check_step_kinks): a result that misses the
    strict rule passes only as the exact gradient of the network with one to four near decisions flipped, and names them.
    Fused at seed 5 is the known case: GINet's one b.z2 pre-activation of 7.8e-7 that is its depth-1 cluster's maximum
    (tools/r06/relu_kink_seed5.py)."""
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.fused_autograd import engine_for
    from deeprank_gnn_amd.topology import Topology
    batch_cpu = _syn64()
    params = cpu_ref.init_params(net_name, 32, 1, 1, seed=seed)
    kw = {"looped": False} if net_name == "FoutNet" else {}
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads(net_name, params, batch_cpu, batch_cpu.y, **kw)
    net = build(net_name, params, 1)
    eng = engine_for(net)
    if path == "pair":
        eng.plan_overrides = {"no_aggregate": 1}
    batch = batch_cpu.clone().to(dev())

    def run():
        net.zero_grad(set_to_none=True)
        topo = Topology.from_batch(batch, need_weights=(net_name == "sGAT"))
        out = net(batch, topo=topo)
        loss = F.mse_loss(out.reshape(-1), batch.y)
        loss.backward()
        return out.detach().clone(), loss.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    out1, loss1, g1 = run()
    if path == "fused":
        assert eng.last_path == "jacobian" and eng.last_plan.family == _lib.STEP_FAMILY_AGGREGATE, eng.last_reason
    else:
        assert eng.last_path is None and "no fused kernel" in eng.last_reason
    out2, loss2, g2 = run()
    assert torch.equal(out1, out2) and torch.equal(loss1, loss2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    where = "%s seed %d %s" % (net_name, seed, path)
    report = check_step_kinks(where, Lazy64(net_name, params, batch_cpu, **kw), loss1.item(), out1.cpu().numpy(),
                              {k: v.cpu().numpy() for k, v in g1.items()}, ref_loss, ref_pred.numpy(),
                              {k: v.numpy() for k, v in ref_grads.items()})
    print(kink_line(where, report))
    if (net_name, seed, path) == ("GINet", 5, "fused"):
        assert [(d["site"], d["kind"], d["graph"], d["channel"]) for d in report["F"]] == [("b.z2", "zero", 19, 27)], \
            describe(report["F"])


@pytest.mark.parametrize("seed", SWEEP_SEEDS["GINet"][:8])
def test_syn64_kink_sweep_fused_trainer(seed):
    """FusedTrainer.compute_gradients (the benchmarked launch) on GINet SYN64 at seeds 0-7, through the kink arbiter."""
    from deeprank_gnn_amd.topology import Topology
    from deeprank_gnn_amd.trainer import FusedTrainer
    batch_cpu = _syn64()
    params = cpu_ref.init_params("GINet", 32, 1, 1, seed=seed)
    ref_pred, ref_loss, ref_grads = cpu_ref.loss_and_grads("GINet", params, batch_cpu, batch_cpu.y)
    net = build("GINet", params, 1)
    tr = FusedTrainer(net, lr=0.01, task="reg")
    batch = batch_cpu.clone().to(dev())

    def run():
        loss = tr.compute_gradients(batch, topo=Topology.from_batch(batch))
        torch.cuda.synchronize()
        return (float(loss), tr.last_pred.detach().clone(),
                {k: p.grad.detach().clone() for k, p in net.named_parameters()})

    loss1, out1, g1 = run()
    loss2, out2, g2 = run()
    assert loss1 == loss2 and torch.equal(out1, out2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    where = "GINet seed %d trainer" % seed
    report = check_step_kinks(where, Lazy64("GINet", params, batch_cpu), loss1, out1.cpu().numpy(),
                              {k: v.cpu().numpy() for k, v in g1.items()}, ref_loss, ref_pred.numpy(),
                              {k: v.numpy() for k, v in ref_grads.items()})
    print(kink_line(where, report))


def test_global_scratch_path_matches_lds_path():
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd.topology import Topology
    batch = synth.make_batch(0, 6, n_nodes=80, n_pairs=150).to(dev())
    params = cpu_ref.init_params("sGAT", 32, 1, 1, seed=7)
    net = build("sGAT", params, 1)
    # (the launch pair of functional.net_body: what runs outside the fused step kernels' LDS budget)
    topo = Topology.from_batch(batch)
    a = net.body(batch, topo=topo)
    topo2 = Topology.from_batch(batch)
    topo2.max_nodes = 0                                 # forces the global-scratch variant
    b = net.body(batch, topo=topo2)
    assert torch.equal(a, b)
    # ... and the whole net through it (unknown bounds: no fused step) against the fused step kernels' predictions
    from deeprank_gnn_amd.fused_autograd import engine_for
    fused = net(batch, topo=topo)
    assert engine_for(net).last_path == "jacobian", engine_for(net).last_reason
    pair = net(batch, topo=topo2)
    assert engine_for(net).last_path is None
    np.testing.assert_allclose(fused.detach().cpu().numpy(), pair.detach().cpu().numpy(), rtol=1e-5, atol=1e-5)


def test_batch_invariance():
    """Same graphs batched vs one at a time (pins collate offsets + per-graph cluster offsets)."""
    graphs = fixture_graphs(count=5)
    from deeprank_gnn_amd.data import Batch
    params = cpu_ref.init_params("GINet", 28, 1, 1, seed=3)
    net = build("GINet", params, 1)
    net.eval()
    together = net(Batch.from_data_list(graphs).to(dev()))
    single = torch.cat([net(Batch.from_data_list([g]).to(dev())) for g in graphs])
    np.testing.assert_allclose(together.detach().cpu().numpy(), single.detach().cpu().numpy(), rtol=1e-5, atol=1e-5)


def test_pretrained_classifier_known_answer():
    from deeprank_gnn_amd.data import Batch
    g = golden("pretrained_class.npz")
    graphs = fixture_graphs(node_feature=[str(s) for s in g["node_feature"]], target=None)
    net = build("GINet", params_of(g), 2)
    net.eval()
    out = net(Batch.from_data_list(graphs).to(dev()))
    np.testing.assert_allclose(out.detach().cpu().numpy(), g["logits_batched"], rtol=1e-4, atol=1e-4)


def test_smoke_entry():
    import __graft_entry__
    __graft_entry__.smoke()


@pytest.mark.gpu
@pytest.mark.parametrize("weights", [False, True])
def test_lean_topology_on_the_device_equals_the_full_build(weights):
    """TOPO_LEAN (the builder's short chains: concatenated scan, orders by counting / size sums, transposed bitmap) at the
    benchmarked shape and on a ragged batch: the oracle's topology, and bit for bit the full build's arrays."""
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.topology import Topology
    from topo_check import check_against_oracle
    import deeprank_gnn_amd.synthetic as synth
    dev = torch.device("cuda:0")
    for batch_cpu in (synth.make_batch(0, 64), synth.make_batch(3, 5, n_nodes=37, n_pairs=60, n_feat=8, n_c1=4, n_internal=10),
                      synth.make_batch(0, 170, n_nodes=20, n_pairs=30, n_feat=4, n_c1=3, n_internal=6)):
        batch = batch_cpu.clone().to(dev)
        full = Topology.from_batch(batch, need_weights=weights)
        lean = Topology.from_batch(batch, need_weights=weights, flags=_lib.TOPO_HIER | _lib.TOPO_LEAN)
        assert lean.status()[0] == 0 and (lean.flags & _lib.TOPO_LEAN)
        check_against_oracle(lean, batch_cpu, weights=weights)
        nptr, eptr = full.array("NPTR").cpu().numpy(), full.array("EPTR").cpu().numpy()
        nc0, ne1, nc1 = (full.array(k).cpu().numpy() for k in ("NC0", "NE1", "NC1"))
        for name in ["ROWPTR0", "COL0", "CL0", "ROWPTR1", "COL1", "COLPTR1", "ROWIDX1", "CL1", "MPTR1", "MEM1", "HORD", "HMP0", "HSPLIT"]:
            a, b = full.array(name).cpu().numpy(), lean.array(name).cpu().numpy()
            for g in range(full.n_graphs):
                n0, N, e0, E, C, E1 = nptr[g], nptr[g + 1] - nptr[g], eptr[g], eptr[g + 1] - eptr[g], nc0[g], ne1[g]
                lo, n = {"ROWPTR0": (n0 + g, N + 1), "COL0": (e0, E), "CL0": (n0, N), "ROWPTR1": (n0 + g, C + 1), "COL1": (e0, E1),
                         "COLPTR1": (n0 + g, C + 1), "ROWIDX1": (e0, E1), "CL1": (n0, C), "MPTR1": (n0 + g, nc1[g] + 1),
                         "MEM1": (n0, C), "HORD": (n0, N), "HMP0": (n0 + g, C + 1), "HSPLIT": (4 * g, 4)}[name]
                np.testing.assert_array_equal(a[lo:lo + n], b[lo:lo + n], err_msg="%s graph %d" % (name, g))
        if weights:       # W0 by slot and the fixed-point sums W1: the same bits from both chains
            for name, count in (("W0", np.diff(eptr)), ("W1", ne1)):
                a, b = (t.weights(name).cpu().numpy().view(np.int32) for t in (full, lean))
                for g in range(full.n_graphs):
                    np.testing.assert_array_equal(a[eptr[g]:eptr[g] + count[g]], b[eptr[g]:eptr[g] + count[g]],
                                                  err_msg="%s graph %d" % (name, g))


@pytest.mark.gpu
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("lean", [False, True])
def test_aggregation_tiles_on_the_device(weights, lean):
    """TOPO_TILES at the benchmarked shape, on a ragged batch and beyond 160 graphs (one builder workgroup per graph)."""
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.topology import Topology
    from topo_check import check_against_oracle, check_tiles
    import deeprank_gnn_amd.synthetic as synth
    dev = torch.device("cuda:0")
    flags = _lib.TOPO_HIER | _lib.TOPO_TILES | (_lib.TOPO_LEAN if lean else 0)
    for batch_cpu in (synth.make_batch(0, 64), synth.make_batch(3, 5, n_nodes=37, n_pairs=60, n_feat=8, n_c1=4, n_internal=10),
                      synth.make_batch(0, 170, n_nodes=20, n_pairs=30, n_feat=4, n_c1=3, n_internal=6),
                      synth.make_batch(7, 6, n_nodes=45, n_pairs=80, n_feat=7, n_c1=4, n_internal=10),      # (rows padded to 8 floats)
                      synth.make_batch(4, 5, n_nodes=45, n_pairs=80, n_feat=7, n_c1=4, n_internal=10),      # (an ODD node total: 225)
                      synth.make_batch(1, 9, n_nodes=132, n_pairs=300, n_feat=26, n_c1=9, n_internal=60)):  # (... to 28)
        batch = batch_cpu.clone().to(dev)
        topo = Topology.from_batch(batch, need_weights=weights, flags=flags)
        assert topo.status()[0] == 0 and topo.tiles is not None
        check_against_oracle(topo, batch_cpu, weights=weights)
        check_tiles(topo, batch_cpu, weights)
