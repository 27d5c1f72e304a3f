"""The topology builder at the sizes where it changes its code path (tests/topo_cases.py), on the device.

Only a device build runs: the single-pass tail of the lean clusters chain (C127; C128 is the scan tail on the device), the
register-prefetched ids (`pre`: N1024 on, N1025 off), the DPP group sums and four-keys-per-trip counting loops (the C* cases),
the per-wave participation tests (E63 - E65), the one-wave loop over the split candidates wrapping at 64 (C127 - C129, N1024 /
N1025) and the block-to-graph mapping of two workgroups per graph (B*).  The outputs are integers and exact sums: besides the
oracle, the device is held to the emulation's bits."""
import numpy as np
import pytest
import torch

import topo_cases as T

pytestmark = pytest.mark.gpu
_built = {}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def built(name, weights, flags_name):
    """one device build per variant, shared by the tests that compare workspaces"""
    key = (name, weights, flags_name)
    if key not in _built:
        _built[key] = T.build(T.BY_NAME[name].batch(), None, _dev(), weights, T.FLAGS[flags_name])
    return _built[key]


@pytest.mark.parametrize("name,weights,flags_name", T.variants())
def test_topology_paths_on_the_device(name, weights, flags_name):
    case = T.BY_NAME[name]
    topo = built(name, weights, flags_name)
    assert topo.status()[0] == 0 and int(topo.flags) == T.FLAGS[flags_name]
    T.check_topology(topo, case.batch(), weights)
    if T.FLAGS[flags_name] & T.LEAN:
        T.check_same_bits(built(name, weights, "default"), topo, weights)


@pytest.mark.parametrize("name", [c.name for c in T.WELL_FORMED])
def test_tiles_are_left_out_exactly_where_the_case_says(name):
    case = T.BY_NAME[name]
    topo = T.build(case.batch(), None, _dev(), False, None, build=False)
    assert (topo.tiles is None) == (case.no_tiles is not None), (name, case.no_tiles)
    assert (topo._inputs[-1] is not None) == case.global_scratch          # (the global scratch buffer)


@pytest.mark.parametrize("name", T.STRIPPED)
@pytest.mark.parametrize("host_tables", [True, False])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("flags_name", ["default", "lean"])
def test_topology_paths_without_the_collate_time_tables(name, host_tables, weights, flags_name):
    batch = T.strip_layout(T.BY_NAME[name].batch().clone())
    topo = T.build(batch, None, _dev(), weights, T.FLAGS[flags_name], host_tables=host_tables)
    assert topo.status()[0] == 0
    assert (topo.host_node_ptr is not None) == host_tables
    T.check_topology(topo, batch, weights)
    T.check_same_bits(built(name, weights, "default"), topo, weights, "collated / stripped")


@pytest.mark.parametrize("name", T.ALONE)
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("flags_name", ["default", "lean"])
def test_a_graph_alone_equals_the_graph_in_its_batch(name, weights, flags_name):
    T.check_alone_equals_batch(T.BY_NAME[name], None, _dev(), weights, T.FLAGS[flags_name])


@pytest.mark.parametrize("name", [c.name for c in T.MALFORMED])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("flags_name", ["default", "lean"])
def test_a_cluster1_list_of_the_wrong_length(name, weights, flags_name):
    T.check_malformed(T.BY_NAME[name], None, _dev(), weights, T.FLAGS[flags_name])


@pytest.mark.parametrize("name", T.DEVICE_VS_EMU)
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("flags_name", ["default", "lean"])
def test_the_device_builds_the_emulations_bits(name, weights, flags_name):
    """Integers and exact fixed-point sums: what the device builds is what the host emulation of the same source builds,
    whichever tail, prefetch or group sum either of them ran."""
    from emu_api import emu
    host = T.build(T.BY_NAME[name].batch(), emu(), None, weights, T.FLAGS[flags_name])
    assert host.status()[0] == 0
    T.check_same_bits(host, built(name, weights, flags_name), weights, "emulation / device")


@pytest.mark.parametrize("name", T.TWICE)
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("flags_name", ["default", "lean"])
def test_two_builds_of_one_request_give_the_same_bytes(name, weights, flags_name):
    topo = T.build(T.BY_NAME[name].batch(), None, _dev(), weights, T.FLAGS[flags_name])
    assert topo.status()[0] == 0
    first_i = topo.ws_i32.clone()
    first_f = topo.ws_f32.clone() if weights else None
    topo.rebuild(T.FLAGS[flags_name])
    assert topo.status()[0] == 0
    assert torch.equal(topo.ws_i32, first_i)
    if weights:
        assert torch.equal(topo.ws_f32.view(torch.int32), first_f.view(torch.int32))


# the co-launched builder: 16 graphs of 3 C nodes, 8 C edges and 16 features per (net, C, depth-1 clusters)
CO_LAUNCHED = [(net, C, n_c1) for net in ("GINet", "sGAT") for C, n_c1 in ((33, 7), (65, 7), (128, 70))]


@pytest.mark.parametrize("net_name,C,n_c1", CO_LAUNCHED)
def test_the_co_launched_builder_at_the_cluster_edges(net_name, C, n_c1):
    """The builder compiled into the step kernels (GINet: WEIGHTS = 0, sGAT: with weights) builds the NEXT mini-batch's
    workspace in the step launch: status 0, the oracle's topology, and the bits of a stand-alone build with the flags the
    trainer asked for (the lean chains wherever the next launch is lean-ready)."""
    from oracle import cpu_ref
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.data import Batch
    from deeprank_gnn_amd.topology import Topology
    from test_gpu_width_classes import _trainer
    dev = _dev()
    batch_cpu = Batch.from_data_list([T.clusters_graph(C, n_c1, n_feat=16, seed=k) for k in range(16)])
    f = T.facts(batch_cpu, 0)
    assert f["C"] == C and f["rc"] == 0 and f["tail"] == ("single" if C < 128 else "scan")
    need_w = net_name == "sGAT"
    params = cpu_ref.init_params(net_name, 16, 1, 1, seed=17)
    net, tr = _trainer(net_name, params, 1, "reg")
    batch = batch_cpu.clone().to(dev)
    topo = Topology.from_batch(batch, need_weights=need_w)
    nxt = Topology.from_batch(batch, need_weights=need_w, build=False)
    plan = tr._fused_prepare(batch, topo, True, nxt)["plan"]
    # (every one of these shapes is within the fused kernels' reach: tests/test_gpu_width_classes.py runs 400-node graphs at
    # this width)
    assert plan.family == _lib.STEP_FAMILY_AGGREGATE and plan.builder_wgs_per_graph >= 1, (plan.family, plan.builder_wgs_per_graph)
    want_flags = tr._flags_for(nxt, 16)
    assert want_flags & T.LEAN, want_flags          # the next launch is lean-ready: the co-launched builder runs the lean chains
    tr.compute_gradients(batch, topo=topo, next_topo=nxt)
    torch.cuda.synchronize()
    assert tr.faults() == 0
    assert nxt.status()[0] == 0 and int(nxt.flags) == want_flags
    T.check_topology(nxt, batch_cpu, need_w)
    alone = Topology.from_batch(batch, need_weights=need_w, flags=want_flags)
    assert alone.status()[0] == 0
    T.check_same_bits(alone, nxt, need_w, "stand-alone / co-launched", hier=bool(want_flags & T.HIER))
    if want_flags & T.TILES:
        n = topo.api.topology_tiles_elems(nxt.n_nodes, 16)
        assert torch.equal(alone.tiles[:n].view(torch.int32), nxt.tiles[:n].view(torch.int32))
