"""The topology builder at the sizes where it changes its code path (tests/topo_cases.py), through the host-emulation build.
CPU only.  The emulation runs the scan tail of the lean clusters chain, serial group sums and no register prefetch: the
device-only forms of the same cases are tests/test_gpu_topology_paths.py."""
import numpy as np
import pytest

import topo_cases as T
from emu_api import emu

_built = {}


def built(name, weights, flags_name):
    """one emulation build per variant, shared by the tests that compare workspaces"""
    key = (name, weights, flags_name)
    if key not in _built:
        _built[key] = T.build(T.BY_NAME[name].batch(), emu(), None, weights, T.FLAGS[flags_name])
    return _built[key]


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_case_sits_on_its_edge(name):
    """From numpy alone: the inequality of the case's row holds for the batch the maker produced."""
    case = T.BY_NAME[name]
    batch = case.batch()
    f = T.facts(batch, case.special, case.global_scratch)
    assert case.edge(f), (name, case.sits_on, {k: v for k, v in f.items() if k != "sizes"})
    lds = emu().topology_lds_bytes(f["max_nodes"], f["max_edges"])
    if case.force:
        assert emu().topology_lds_bytes(T.FORCED_GLOBAL, T.FORCED_GLOBAL) > T.LDS_LIMIT
    elif case.global_scratch:
        assert lds > T.LDS_LIMIT, (name, lds)
    else:
        assert not f["forced"] and lds <= T.LDS_LIMIT, (name, lds)      # (capT / capF of `facts` are the LDS carve's)


def test_sizes_next_to_the_special_graphs():
    """What the table states beside the special graph: the LDS need at N1024 / N1025, the second packed_edge_ids graph, the
    ordinary neighbours on the lean chain, the graphs of one_cluster."""
    api = emu()
    assert api.topology_lds_bytes(1024, 2048) == 152304 <= 160 * 1024
    assert api.topology_lds_bytes(1025, 2050) == 152480 <= 160 * 1024
    f = T.facts(T.BY_NAME["packed_edge_ids"].batch(), 2)
    assert f["E"] == 0x10001 and f["C"] == 300
    for name in ("C32", "C128", "E64", "signed_weights"):
        batch = T.BY_NAME[name].batch()
        assert all(T.facts(batch, g)["rc"] == 0 for g in range(batch.num_graphs)), name
    batch = T.BY_NAME["one_cluster"].batch()
    assert [(T.facts(batch, g)["N"], T.facts(batch, g)["E"]) for g in (2, 3)] == [(1, 0), (5, 0)]
    # the pooled runs of signed_weights' second graph hold about 400 addends each
    f = T.facts(T.BY_NAME["signed_weights"].batch(), 1)
    assert f["E"] / (f["C"] * (f["C"] - 1)) > 400
    w = T.BY_NAME["signed_weights"].batch().edge_attr.numpy()
    assert (w > 0).any() and (w < 0).any() and np.abs(w).max() / np.abs(w[w != 0]).min() > 1e9
    assert not T.BY_NAME["zero_weights"].batch().edge_attr.numpy().any()


@pytest.mark.parametrize("name,weights,flags_name", T.variants())
def test_topology_paths(name, weights, flags_name):
    case = T.BY_NAME[name]
    batch = case.batch()
    topo = built(name, weights, flags_name)
    assert topo.status()[0] == 0 and int(topo.flags) == T.FLAGS[flags_name]
    T.check_topology(topo, batch, weights)
    if T.FLAGS[flags_name] & T.LEAN:
        T.check_same_bits(built(name, weights, "default"), topo, weights)


@pytest.mark.parametrize("name", [c.name for c in T.WELL_FORMED])
def test_tiles_are_left_out_exactly_where_the_case_says(name):
    case = T.BY_NAME[name]
    topo = T.build(case.batch(), emu(), None, False, None, build=False)
    assert (topo.tiles is None) == (case.no_tiles is not None), (name, case.no_tiles)
    assert (topo._inputs[-1] is not None) == case.global_scratch          # (the global scratch buffer)


@pytest.mark.parametrize("name", T.STRIPPED)
@pytest.mark.parametrize("host_tables", [True, False])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("flags_name", ["default", "lean"])
def test_topology_paths_without_the_collate_time_tables(name, host_tables, weights, flags_name):
    batch = T.strip_layout(T.BY_NAME[name].batch().clone())
    topo = T.build(batch, emu(), None, weights, T.FLAGS[flags_name], host_tables=host_tables)
    assert topo.status()[0] == 0
    assert (topo.host_node_ptr is not None) == host_tables
    T.check_topology(topo, batch, weights)
    T.check_same_bits(built(name, weights, "default"), topo, weights, "collated / stripped")


@pytest.mark.parametrize("name", T.ALONE)
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("flags_name", ["default", "lean"])
def test_a_graph_alone_equals_the_graph_in_its_batch(name, weights, flags_name):
    fa, fb = T.check_alone_equals_batch(T.BY_NAME[name], emu(), None, weights, T.FLAGS[flags_name])
    if name == "C129_roomy":        # capT comes from the batch's largest graph: alone the lean chain refuses it (rc == 2)
        assert (fa["rc"], fb["rc"]) == (2, 0)
    else:
        assert fa["rc"] == fb["rc"]


@pytest.mark.parametrize("name", [c.name for c in T.MALFORMED])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("flags_name", ["default", "lean"])
def test_a_cluster1_list_of_the_wrong_length(name, weights, flags_name):
    T.check_malformed(T.BY_NAME[name], emu(), None, weights, T.FLAGS[flags_name])
