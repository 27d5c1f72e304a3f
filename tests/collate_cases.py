"""Inputs and checks shared by tests/test_emu_collate.py (host emulation) and tests/test_gpu_collate.py (the device) for
the resident graph set beyond nine graphs: drgnn_collate, drgnn_batch_offsets (csrc/drgnn_collate.h) and what
ResidentGraphSet puts around them (resident.py).

    slot counts     B and batch_size on both sides of a wave (64), of a workgroup (DRGNN_NTHREADS = 1024) and of the 4096
                    drgnn_batch_offsets accepts: the second stride of collate_block's slot loop, W = batch_size + 1 on both
                    sides of the 1024 at which wg_exscan leaves its one-element-per-lane path for the chunked one
    row copies      n_feat with F % 4 == 0 (128-bit copies in the device build) and the others (scalar copies)
    optional data   sets without edge_attr / y / cluster1 / cluster0, int64 targets, targets replaced between batches
    raw entries     ids outside the set (they select nothing, collate_extent) and every refusal before a launch

Every call takes (api, device): api = emu() with "cpu", api = None (the product library) with "cuda".

No expectation here comes from the code under test: they are Batch.from_data_list (the restated PyG collate pinned by
tests/golden/collate.npz) and numpy prefix sums of the graphs' own sizes.  Everything is a copy or an integer shift: every
comparison is exact.  A reference batch is computed once per (set, selection) and left unchanged."""
import numpy as np
import pytest
import torch

from collate_check import assert_same_batch, check_collate, check_set_topology, ragged_graphs
from deeprank_gnn_amd import _lib
from deeprank_gnn_amd._lib import DrgnnError
from deeprank_gnn_amd.data import Batch
from deeprank_gnn_amd.resident import ResidentGraphSet

N_TINY = 1100                   # more slots than a workgroup has lanes
TINY_FEAT = 4                   # one 128-bit copy per node in the device build
SLOT_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 1100)
ROW_FEATS = (1, 2, 3, 4, 5, 8, 12, 36, 64, 68)
OFFSET_BATCH_SIZES = (1, 63, 64, 65, 1022, 1023, 1024, 1025, 4095, 4096)
N_ORDER = 9000
MAX_BATCH = 4096                # drgnn_batch_offsets: DRGNN_E_CAPACITY beyond
PAD = 5                         # sentinel elements behind every raw output
I_SENT, F_SENT = -77, -77.5     # neither a node id, an offset, a slot number, a target nor a drawn float


def tiny_graphs(count, n_feat, seed):
    """`count` graphs of 1-5 nodes and 0 to 3n drawn edges, alternately symmetric and directed; every 7th graph and every
    1-node graph has no edge; y of a graph is its index, its name is t<index>"""
    from test_emu_topology import random_graph
    rng = np.random.default_rng(seed)
    graphs = []
    for k in range(count):
        n = int(rng.integers(1, 6))
        e = 0 if (k % 7 == 0 or n == 1) else int(rng.integers(0, 3 * n + 1))
        g = random_graph(rng, n, e, int(rng.integers(1, n + 1)), int(rng.integers(1, 5)), sym=bool(k % 2))
        g.x = torch.from_numpy(rng.standard_normal((n, n_feat)).astype(np.float32))
        g.edge_attr = torch.from_numpy(rng.uniform(0.1, 2.0, (g.edge_index.size(1), 1)).astype(np.float32))
        g.y = torch.tensor([float(k)])
        g.mol = "t%d" % k
        graphs.append(g)
    return graphs


def mixed_graphs(n_feat, seed=21, n_tiny=60):
    """ragged_graphs (up to 50 nodes, a 1-node graph at 2) followed by tiny graphs: slots of very different extents next to
    each other; y of a graph is 1000 + its index"""
    graphs = ragged_graphs(seed, n_feat) + tiny_graphs(n_tiny, n_feat, seed + 1)
    for k, g in enumerate(graphs):
        g.y = torch.tensor([1000.0 + k])
        g.mol = "m%d" % k
    return graphs


_GRAPHS, _SETS, _WANT = {}, {}, {}


def set_graphs(name):
    """the graphs of the two shared sets: "tiny" (1100 tiny graphs, F = 4) and "mixed" (9 ragged + 60 tiny graphs, F = 5)"""
    if name not in _GRAPHS:
        _GRAPHS[name] = tiny_graphs(N_TINY, TINY_FEAT, 17) if name == "tiny" else mixed_graphs(5)
    return _GRAPHS[name]


def tiny_set_graphs():
    return set_graphs("tiny")


def mixed_set_graphs():
    return set_graphs("mixed")


def resident(name, api, device):
    """the resident set over the graphs `name` ("tiny" / "mixed"), uploaded once per build"""
    key = (name, str(device), id(api))
    if key not in _SETS:
        _SETS[key] = ResidentGraphSet(set_graphs(name), device, api=api)
    return _SETS[key]


def reference(name, ids):
    """Batch.from_data_list of the graphs `ids` of the set `name`, computed once and left unchanged"""
    key = (name, tuple(int(i) for i in ids))
    if key not in _WANT:
        graphs = set_graphs(name)
        _WANT[key] = Batch.from_data_list([graphs[i] for i in key[1]])
    return _WANT[key]


def sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


# ---- 1. collate at the slot-count edges ------------------------------------------------------------------------------
def slot_selections(graphs, B):
    """(name, ids) of B slots: a permutation prefix, the reversed range, repeated ids with the same one in the first and
    the last slot, and a selection of edge-less graphs only (E = 0: the edge buffers are empty)"""
    G = len(graphs)
    rng = np.random.default_rng(100 + B)
    again = rng.integers(0, G, B)
    again[0] = again[-1] = again[B // 2] = int(rng.integers(0, G))
    if B > 4:
        again[1] = again[2]
    bare = np.asarray([k for k, g in enumerate(graphs) if g.num_edges == 0])
    assert bare.size > 100
    return [("permutation", rng.permutation(G)[:B].tolist()), ("reversed", list(range(G - 1, G - 1 - B, -1))),
            ("repeated", again.tolist()), ("edge-less", rng.choice(bare, B).tolist())]


def check_slot_counts(B, api, device):
    graphs = tiny_set_graphs()
    rs = resident("tiny", api, device)
    picks = slot_selections(graphs, B)
    dev_ids = rs.upload_ids([i for _, ids in picks for i in ids])         # one upload, sliced per batch
    lo = 0
    for name, ids in picks:
        want = reference("tiny", ids)
        if name == "edge-less":
            assert want.edge_index.size(1) == 0
        assert_same_batch(rs.batch(ids), want)
        got = rs.batch(ids, dev_ids[lo:lo + B])
        assert_same_batch(got, want)
        if name == "edge-less":
            assert tuple(got.edge_index.shape) == (2, 0) and tuple(got.edge_attr.shape) == (0, 1)
        lo += B


# ---- 2. row-copy paths -----------------------------------------------------------------------------------------------
def check_row_copies(n_feat, api, device):
    """F % 4 == 0: 128-bit copies in the device build, else scalar ones; graphs of odd node counts, a 1-node graph in the
    first and in the last slot, large and tiny rows next to each other"""
    graphs = mixed_graphs(n_feat, seed=40 + n_feat)
    G = len(graphs)
    single = [k for k, g in enumerate(graphs) if g.num_nodes == 1]
    assert len(single) >= 2 and any(g.num_nodes % 2 == 1 and g.num_nodes > 1 for g in graphs)
    rng = np.random.default_rng(n_feat)
    middle = rng.permutation(G).tolist()
    selections = [[single[0]] + middle + [single[-1]], [single[-1]] + list(range(G - 1, -1, -1)) + [single[0]],
                  [single[0]], single[:2]]
    rs = check_collate(graphs, device, api=api, selections=selections)
    assert rs.n_feat == n_feat and rs.x.data_ptr() % 16 == 0             # (a torch allocation: nothing misaligned)


# ---- 3. optional fields and targets ----------------------------------------------------------------------------------
def without(graphs, field):
    out = []
    for g in graphs:
        h = g.clone()
        if field in ("edge_attr", "y"):
            setattr(h, field, None)
        else:
            h.__dict__.pop(field)
        out.append(h)
    return out


def check_without(field, api, device, B=65):
    graphs = without(mixed_set_graphs(), field)
    G = len(graphs)
    rng = np.random.default_rng(3)
    ids = rng.permutation(G)[:B].tolist()
    rs = check_collate(graphs, device, api=api, selections=[ids, ids[::-1]])
    got = rs.batch(ids)
    assert got[field] is None
    if field == "cluster1":
        assert "_c1_ptr" not in got.__dict__
        # the third offset table of a set without cluster1 is all zeros
        ptrs = rs.batch_offsets(rs.upload_ids(ids), 16)
        assert ptrs.shape == (5, 3, 17) and not bool(ptrs[:, 2].any()) and bool(ptrs[:, 0, 1:].all())
        assert_offsets(ptrs, expected_offsets(rs, ids, 16), "a set without cluster1")


def int_targets(G):
    """distinct int64 class targets that differ in both 32-bit halves"""
    return torch.arange(G, dtype=torch.int64) * ((1 << 33) + 3) - 5


def check_int64_targets(api, device):
    graphs = tiny_set_graphs()
    G = len(graphs)
    rs = ResidentGraphSet(graphs, device, api=api)
    rng = np.random.default_rng(8)
    picks = {B: rng.permutation(G)[:B].tolist() for B in (65, 1025)}
    first = rs.batch(picks[65])                                           # a batch taken before the targets change
    assert first.y.dtype == torch.float32 and first.y.tolist() == [float(i) for i in picks[65]]
    y64 = int_targets(G)
    rs.set_targets(y64)
    for B, ids in picks.items():
        for got in (rs.batch(ids), rs.batch(ids, rs.upload_ids(ids))):
            assert got.y.dtype == torch.int64 and tuple(got.y.shape) == (B,)
            assert got.y.cpu().tolist() == y64[ids].tolist()
            want = reference("tiny", ids).clone()
            want.y = y64[ids]
            assert_same_batch(got, want)
    assert first.y.tolist() == [float(i) for i in picks[65]]              # (the earlier batch owns its targets)
    back = torch.arange(G, dtype=torch.float32) * 0.5 + 0.25              # and back to float
    rs.set_targets(back)
    for B, ids in picks.items():
        got = rs.batch(ids)
        assert got.y.dtype == torch.float32 and got.y.cpu().tolist() == back[ids].tolist()
    with pytest.raises(ValueError):
        rs.set_targets(back[:-1])


# ---- 4. batch_offsets ------------------------------------------------------------------------------------------------
def visiting_order():
    return np.random.default_rng(33).integers(0, N_TINY, N_ORDER)


def expected_offsets(rs, ids, batch_size, n_graphs=None):
    """int32 [n_batches, 3, batch_size + 1]: np.concatenate([[0], np.cumsum(counts[ids])]) per mini-batch and table; ids
    outside [0, n_graphs) and the slots behind a short last mini-batch count zero, so its tail repeats its total"""
    ids = np.asarray(ids, dtype=np.int64)
    G = len(rs) if n_graphs is None else n_graphs
    nb = (ids.size + batch_size - 1) // batch_size
    inside = (ids >= 0) & (ids < G)
    out = np.zeros((nb, 3, batch_size + 1), dtype=np.int64)
    for t, counts in enumerate((rs.n_nodes, rs.n_edges, rs.n_c1)):
        c = np.zeros(nb * batch_size, dtype=np.int64)
        c[:ids.size] = np.where(inside, counts[np.where(inside, ids, 0)], 0)
        out[:, t, 1:] = np.cumsum(c.reshape(nb, batch_size), axis=1)
    assert out.max(initial=0) < 2 ** 31
    return out.astype(np.int32)


def assert_offsets(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        k, t, q = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError("%s: mini-batch %d table %d entry %d is %d, expected %d"
                             % (what, k, t, q, got[k, t, q], want[k, t, q]))


def check_batch_offsets(batch_size, api, device):
    rs = resident("tiny", api, device)
    order = visiting_order()
    lengths = [N_ORDER, 2 * batch_size if 2 * batch_size <= N_ORDER else batch_size,       # exact multiples
               batch_size, batch_size - 1, 1, batch_size + 1]                              # n_ids < batch_size; one over
    ids_dev = rs.upload_ids(order)
    for n in sorted(set(v for v in lengths if v > 0), reverse=True):
        got = rs.batch_offsets(ids_dev[:n], batch_size)
        want = expected_offsets(rs, order[:n], batch_size)
        if n % batch_size:                                                # the short last mini-batch: its tail is its total
            B = n % batch_size
            assert (want[-1, :, B:] == want[-1, :, B:B + 1]).all()
        assert_offsets(got, want, "batch_size %d, %d ids" % (batch_size, n))


def raw_offsets(api, desc, ids_dev, n_ids, batch_size, device, n_batches=None):
    """api.batch_offsets into a sentinel-filled buffer with PAD sentinels behind it -> (tables, padding)"""
    nb = (n_ids + batch_size - 1) // batch_size if n_batches is None else n_batches
    words = nb * 3 * (batch_size + 1)
    buf = torch.full((words + PAD,), I_SENT, dtype=torch.int32, device=device)
    api.batch_offsets(desc, ids_dev, n_ids, batch_size, buf, _lib.current_stream(buf))
    sync(device)
    return buf[:words].reshape(nb, 3, batch_size + 1), buf[words:]


def check_batch_offsets_no_ids(api, device):
    """n_ids == 0 returns without a launch: the output is untouched"""
    rs = resident("tiny", api, device)
    ids_dev = rs.upload_ids([5])
    tables, pad = raw_offsets(rs.api, rs._desc, ids_dev, 0, 64, device, n_batches=1)
    assert bool((tables == I_SENT).all()) and bool((pad == I_SENT).all())
    tables, pad = raw_offsets(rs.api, rs._desc, ids_dev, 1, 64, device)   # and one id fills one mini-batch's tables
    assert_offsets(tables, expected_offsets(rs, [5], 64), "one id")
    assert bool((pad == I_SENT).all())


def check_batch_offsets_capacity(api, device):
    """batch_size 4097 (DRGNN_E_CAPACITY) and 0 (DRGNN_E_ARG) are refused with the output untouched; 4096 runs"""
    rs = resident("tiny", api, device)
    order = visiting_order()[:MAX_BATCH + 1]
    ids_dev = rs.upload_ids(order)
    buf = torch.full((3 * (MAX_BATCH + 2) + PAD,), I_SENT, dtype=torch.int32, device=device)
    stream = _lib.current_stream(buf)
    with pytest.raises(DrgnnError, match="capacity"):
        rs.api.batch_offsets(rs._desc, ids_dev, MAX_BATCH + 1, MAX_BATCH + 1, buf, stream)
    with pytest.raises(DrgnnError, match="capacity"):
        rs.batch_offsets(ids_dev, MAX_BATCH + 1)
    for bad in (0, -1, -MAX_BATCH):
        with pytest.raises(DrgnnError, match="bad argument"):
            rs.api.batch_offsets(rs._desc, ids_dev, MAX_BATCH + 1, bad, buf, stream)
    sync(device)
    assert bool((buf == I_SENT).all())
    tables, pad = raw_offsets(rs.api, rs._desc, ids_dev, MAX_BATCH, MAX_BATCH, device)
    assert_offsets(tables, expected_offsets(rs, order[:MAX_BATCH], MAX_BATCH), "batch_size 4096")
    assert bool((pad == I_SENT).all())


# ---- 5. resident-set topology mode -----------------------------------------------------------------------------------
def check_topology(which, batch_size, need_weights, api, device):
    graphs = tiny_set_graphs() if which == "tiny" else mixed_set_graphs()
    check_set_topology(graphs, device, api=api, need_weights=need_weights, batch_size=batch_size)


# ---- 6. ids outside the set on the raw entries -----------------------------------------------------------------------
def copy_desc(desc, **over):
    d = _lib.GraphSet()
    for name, _ in _lib.GraphSet._fields_:
        setattr(d, name, getattr(desc, name))
    for k, v in over.items():
        setattr(d, k, v)
    return d


class RawCollate(object):
    """Sentinel-filled outputs for api.collate of the graphs `valid` of `rs` in `n_slots` slots, PAD sentinels behind each"""

    def __init__(self, rs, valid, n_slots):
        dev = rs.device
        valid = np.asarray(valid, dtype=np.int64)
        self.rs, self.B = rs, n_slots
        self.N, self.E = int(rs.n_nodes[valid].sum()), int(rs.n_edges[valid].sum())
        self.C = int(rs.n_c1[valid].sum())
        ints = lambda n, dtype=torch.int64: torch.full((n + PAD,), I_SENT, dtype=dtype, device=dev)
        self.x = torch.full((self.N + PAD, rs.n_feat), F_SENT, dtype=torch.float32, device=dev)
        self.edge_index = ints(2 * self.E)                                # rows [0, E) and [E, 2E), the padding behind
        self.edge_attr = torch.full((self.E + PAD,), F_SENT, dtype=torch.float32, device=dev)
        self.batch, self.cluster0, self.cluster1 = ints(self.N), ints(self.N), ints(self.C)
        self.y = torch.full((n_slots + PAD,), F_SENT if rs.y.is_floating_point() else I_SENT, dtype=rs.y.dtype, device=dev)
        self.node_ptr, self.edge_ptr, self.c1_ptr = (ints(n_slots + 1, torch.int32) for _ in range(3))

    NAMES = ("x", "edge_index", "edge_attr", "batch", "cluster0", "cluster1", "y", "node_ptr", "edge_ptr", "c1_ptr")

    def call(self, ids_dev, desc=None, **over):
        a = {k: getattr(self, k) for k in self.NAMES}
        a.update(ids=ids_dev, n_graphs=self.B, n_nodes=self.N, n_edges=self.E)
        a.update(over)
        self.rs.api.collate(self.rs._desc if desc is None else desc, a["ids"], a["n_graphs"], a["n_nodes"], a["n_edges"],
                            a["x"], a["edge_index"], a["edge_attr"], a["batch"], a["cluster0"], a["cluster1"], a["y"],
                            a["node_ptr"], a["edge_ptr"], a["c1_ptr"], _lib.current_stream(self.x))

    def untouched(self):
        sync(self.rs.device)
        for k in self.NAMES:
            t = getattr(self, k)
            sent = F_SENT if t.is_floating_point() else I_SENT
            assert bool((t == sent).all()), k
        return True


def outside_id_lists(G):
    return ([3, G, 5, -1, 7],
            [G, 2, -(2 ** 31), 2, 2 ** 31 - 1],                         # empty first and last slot, a 1-node graph twice
            [-1] * 70 + [4] + [G + 1] * 70 + [0, G - 1])                 # more empty slots than a wave in front of a valid one


N_OUTSIDE_LISTS = 3


def check_collate_outside_ids(which, api, device):
    """ids outside the set select nothing (collate_extent): the valid slots are Batch.from_data_list of the valid graphs
    with `batch` carrying their slot numbers, the offset tables repeat across the empty slots, whose y stays as it was"""
    rs = resident("mixed", api, device)
    G = len(rs)
    ids = outside_id_lists(G)[which]
    slots = [q for q, i in enumerate(ids) if 0 <= i < G]
    valid = [ids[q] for q in slots]
    assert valid and len(valid) < len(ids)
    want = reference("mixed", valid)
    out = RawCollate(rs, valid, len(ids))
    out.call(torch.tensor(ids, dtype=torch.int32).to(device))
    sync(device)
    N, E, C, B = out.N, out.E, out.C, out.B
    assert torch.equal(out.x[:N].cpu(), want.x)
    assert torch.equal(out.edge_index[:2 * E].reshape(2, E).cpu(), want.edge_index)
    assert torch.equal(out.edge_attr[:E].cpu(), want.edge_attr.reshape(-1))
    assert torch.equal(out.cluster0[:N].cpu(), want.cluster0) and torch.equal(out.cluster1[:C].cpu(), want.cluster1)
    assert out.batch[:N].cpu().tolist() == [slots[g] for g in want.batch.tolist()]
    inside = np.asarray([0 <= i < G for i in ids])
    pick = np.where(inside, np.asarray(ids, dtype=np.int64), 0)
    for name, counts in (("node_ptr", rs.n_nodes), ("edge_ptr", rs.n_edges), ("c1_ptr", rs.n_c1)):
        table = np.concatenate([[0], np.cumsum(np.where(inside, counts[pick], 0))])
        assert getattr(out, name)[:B + 1].cpu().tolist() == table.tolist(), name
    y = out.y[:B].cpu().tolist()
    assert [y[q] for q in slots] == want.y.tolist()
    assert all(y[q] == F_SENT for q in range(B) if q not in slots)
    for t, used in ((out.x, N), (out.edge_index, 2 * E), (out.edge_attr, E), (out.batch, N), (out.cluster0, N),
                    (out.cluster1, C), (out.y, B), (out.node_ptr, B + 1), (out.edge_ptr, B + 1), (out.c1_ptr, B + 1)):
        sent = F_SENT if t.is_floating_point() else I_SENT
        assert t.size(0) == used + PAD and bool((t[used:] == sent).all())


def check_offsets_outside_ids(api, device):
    rs = resident("mixed", api, device)
    G = len(rs)
    ids = [3, G, 5, -1, 7, G + 100, 0, 2 ** 31 - 1, -(2 ** 31), G - 1, G]
    ids_dev = torch.tensor(ids, dtype=torch.int32).to(device)
    for batch_size in (3, 4, 11, 65):
        tables, pad = raw_offsets(rs.api, rs._desc, ids_dev, len(ids), batch_size, device)
        assert_offsets(tables, expected_offsets(rs, ids, batch_size), "ids outside the set, batch_size %d" % batch_size)
        assert bool((pad == I_SENT).all())


def check_offsets_outside_declared_set(api, device):
    """The descriptor declares 8 graphs fewer than its tables hold: the numbers of those 8 are outside the set and count
    zero, and no extent read can leave a table whatever the kernel makes of them"""
    rs = resident("mixed", api, device)
    G = len(rs)
    short = copy_desc(rs._desc, n_graphs=G - 8)
    ids = [3, G - 8, 5, G - 2, 7, G - 9, G - 5]
    assert all(rs.n_nodes[i] > 0 for i in ids)
    ids_dev = torch.tensor(ids, dtype=torch.int32).to(device)
    for batch_size in (3, 7, 65):
        want = expected_offsets(rs, ids, batch_size, n_graphs=G - 8)
        tables, pad = raw_offsets(rs.api, short, ids_dev, len(ids), batch_size, device)
        assert_offsets(tables, want, "ids outside the declared set, batch_size %d" % batch_size)
        assert bool((pad == I_SENT).all())
    assert int(want[0, 0, 7]) == int(rs.n_nodes[[3, 5, 7, G - 9]].sum())


# ---- 7. refusals before a launch -------------------------------------------------------------------------------------
def check_collate_refusals(api, device):
    """every DRGNN_E_ARG / DRGNN_E_CAPACITY exit of drgnn_collate, each with otherwise valid sentinel-filled buffers:
    DrgnnError and nothing written; n_graphs == 0 returns 0 and launches nothing; the good call then runs"""
    rs = resident("mixed", api, device)
    ids = [3, 2, 40, 7, 2]
    want = reference("mixed", ids)
    ids_dev = rs.upload_ids(ids)
    out = RawCollate(rs, ids, len(ids))
    assert out.N > 0 and out.E > 0 and out.C > 0
    d = rs._desc
    bad = [dict(ids=None), dict(node_ptr=None), dict(edge_ptr=None), dict(x=None), dict(batch=None), dict(edge_index=None),
           dict(n_graphs=-1), dict(n_nodes=-1), dict(n_edges=-1),
           dict(desc=copy_desc(d, edge_attr=None)),                       # edge_attr asked of a set without one
           dict(desc=copy_desc(d, cluster0=None)),
           dict(desc=copy_desc(d, cluster1=None)),
           dict(desc=copy_desc(d, c1_ptr=None)),                          # cluster1 of a set without its offsets
           dict(c1_ptr=None),                                             # cluster1 without c1_ptr
           dict(desc=copy_desc(d, y=None))]
    bad += [dict(desc=copy_desc(d, y_bytes=v)) for v in (0, 2, 12, 16, -4)]
    bad += [dict(desc=copy_desc(d, n_feat=v)) for v in (0, -1)]
    bad += [dict(desc=copy_desc(d, n_graphs=-1)), dict(desc=copy_desc(d, node_ptr=None)),
            dict(desc=copy_desc(d, edge_ptr=None)), dict(desc=copy_desc(d, x=None)),
            dict(desc=copy_desc(d, edge_index=None))]
    for over in bad:
        with pytest.raises(DrgnnError, match="bad argument"):
            out.call(ids_dev, **over)
    for over in (dict(n_nodes=2 ** 31), dict(n_edges=2 ** 31)):           # int32 offset tables
        with pytest.raises(DrgnnError, match="capacity"):
            out.call(ids_dev, **over)
    with pytest.raises(DrgnnError, match="bad argument"):                 # no set at all
        p = _lib._ptr
        _lib._check(rs.api.lib.drgnn_collate(None, p(ids_dev), out.B, out.N, out.E, p(out.x), p(out.edge_index),
                                             p(out.edge_attr), p(out.batch), p(out.cluster0), p(out.cluster1), p(out.y),
                                             p(out.node_ptr), p(out.edge_ptr), p(out.c1_ptr), _lib.current_stream(out.x)),
                    "drgnn_collate")
    assert out.untouched()
    out.call(ids_dev, n_graphs=0)                                         # returns 0, launches nothing
    assert out.untouched()
    # sets that really lack a field refuse it as well
    for field, arg in (("edge_attr", "edge_attr"), ("cluster0", "cluster0"), ("cluster1", "cluster1")):
        lean = ResidentGraphSet(without(mixed_set_graphs(), field), device, api=rs.api)
        with pytest.raises(DrgnnError, match="bad argument"):
            out.call(ids_dev, desc=lean._desc)
    assert out.untouched()
    out.call(ids_dev)                                                     # the same buffers, nothing overridden
    sync(device)
    N, E, C, B = out.N, out.E, out.C, out.B
    assert torch.equal(out.x[:N].cpu(), want.x) and torch.equal(out.batch[:N].cpu(), want.batch)
    assert torch.equal(out.edge_index[:2 * E].reshape(2, E).cpu(), want.edge_index)
    assert torch.equal(out.y[:B].cpu(), want.y) and torch.equal(out.cluster1[:C].cpu(), want.cluster1)
    assert torch.equal(out.c1_ptr[:B + 1].cpu(), want._c1_ptr)


def check_offsets_refusals(api, device):
    """every DRGNN_E_ARG exit of drgnn_batch_offsets with an otherwise valid sentinel-filled buffer"""
    rs = resident("mixed", api, device)
    ids = [3, 2, 40, 7, 2]
    ids_dev = rs.upload_ids(ids)
    buf = torch.full((2 * 3 * 4 + PAD,), I_SENT, dtype=torch.int32, device=device)
    stream = _lib.current_stream(buf)
    d = rs._desc
    good = dict(desc=d, ids=ids_dev, n_ids=5, batch_size=3, ptrs=buf)
    bad = [dict(ids=None), dict(ptrs=None), dict(n_ids=-1), dict(batch_size=0), dict(batch_size=-3),
           dict(desc=copy_desc(d, node_ptr=None)), dict(desc=copy_desc(d, edge_ptr=None))]
    for over in bad:
        a = dict(good, **over)
        with pytest.raises(DrgnnError, match="bad argument"):
            rs.api.batch_offsets(a["desc"], a["ids"], a["n_ids"], a["batch_size"], a["ptrs"], stream)
    with pytest.raises(DrgnnError, match="bad argument"):
        _lib._check(rs.api.lib.drgnn_batch_offsets(None, _lib._ptr(ids_dev), 5, 3, _lib._ptr(buf), stream),
                    "drgnn_batch_offsets")
    sync(device)
    assert bool((buf == I_SENT).all())
    rs.api.batch_offsets(d, ids_dev, 5, 3, buf, stream)
    sync(device)
    assert_offsets(buf[:24].reshape(2, 3, 4), expected_offsets(rs, ids, 3), "the good call")
    assert bool((buf[24:] == I_SENT).all())


# ---- 8. upload_ids ---------------------------------------------------------------------------------------------------
def check_upload_ids_range(api, device):
    rs = resident("mixed", api, device)
    G = len(rs)
    for ids in ([0, G], [-1], [G - 1, 0, -G], [2 ** 31]):
        with pytest.raises(IndexError):
            rs.upload_ids(ids)
        with pytest.raises(IndexError):
            rs.batch(ids)
    ok = rs.upload_ids([G - 1, 0])
    assert ok.dtype == torch.int32 and ok.device == rs.device and ok.tolist() == [G - 1, 0]
    assert rs.upload_ids([]).numel() == 0


def check_upload_ids_ring(device):
    """The pinned staging ring (capacity 1024, four slots, a side stream): uploads below, at and beyond its capacity (it
    grows), then six in a row without a synchronisation, which goes round its four slots; one synchronisation at the end"""
    rs = ResidentGraphSet(mixed_set_graphs(), device)
    G = len(rs)
    rng = np.random.default_rng(6)
    sent, got = [], []
    for n in (1, 1024, 1025, 5000, 3):
        sent.append(rng.integers(0, G, n))
        got.append(rs.upload_ids(sent[-1]))
    ring = rs.__dict__["_id_staging"]
    assert len(ring["slots"]) == 4 and ring["slots"][0][0].numel() == 5000 and ring["slots"][0][0].is_pinned()
    for n in (7, 5000, 2, 1024, 4999, 1):
        sent.append(rng.integers(0, G, n))
        got.append(rs.upload_ids(sent[-1]))
    torch.cuda.synchronize()
    for a, b in zip(sent, got):
        assert b.dtype == torch.int32 and b.is_cuda and b.cpu().tolist() == a.tolist()


# ---- 9. image round trip ---------------------------------------------------------------------------------------------
def check_image_round_trip(path, api, device, B=65):
    graphs = mixed_set_graphs()
    rs = resident("mixed", api, device)
    rs.save(path)
    back = ResidentGraphSet.load(path, device, api=rs.api)
    assert len(back) == len(rs) and back.mols == rs.mols and back.device == rs.device
    rng = np.random.default_rng(2)
    for ids in (rng.permutation(len(graphs))[:B].tolist(), list(range(B))[::-1]):
        want = reference("mixed", ids)
        assert_same_batch(back.batch(ids), want)
        assert_same_batch(back.batch(ids), rs.batch(ids))
