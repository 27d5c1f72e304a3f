"""The function-level pooling API (deeprank-gnn_amd/community_pooling.py; kernels segpool_fwd_block, segmax_bwd_item,
edge_export_block and cluster_{max,scan,add} of csrc/drgnn_layers.h) beyond the fixture graphs: ragged batches whose graphs
need a second and third trip of the 1024-lane loops, widths that do not divide them, gapped and offset cluster ids, ties,
NaN and -inf.  Shared by test_emu_pool.py (host emulation) and test_gpu_pool.py (MI355X).

References.  Everything is compared with plain numpy restatements written here (``ref_max``, ``ref_sums``,
``ref_pooled_edges``: loops / np.add.at in float64) and with oracle/cpu_ref.py where it states the operation
(consecutive_cluster, pool_edge, scatter_max, get_preloaded_cluster).  ``check_references_on_fixture`` ties the numpy
restatements to cpu_ref -- which tests/test_oracle_golden.py pins on the reference's own vectors -- on the fixture batch.

Bounds.  Integers, maxima, arg-max rows and gradients of the max are compared EXACTLY.  Float sums have derived bounds
(u = 2^-24, the unit round-off of float32):

  * cluster sums and means (``sum_bound`` / ``mean_bound``).  The kernel adds the k members of a cluster one after the other
    in float32 and divides once by k; scatter_sum multiplies the mean by k again.  A sequential float32 sum of k terms is
    within (k - 1) u sum|x_i| of the exact one (to first order in u), the division adds one rounding of the quotient
    (<= u sum|x_i| / k) and the multiplication one of the product (<= u sum|x_i|): together (k + 1) u sum|x_i|, and k + 2
    absorbs the terms of second order (k u << 1).  So
        |sum  - ref64| <= (k + 2) u sum|x_i|          per (cluster, channel)
        |mean - ref64| <= (k + 2) u sum|x_i| / k      (the same chain without the multiplication, divided by k)

  * pooled edge attributes (``edge_bound``).  The builder (csrc/drgnn_topology.h: topo_wscale, topo_wfix) turns every
    addend into 64-bit fixed point with steps of 2^(ex - 40), where 2^(ex - 1) <= wmax < 2^ex and wmax is the largest |w|
    of the graph, adds the integers exactly and rounds the total to float32 once.  An addend is therefore off by at most
    half a step, 2^(ex - 41) (and by nothing when |w| >= 2^-16 wmax), and with k addends
        |attr - ref64| <= u |ref64| + (1 + u) k 2^(ex - 41)  (+ k 2^-52 sum|w_i| for the float64 reference's own sum).

Every check prints the worst ratio of error to bound it met ("POOL ratio ...").
"""
import contextlib
import functools
import types

import numpy as np
import torch

import deeprank_gnn_amd.community_pooling as cp
from deeprank_gnn_amd.data import Batch, Data
from oracle import cpu_ref

U = 2.0 ** -24
NODES = (1, 64, 65, 1500)           # nodes per graph of the ragged batch
WIDTHS = (1, 33, 200)
VARIANTS = ("random", "shapes")
BIG = len(NODES) - 1                # the graph that holds the planted rows


@contextlib.contextmanager
def using(api):
    """the function API on ``api`` (the host-emulation build) or, with None, on the product library"""
    cp._API = api
    try:
        yield
    finally:
        cp._API = None


# ---- references (plain numpy, float64) ----------------------------------------------------------------------------
def ref_max(x, labels):
    """(cons [N], maxima [C, H] float32, arg [C, H]) of torch_scatter.scatter_max over the consecutive ranks of ``labels``:
    rows are visited in node order and replace the running maximum on a strict '>', so the FIRST row of a tie wins, a NaN
    never does and -inf never beats the start value; a cell nothing entered is 0 with arg = N."""
    x = np.asarray(x)
    n, h = x.shape
    uniq, cons = np.unique(np.asarray(labels), return_inverse=True)
    best = np.full((len(uniq), h), -np.inf)
    arg = np.full((len(uniq), h), n, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            c = cons[i]
            v = x[i].astype(np.float64)
            better = v > best[c]
            best[c, better] = v[better]
            arg[c, better] = i
    return cons, np.where(arg == n, 0.0, best).astype(np.float32), arg


def ref_sums(x, labels):
    """(cons, sum [C, H], sum of |x| [C, H], members k [C]) in float64"""
    x = np.asarray(x, dtype=np.float64)
    uniq, cons = np.unique(np.asarray(labels), return_inverse=True)
    total = np.zeros((len(uniq), x.shape[1]))
    mass = np.zeros_like(total)
    np.add.at(total, cons, x)
    np.add.at(mass, cons, np.abs(x))
    return cons, total, mass, np.bincount(cons, minlength=len(uniq))


def sum_bound(mass, k):
    return (k[:, None] + 2.0) * U * mass


def mean_bound(mass, k):
    return sum_bound(mass, k) / k[:, None]


def ref_pooled_edges(cons, n_clusters, edge_index, edge_attr):
    """(index [2, E1], float64 sums [E1], addends k [E1], sum of |w| [E1]) of pool_edge: both ends relabelled, self loops
    dropped, the rest sorted by (row, col) with duplicates merged and their attributes summed"""
    ei = np.asarray(edge_index)
    r, c = cons[ei[0]], cons[ei[1]]
    keep = r != c
    ukey, slot = np.unique(r[keep] * n_clusters + c[keep], return_inverse=True)
    index = np.stack([ukey // n_clusters, ukey % n_clusters])
    if edge_attr is None:
        return index, None, np.bincount(slot, minlength=len(ukey)), None
    w = np.asarray(edge_attr, dtype=np.float64).reshape(-1)[keep]
    total = np.zeros(len(ukey))
    mass = np.zeros(len(ukey))
    np.add.at(total, slot, w)
    np.add.at(mass, slot, np.abs(w))
    return index, total, np.bincount(slot, minlength=len(ukey)), mass


def edge_bound(total, k, mass, wmax):
    """``wmax``: the largest |w| of the pooled edge's graph (float32 values)"""
    ex = np.frexp(np.asarray(wmax, dtype=np.float32))[1].astype(np.float64)
    return U * np.abs(total) + (1.0 + U) * k * np.exp2(ex - 41.0) + k * 2.0 ** -52 * mass


def _ratio(what, err, bound):
    """asserts err <= bound element by element; prints and returns the worst err / bound"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert err.shape == bound.shape, (what, err.shape, bound.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    worst = float(ratio.max()) if ratio.size else 0.0
    print("POOL ratio %-44s %.4f (%d elements)" % (what, worst, err.size))
    assert not np.isnan(err).any() and worst <= 1.0, "%s: error / bound = %r" % (what, worst)
    return worst


# ---- inputs -------------------------------------------------------------------------------------------------------
def gapped_labels(rng, n, spread=None):
    """n labels ``randint(0, n // 3 + 1) * 3 + 5``: gapped and offset; about n / 3 clusters (``spread``: the range drawn from)"""
    return rng.integers(0, (n // 3 + 1) if spread is None else spread, size=n) * 3 + 5


def _edges(rng, n, pairs):
    """symmetric random edges with duplicates and self loops: [2, E], [E, 1]"""
    if n < 2 or pairs == 0:
        ei = np.zeros((2, 0), dtype=np.int64)
    else:
        p = rng.integers(0, n, size=(pairs, 2))
        p = np.concatenate([p, p[:5]])                                      # duplicates
        p[1] = [n // 2, n // 2]                                             # self loops
        p[2] = [n - 1, n - 1]
        ei = np.ascontiguousarray(np.concatenate([p, p[:, ::-1]]).T)
    w = rng.uniform(0.1, 2.0, size=(ei.shape[1], 1)).astype(np.float32)
    tiny = rng.random(ei.shape[1]) < 0.05                                   # addends the fixed point has to round
    w[tiny] *= np.float32(1e-7)
    return torch.from_numpy(ei), torch.from_numpy(w)


@functools.lru_cache(maxsize=None)
def ragged(variant):
    """The ragged batch of NODES, on the CPU (callers must not modify it).  x [N, 200] (use the first H columns) with about
    20 % of the rows exactly 0, one row of -inf (node ``p``) and one NaN (node ``q``, channel 0); p and q form a cluster of their
    own, so its channel 0 has no candidate but -inf and NaN.  Labels (``cluster``: made batch-global by the oracle's
    get_preloaded_cluster) by ``variant``:
      random   every graph: gapped_labels (about 500 clusters in the large graph)
      shapes   graph 1: singletons, without edges; graph 2: ONE cluster (its pooled graph has no edge); the large graph:
               about 1200 distinct labels (more clusters than lanes)
    Graph 0 (one node) has no edges in either."""
    rng = np.random.default_rng({"random": 11, "shapes": 12}[variant])
    graphs, local = [], []
    for g, n in enumerate(NODES):
        lab = gapped_labels(rng, n)
        pairs = 2 * n
        if variant == "shapes":
            if g == 1:
                lab = np.arange(n) * 3 + 5
                pairs = 0
            elif g == 2:
                lab = np.full(n, 5)
            elif g == BIG:
                lab = gapped_labels(rng, n, spread=3500)
        x = rng.standard_normal((n, max(WIDTHS))).astype(np.float32)
        x[rng.random(n) < 0.2] = 0.0
        if g == BIG:
            p, q = 700, 900
            lab[[p, q]] = 6                                                 # (every other label is 2 mod 3)
            x[p] = -np.inf
            x[q, 0] = np.nan
        ei, ea = _edges(rng, n, pairs)
        iei, iea = _edges(rng, n, pairs // 2)
        graphs.append(Data(x=torch.from_numpy(x), edge_index=ei, edge_attr=ea,
                           pos=torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)),
                           internal_edge_index=iei, internal_edge_attr=iea))
        local.append(torch.from_numpy(lab))
    b = Batch.from_data_list(graphs)
    cluster = cpu_ref.get_preloaded_cluster(torch.cat(local), b.batch)
    n0 = sum(NODES[:BIG])
    return types.SimpleNamespace(batch=b, cluster=cluster, p=n0 + 700, q=n0 + 900)


@functools.lru_cache(maxsize=None)
def _max_reference(variant, width):
    r = ragged(variant)
    return ref_max(r.batch.x[:, :width].numpy(), r.cluster.numpy())


def _data(r, width, device):
    b = r.batch.clone()
    b.x = b.x[:, :width].contiguous()
    return b.to(device)


def _expected_grad(arg, wgt, n):
    """wgt [C, H] scattered to the arg-max rows (every (row, channel) is the arg-max of at most one cluster)"""
    g = np.zeros((n, arg.shape[1]), dtype=np.float32)
    c, h = np.nonzero(arg < n)
    g[arg[c, h], h] = wgt[c, h]
    return g


# ---- 1. cluster max / mean ----------------------------------------------------------------------------------------
def check_cluster_max(device, variant, width, api=None):
    """community_pooling and max_pool_x on the ragged batch: maxima, arg-max (through the gradient), batch vectors and shapes
    exactly; the gradient of sum(pooled.x * wgt) is wgt at the reference's arg-max rows and 0 elsewhere, exactly."""
    r = ragged(variant)
    cons, want, arg = _max_reference(variant, width)
    n, n_clusters = r.cluster.numel(), want.shape[0]
    if variant == "random" and width == WIDTHS[0]:
        # what the inputs were built to contain
        cell = cons[r.p]
        assert cons[r.q] == cell and (cons == cell).sum() == 2 and arg[cell, 0] == n and want[cell, 0] == 0.0
        ties = 0
        for c in range(n_clusters):
            col = r.batch.x[cons == c, 0].numpy()
            ties += int((col == want[c, 0]).sum() > 1)
        assert ties > 10, ties
    perm = cpu_ref.consecutive_cluster(r.cluster)[1]
    want_batch = r.batch.batch[perm].numpy()
    wgt = np.random.default_rng(5).standard_normal(want.shape).astype(np.float32)
    want_grad = _expected_grad(arg, wgt, n)
    with using(api):
        for through in ("community_pooling", "max_pool_x", "max_pool_x without graph 2"):
            d = _data(r, width, device)
            x = d.x.requires_grad_(True)
            cluster, bvec, wb = r.cluster.to(device), d.batch, want_batch
            if through == "community_pooling":
                pooled = cp.community_pooling(cluster, d)
                got, got_batch = pooled.x, pooled.batch
                assert pooled.num_graphs == len(NODES)
            else:
                if through != "max_pool_x":                                  # an EMPTY graph in the middle of the batch
                    bvec = bvec + (bvec >= 2).to(bvec.dtype)
                    wb = want_batch + (want_batch >= 2)
                got, got_batch = cp.max_pool_x(cluster, x, bvec)
            assert got.shape == (n_clusters, width) and got.dtype == torch.float32, through
            np.testing.assert_array_equal(got.detach().cpu().numpy(), want, err_msg=through)
            assert got_batch.dtype == torch.int64 and got_batch.shape == (n_clusters,)
            np.testing.assert_array_equal(got_batch.cpu().numpy(), wb, err_msg=through)
            (got * torch.from_numpy(wgt).to(device)).sum().backward()
            np.testing.assert_array_equal(x.grad.cpu().numpy(), want_grad, err_msg=through)


def check_scatter_on_ragged(device, width, api=None):
    """scatter_max / scatter_sum / scatter_mean with the ragged batch's labels as ONE index vector of 1630 entries: the compact
    result (dim_size = number of distinct ids) and the dense one (absent ids: rows of 0, arg = N)."""
    r = ragged("random")
    cons, want, arg = _max_reference("random", width)
    n, n_clusters = r.cluster.numel(), want.shape[0]
    clean = np.random.default_rng(21).standard_normal((n, width)).astype(np.float32)
    clean[np.random.default_rng(22).random(n) < 0.2] = 0.0
    _, total, mass, k = ref_sums(clean, r.cluster.numpy())
    ids = np.unique(r.cluster.numpy())
    with using(api):
        index = r.cluster.to(device)
        x = r.batch.x[:, :width].contiguous().to(device)
        got, got_arg = cp.scatter_max(x, index, dim=0, dim_size=n_clusters)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        np.testing.assert_array_equal(got_arg.cpu().numpy(), arg)
        got, got_arg = cp.scatter_max(x, index, dim=0)
        rows = int(ids[-1]) + 1
        dense, dense_arg = np.zeros((rows, width), dtype=np.float32), np.full((rows, width), n, dtype=np.int64)
        dense[ids], dense_arg[ids] = want, arg
        np.testing.assert_array_equal(got.cpu().numpy(), dense)
        np.testing.assert_array_equal(got_arg.cpu().numpy(), dense_arg)
        src = torch.from_numpy(clean).to(device)
        got = cp.scatter_sum(src, index, dim=0, dim_size=n_clusters).cpu().numpy()
        assert got.shape == total.shape
        worst = _ratio("scatter_sum ragged H=%d" % width, np.abs(got - total), sum_bound(mass, k))
        got = cp.scatter_mean(src, index, dim=0, dim_size=n_clusters).cpu().numpy()
        assert got.shape == total.shape
        worst = max(worst, _ratio("scatter_mean ragged H=%d" % width, np.abs(got - total / k[:, None]), mean_bound(mass, k)))
        dense = cp.scatter_mean(src, index, dim=0).cpu().numpy()
        assert dense.shape == (rows, width) and not dense[np.setdiff1d(np.arange(rows), ids)].any()
        np.testing.assert_array_equal(dense[ids], got)
    return worst


# ---- 2. pooled edges, mean positions ------------------------------------------------------------------------------
def _check_pooled_edges(what, got_index, got_attr, cons, n_clusters, edge_index, edge_attr, cluster_graph, edge_graph):
    """edge_index == cpu_ref.pool_edge exactly (and == the numpy restatement); edge_attr within edge_bound of the float64 sums"""
    pei, _ = cpu_ref.pool_edge(torch.from_numpy(cons), edge_index, edge_attr)
    index, total, k, mass = ref_pooled_edges(cons, n_clusters, edge_index.numpy(), edge_attr.numpy())
    np.testing.assert_array_equal(pei.numpy().reshape(2, -1), index, err_msg=what)
    assert got_index.dtype == torch.int64 and tuple(got_index.shape) == index.shape, (what, tuple(got_index.shape), index.shape)
    np.testing.assert_array_equal(got_index.cpu().numpy(), index, err_msg=what)
    assert tuple(got_attr.shape) == (index.shape[1], 1), what
    w = np.abs(edge_attr.numpy().reshape(-1)).astype(np.float64)
    wmax = np.zeros(int(cluster_graph.max()) + 1)
    np.maximum.at(wmax, edge_graph, w)                                      # the largest |w| of every graph: ALL its edges
    bound = edge_bound(total, k, mass, wmax[cluster_graph[index[0]]])
    return _ratio(what, np.abs(got_attr.cpu().numpy().reshape(-1).astype(np.float64) - total), bound), index


def check_pooled_edges(device, variant, api=None):
    """community_pooling on the ragged batch: pooled edge_index / edge_attr, the internal_edge_* path and the mean positions"""
    r = ragged(variant)
    b = r.batch
    cons, _, _ = _max_reference(variant, 1)
    n_clusters = int(cons.max()) + 1
    perm = cpu_ref.consecutive_cluster(r.cluster)[1]
    cluster_graph = b.batch[perm].numpy()
    with using(api):
        pooled = cp.community_pooling(r.cluster.to(device), _data(r, 1, device))
    worst, index = _check_pooled_edges("edge_attr %s" % variant, pooled.edge_index, pooled.edge_attr, cons, n_clusters,
                                       b.edge_index, b.edge_attr, cluster_graph, b.batch[b.edge_index[0]].numpy())
    w2, _ = _check_pooled_edges("internal_edge_attr %s" % variant, pooled.internal_edge_index, pooled.internal_edge_attr, cons,
                                n_clusters, b.internal_edge_index, b.internal_edge_attr, cluster_graph,
                                b.batch[b.internal_edge_index[0]].numpy())
    per_graph = np.bincount(cluster_graph[index[0]], minlength=len(NODES))
    assert per_graph[0] == 0 and per_graph[BIG] > 0                        # the one-node graph has no edge to pool
    if variant == "shapes":
        assert per_graph[2] == 0 and (cluster_graph == 2).sum() == 1       # one cluster: every edge falls inside it
        assert per_graph[1] == 0 and (cluster_graph == 1).sum() == NODES[1]
        assert (cluster_graph == BIG).sum() > 1024                          # more clusters than lanes in one graph
    _, total, mass, k = ref_sums(b.pos.numpy(), r.cluster.numpy())
    got = pooled.pos.cpu().numpy()
    assert got.shape == total.shape and got.dtype == np.float32
    w3 = _ratio("pos %s" % variant, np.abs(got - total / k[:, None]), mean_bound(mass, k))
    return max(worst, w2, w3)


def check_plain_data(device, api=None):
    """a plain Data (no batch vector) pools to a Data; the pos2D path, which only that branch takes"""
    rng = np.random.default_rng(31)
    n = 1500
    ei, ea = _edges(rng, n, 2 * n)
    lab = torch.from_numpy(gapped_labels(rng, n))
    x = torch.from_numpy(rng.standard_normal((n, 7)).astype(np.float32))
    pos = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
    pos2d = torch.from_numpy(rng.standard_normal((n, 2)).astype(np.float32))
    d = Data(x=x, edge_index=ei, edge_attr=ea, pos=pos, pos2D=pos2d).to(device)
    with using(api):
        pooled = cp.community_pooling(lab.to(device), d)
    assert isinstance(pooled, Data) and not isinstance(pooled, Batch)
    cons, want, _ = ref_max(x.numpy(), lab.numpy())
    np.testing.assert_array_equal(pooled.x.cpu().numpy(), want)
    graph = np.zeros(want.shape[0], dtype=np.int64)
    worst, _ = _check_pooled_edges("edge_attr plain Data", pooled.edge_index, pooled.edge_attr, cons, want.shape[0], ei, ea, graph,
                                   np.zeros(ei.size(1), dtype=np.int64))
    for name, src, got in (("pos", pos, pooled.pos), ("pos2D", pos2d, pooled.pos2D)):
        _, total, mass, k = ref_sums(src.numpy(), lab.numpy())
        assert tuple(got.shape) == total.shape
        worst = max(worst, _ratio("%s plain Data" % name, np.abs(got.cpu().numpy() - total / k[:, None]), mean_bound(mass, k)))
    return worst


# ---- 3. get_preloaded_cluster -------------------------------------------------------------------------------------
PRELOADED_NODES = (1, 64, 2500, 65)          # (2500 nodes: three trips of the 1024-lane loop)
PRELOADED_CASES = [("first", 0), ("lane63", 0), ("beyond2048", 0), ("last", 0), ("beyond2048", 10 ** 11)]


def check_preloaded_cluster(device, where, shift, api=None):
    """every graph's largest label at one position (index 0, the last lane of the first wave, an index of the third trip, the
    last node; clipped to the graph), labels with gaps, optionally shifted beyond 32 bits: == the oracle exactly, in place.
    (Every graph has a node: with an empty graph in the middle the oracle itself raises, as the reference's loop would.)"""
    rng = np.random.default_rng(41)
    labels, batch = [], []
    for g, n in enumerate(PRELOADED_NODES):
        lab = gapped_labels(rng, n)
        at = {"first": 0, "lane63": min(63, n - 1), "beyond2048": min(2100, n - 1), "last": n - 1}[where]
        lab[at] = lab.max() + 7
        assert (lab == lab.max()).sum() == 1 and lab.argmax() == at
        labels.append(lab + shift)
        batch.append(np.full(n, g))
    cluster = torch.from_numpy(np.concatenate(labels))
    batch = torch.from_numpy(np.concatenate(batch))
    want = cpu_ref.get_preloaded_cluster(cluster.clone(), batch)
    with using(api):
        mine = cluster.clone().to(device)
        ret = cp.get_preloaded_cluster(mine, batch.to(device))
    assert ret is mine
    np.testing.assert_array_equal(mine.cpu().numpy(), want.numpy())
    assert shift == 0 or int(want.max()) > 2 ** 33


# ---- 5. scatter_* at size -----------------------------------------------------------------------------------------
SCATTER_CASES = {"dense700": (20000, 700, 1), "sparse50": (5000, 50, 1000003)}


@functools.lru_cache(maxsize=None)
def _scatter_case(name):
    n, ids, stride = SCATTER_CASES[name]
    rng = np.random.default_rng(n)
    index = rng.integers(0, ids, size=n) * stride
    src = rng.standard_normal((n, 5)).astype(np.float32)
    src[rng.random(n) < 0.2] = 0.0
    return index, src, ref_max(src, index), ref_sums(src, index)


def check_scatter_at_size(device, name, api=None):
    """20 000 entries over 700 ids (presence flags, 20 trips) and 5 000 entries over 50 ids that are 1 000 003 apart (the
    rank-sort branch of wg_cluster_rank); dim_size = the number of distinct ids, so the result stays compact"""
    index, src, (_, want, arg), (_, total, mass, k) = _scatter_case(name)
    with using(api):
        idx, x = torch.from_numpy(index).to(device), torch.from_numpy(src).to(device)
        dim_size = int(torch.unique(idx).numel())
        assert dim_size == want.shape[0]
        got, got_arg = cp.scatter_max(x, idx, dim=0, dim_size=dim_size)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        np.testing.assert_array_equal(got_arg.cpu().numpy(), arg)
        got = cp.scatter_sum(x, idx, dim=0, dim_size=dim_size).cpu().numpy()
        assert got.shape == total.shape
        worst = _ratio("scatter_sum %s" % name, np.abs(got - total), sum_bound(mass, k))
        got = cp.scatter_mean(x, idx, dim=0, dim_size=dim_size).cpu().numpy()
        assert got.shape == total.shape
        return max(worst, _ratio("scatter_mean %s" % name, np.abs(got - total / k[:, None]), mean_bound(mass, k)))


# ---- the two references against each other, on the pinned fixture ------------------------------------------------------
def check_references_on_fixture():
    """ref_max / ref_sums / ref_pooled_edges == oracle/cpu_ref.py on the fixture batch (with a NaN, a row of -inf and rows of
    zeros planted), whose pooling test_oracle_golden.py pins on the reference's own vectors"""
    from helpers import fixture_batch
    b = fixture_batch(8)
    cluster = cpu_ref.get_preloaded_cluster(b.cluster0.clone(), b.batch)
    x = b.x.clone()
    x[::5] = 0.0
    x[3] = -np.inf
    x[4, 2] = np.nan
    cons, want, arg = ref_max(x.numpy(), cluster.numpy())
    oc, _ = cpu_ref.consecutive_cluster(cluster)
    np.testing.assert_array_equal(cons, oc.numpy())
    om, oa = cpu_ref.scatter_max(x, oc)
    np.testing.assert_array_equal(want, om.numpy())
    np.testing.assert_array_equal(arg, oa.numpy())
    _, total, mass, k = ref_sums(b.pos.numpy(), cluster.numpy())
    np.testing.assert_allclose(total / k[:, None], cpu_ref.scatter_mean(b.pos.double(), oc).numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(total, cpu_ref.scatter_sum(b.pos.double(), oc).numpy(), rtol=1e-13, atol=1e-13)
    for ei, ea in ((b.edge_index, b.edge_attr), (b.internal_edge_index, getattr(b, "internal_edge_attr", None))):
        index, tot, _, _ = ref_pooled_edges(cons, want.shape[0], ei.numpy(), None if ea is None else ea.numpy())
        pei, pea = cpu_ref.pool_edge(oc, ei, None if ea is None else ea.double())
        np.testing.assert_array_equal(index, pei.numpy().reshape(2, -1))
        if ea is not None:
            np.testing.assert_allclose(tot, pea.numpy().reshape(-1), rtol=1e-13, atol=1e-13)
