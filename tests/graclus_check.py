"""graclus / normalized_cut / max_pool (README custom-net recipe) against oracle/graclus_ref.py and structural
properties.  Shared by the emulated (CPU) and the MI355X test."""
import numpy as np
import torch
import torch.nn.functional as F

import deeprank_gnn_amd.community_pooling as cp
from deeprank_gnn_amd.data import Batch, Data
from deeprank_gnn_amd.ginet import GINetConvLayer
from elementwise import assert_arbiter_rate, check, new_stats
from oracle import cpu_ref, graclus_ref


def random_graphs(seed, count=5):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(1, 40))
        m = int(rng.integers(0, 3 * n))
        pairs = rng.integers(0, n, size=(m, 2))
        if k == 1 and m:
            pairs[0] = [0, 0]                                       # a self loop
        ei = np.concatenate([pairs, pairs[:, ::-1]], axis=0).T      # symmetric, like the loader's edge_index
        g = Data(x=torch.from_numpy(rng.standard_normal((n, 6)).astype(np.float32)),
                 edge_index=torch.from_numpy(np.ascontiguousarray(ei)).long(),
                 edge_attr=torch.from_numpy(rng.uniform(0.1, 2.0, (2 * m, 1)).astype(np.float32)),
                 pos=torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)))
        out.append(g)
    return out


def check_graclus(device, api=None, seed=0):
    cp._API = api
    try:
        rng = np.random.default_rng(seed)
        graphs = random_graphs(seed)
        for weighted in (False, True):
            for use_perm in (False, True):
                # one graph at a time against the oracle
                for g in graphs:
                    n = g.x.size(0)
                    perm = rng.permutation(n) if use_perm else None
                    w = g.edge_attr.reshape(-1) if weighted else None
                    want = graclus_ref.graclus(g.edge_index.numpy(), None if w is None else w.numpy(), n, perm)
                    got = cp.graclus(g.edge_index.to(device), None if w is None else w.to(device), n,
                                     perm=None if perm is None else torch.from_numpy(perm).to(device))
                    assert got.cpu().tolist() == want.tolist()
                    _properties(g.edge_index.numpy(), want, n)
                # the block-diagonal batch, split by `batch`: per-graph labels shifted by the node offsets
                b = Batch.from_data_list(graphs)
                perms = [rng.permutation(g.x.size(0)) for g in graphs] if use_perm else None
                w = b.edge_attr.reshape(-1) if weighted else None
                got = cp.graclus(b.edge_index.to(device), None if w is None else w.to(device), perm=None if perms is None
                                 else torch.from_numpy(np.concatenate(perms)).to(device), batch=b.batch.to(device))
                want, off = [], 0
                for i, g in enumerate(graphs):
                    n = g.x.size(0)
                    lab = graclus_ref.graclus(g.edge_index.numpy(), g.edge_attr.reshape(-1).numpy() if weighted else None,
                                              n, None if perms is None else perms[i])
                    want += (lab + off).tolist()
                    off += n
                assert got.cpu().tolist() == want
        # normalized_cut
        g = graphs[0]
        nc = cp.normalized_cut(g.edge_index.to(device), g.edge_attr.to(device), g.x.size(0))
        np.testing.assert_allclose(nc.cpu().numpy(), graclus_ref.normalized_cut(g.edge_index.numpy(), g.edge_attr.numpy(),
                                                                              g.x.size(0)), rtol=1e-6)
    finally:
        cp._API = None


def _properties(edge_index, labels, n):
    """A maximal matching: clusters of size <= 2, pairs are adjacent, no edge joins two singletons."""
    members = {}
    for i, l in enumerate(labels.tolist()):
        members.setdefault(l, []).append(i)
    adj = {(int(a), int(b)) for a, b in zip(edge_index[0], edge_index[1]) if a != b}
    single = set()
    for l, m in members.items():
        assert len(m) <= 2 and l == min(m)
        if len(m) == 2:
            assert (m[0], m[1]) in adj or (m[1], m[0]) in adj
        else:
            single.add(m[0])
    for a, b in adj:
        assert not (a in single and b in single)


LDS_LIMIT = 160 * 1024          # DRGNN_LDS_LIMIT of csrc/drgnn_capi_common.h: the largest carve drgnn_graclus accepts


def carve_bytes(n, e):
    """drgnn_graclus's LDS carve for a batch whose largest graph has n nodes and e (directed) edges: (N + 1) row pointers,
    E columns, E weights, N labels, 4 bytes each"""
    return 4 * ((n + 1) + 2 * e + n)


def large_graph(variant="plain", n=1000, n_pairs=4000, seed=7):
    """(edge_index [2, 2 n_pairs], pairs): random pairs listed in both directions; ``variant`` "loops": a self loop and a
    duplicated pair among them (the edge count stays)"""
    rng = np.random.default_rng(seed)
    pairs = rng.integers(0, n, size=(n_pairs, 2))
    if variant == "loops":
        pairs[0] = [5, 5]
        pairs[2] = pairs[1]
    return np.ascontiguousarray(np.concatenate([pairs, pairs[:, ::-1]], axis=0).T)


def _batched(small, ei, n):
    """the large graph between two small ones, block-diagonal: (edge_index, batch, [(edge_index, n) per graph])"""
    parts = [(small[0].edge_index.numpy(), small[0].x.size(0)), (ei, n), (small[1].edge_index.numpy(), small[1].x.size(0))]
    off, eis, bvec = 0, [], []
    for g, (e, k) in enumerate(parts):
        eis.append(e + off)
        bvec.append(np.full(k, g))
        off += k
    return np.concatenate(eis, axis=1), np.concatenate(bvec), parts


def check_graclus_large(device, api=None):
    """A graph of 1 000 nodes and 8 000 directed edges between two small ones: its carve, (N + 1) + 2 E + N = 18 001 words =
    72 004 bytes, is beyond the 64 KiB a kernel gets without asking (the device build raises its dynamic-LDS attribute).
    Weights rounded to one decimal (long runs of ties: the first in edge order wins), normalized_cut of unit attributes,
    no weights, a permutation, a self loop and a duplicated pair: labels == oracle/graclus_ref.py exactly, alone and
    in the batch, and a maximal matching; a second run gives the same labels."""
    cp._API = api
    try:
        n = 1000
        assert carve_bytes(n, 8000) == 72004 > 64 * 1024
        rng = np.random.default_rng(17)
        small = random_graphs(5, count=2)
        for variant, weights, use_perm in (("plain", "rounded", False), ("plain", "cut", False), ("plain", None, False),
                                           ("plain", "rounded", True), ("loops", "rounded", False), ("loops", None, True)):
            ei = large_graph(variant)
            assert ei.shape == (2, 8000)
            t_ei = torch.from_numpy(ei).to(device)
            if weights == "rounded":
                w = np.round(rng.uniform(0.1, 2.0, ei.shape[1]), 1).astype(np.float32)
                assert len(np.unique(w)) <= 20
            elif weights == "cut":
                # the oracle matches on the weights the function under test returned (it is compared with the oracle's own
                # below): where two correctly rounded divisions could differ in the last bit, the ties would move
                w = cp.normalized_cut(t_ei, torch.ones(ei.shape[1], 1, device=device), n).cpu().numpy()
                np.testing.assert_allclose(w, graclus_ref.normalized_cut(ei, np.ones(ei.shape[1], np.float32), n), rtol=1e-6)
            else:
                w = None
            perm = rng.permutation(n) if use_perm else None
            want = graclus_ref.graclus(ei, w, n, perm)
            _properties(ei, want, n)
            assert w is None or (np.bincount(want, minlength=n) == 2).sum() > 300      # (a matching worth the name)
            t_w = None if w is None else torch.from_numpy(w).to(device)
            t_perm = None if perm is None else torch.from_numpy(perm).to(device)
            got = cp.graclus(t_ei, t_w, n, perm=t_perm)
            assert got.dtype == torch.int64 and got.cpu().tolist() == want.tolist(), (variant, weights, use_perm)
            again = cp.graclus(t_ei, t_w, n, perm=t_perm)
            assert torch.equal(got, again)
            # ... and between two small graphs
            bei, bvec, parts = _batched(small, ei, n)
            bw = None if w is None else np.concatenate([small[0].edge_attr.reshape(-1).numpy(), w,
                                                        small[1].edge_attr.reshape(-1).numpy()])
            perms = None if perm is None else [rng.permutation(parts[0][1]), perm, rng.permutation(parts[2][1])]
            got = cp.graclus(torch.from_numpy(bei).to(device), None if bw is None else torch.from_numpy(bw).to(device),
                             perm=None if perms is None else torch.from_numpy(np.concatenate(perms)).to(device),
                             batch=torch.from_numpy(bvec).to(device))
            wanted, off, eoff = [], 0, 0
            for g, (e, k) in enumerate(parts):
                lab = graclus_ref.graclus(e, None if bw is None else bw[eoff:eoff + e.shape[1]], k,
                                          None if perms is None else perms[g])
                wanted += (lab + off).tolist()
                off += k
                eoff += e.shape[1]
            assert got.cpu().tolist() == wanted, (variant, weights, use_perm, "batched")
    finally:
        cp._API = None


def check_graclus_carve_limit(device, api=None):
    """The largest carve drgnn_graclus accepts for a graph of 1 024 nodes, and one edge more: the first == the oracle, the
    second is refused with DrgnnError "capacity" before anything is launched (the output keeps what it held)."""
    import types
    import pytest
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.topology import Topology
    api_ = api or _lib.get()
    cp._API = api
    try:
        n = 1024
        e_fit = (LDS_LIMIT // 4 - (2 * n + 1)) // 2
        assert carve_bytes(n, e_fit) <= LDS_LIMIT < carve_bytes(n, e_fit + 1)
        assert e_fit % 2 == 1                                          # pairs in both directions and one self loop
        rng = np.random.default_rng(23)
        pairs = rng.integers(0, n, size=((e_fit + 1) // 2, 2))
        over = np.ascontiguousarray(np.concatenate([pairs, pairs[:, ::-1]], axis=0).T)
        fit = np.ascontiguousarray(np.concatenate([over[:, :-2], [[9], [9]]], axis=1))
        assert fit.shape[1] == e_fit and over.shape[1] == e_fit + 1
        w = np.round(rng.uniform(0.1, 2.0, e_fit), 1).astype(np.float32)
        want = graclus_ref.graclus(fit, w, n)
        _properties(fit, want, n)
        got = cp.graclus(torch.from_numpy(fit).to(device), torch.from_numpy(w).to(device), n)
        assert got.cpu().tolist() == want.tolist()
        # one edge more
        t_over = torch.from_numpy(over).to(device)
        with pytest.raises(_lib.DrgnnError, match="capacity"):
            cp.graclus(t_over, None, n)
        s = types.SimpleNamespace(edge_index=t_over, edge_attr=None, cluster0=None, cluster1=None,
                                  batch=torch.zeros(n, dtype=torch.int64, device=device))
        s.__dict__["_num_graphs"] = 1
        topo = Topology.from_batch(s, api=api_, with_level1=False, graph_only=True, need_weights=False)
        topo.check()
        assert (topo.max_nodes, topo.max_edges) == (n, e_fit + 1)
        out = torch.full((n,), -7, dtype=torch.int64, device=device)
        with pytest.raises(_lib.DrgnnError, match="capacity"):
            api_.graclus(topo.ws_i32, n, topo.n_edges, topo.n_graphs, topo.max_nodes, topo.max_edges, None, None, out,
                         _lib.current_stream(out))
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()
        assert bool((out == -7).all())
    finally:
        cp._API = None


def _recipe_oracle(dtype, hb, weights, cluster, cluster2, wgt):
    """(out, grad conv1.fc.weight, grad conv2.fc.weight) of conv -> relu -> max_pool -> conv -> relu -> max_pool_x -> mean in
    ``dtype`` on the CPU: oracle/cpu_ref.py's layer and pooling functions on the labels the code under test produced"""
    leaves = [w.detach().cpu().clone().to(dtype).requires_grad_(i % 3 == 0) for i, w in enumerate(weights)]
    x1 = F.relu(cpu_ref.ginet_conv(hb.x.to(dtype), hb.edge_index, hb.edge_attr.to(dtype), *leaves[:3]))
    cons, perm = cpu_ref.consecutive_cluster(cluster)
    xp, _ = cpu_ref.scatter_max(x1, cons)
    pei, pea = cpu_ref.pool_edge(cons, hb.edge_index, hb.edge_attr.to(dtype))
    pbatch = hb.batch[perm]
    x2 = F.relu(cpu_ref.ginet_conv(xp, pei, pea, *leaves[3:]))
    cons2, perm2 = cpu_ref.consecutive_cluster(cluster2)
    x3, _ = cpu_ref.scatter_max(x2, cons2)
    out = cpu_ref.scatter_mean(x3, pbatch[perm2])
    (out * wgt.to(dtype)).sum().backward()
    return [out.detach().numpy(), leaves[0].grad.numpy(), leaves[3].grad.numpy()], pei


def check_custom_net_recipe(device, api=None):
    """The README pipeline: normalized_cut -> graclus -> max_pool -> ... -> graclus -> max_pool_x -> scatter_mean, on a
    batch; max_pool against a plain torch restatement of the PyG pooling (unique / amax / coalesce-add) on the same labels.
    Then the same pipeline with a GINetConvLayer (and a ReLU) before each pooling: the final scatter_mean and the gradients of
    both layers' fc.weight against the pipeline restated with oracle/cpu_ref.py (ginet_conv, the oracle pooling on the labels
    the code under test produced, the mean) under tests/elementwise.py's rule, the float64 pipeline as its arbiter."""
    cp._API = api
    try:
        graphs = random_graphs(3, count=4)
        b = Batch.from_data_list(graphs).to(device)
        w = cp.normalized_cut(b.edge_index, b.edge_attr, b.x.size(0))
        cluster = cp.graclus(b.edge_index, w, b.x.size(0), batch=b.batch)
        pooled = cp.max_pool(cluster, b)
        # oracle pooling of the same labels
        hb = Batch.from_data_list(graphs)
        uniq, inv = torch.unique(cluster.cpu(), return_inverse=True)
        x_ref = torch.full((uniq.numel(), hb.x.size(1)), float("-inf"))
        x_ref = x_ref.scatter_reduce(0, inv[:, None].expand(-1, hb.x.size(1)), hb.x, reduce="amax")
        assert torch.equal(pooled.x.cpu(), x_ref)
        r, c = inv[hb.edge_index[0]], inv[hb.edge_index[1]]
        keep = r != c
        key = r[keep] * uniq.numel() + c[keep]
        ukey, kinv = torch.unique(key, return_inverse=True)
        attr = torch.zeros(ukey.numel()).index_add_(0, kinv, hb.edge_attr.reshape(-1)[keep])
        assert torch.equal(pooled.edge_index.cpu(), torch.stack([ukey // uniq.numel(), ukey % uniq.numel()]))
        np.testing.assert_allclose(pooled.edge_attr.cpu().reshape(-1).numpy(), attr.numpy(), rtol=1e-6)
        first = torch.zeros(uniq.numel(), dtype=torch.long).scatter_reduce(0, inv, hb.batch, reduce="amin", include_self=False)
        assert torch.equal(pooled.batch.cpu(), first)
        # second level
        w2 = cp.normalized_cut(pooled.edge_index, pooled.edge_attr, pooled.x.size(0))
        cluster2 = cp.graclus(pooled.edge_index, w2, pooled.x.size(0), batch=pooled.batch)
        x2, batch2 = cp.max_pool_x(cluster2, pooled.x, pooled.batch)
        out = cp.scatter_mean(x2, batch2, dim=0)
        assert out.shape == (4, 6) and torch.isfinite(out).all()
        # with a conv layer before each pooling, against the oracle's pipeline
        torch.manual_seed(9)
        conv1, conv2 = GINetConvLayer(6, 8, 1).to(device), GINetConvLayer(8, 10, 1).to(device)
        d = b.clone()
        d.x = F.relu(conv1(b.x, b.edge_index, b.edge_attr))
        pooled = cp.max_pool(cluster, d)
        x2 = F.relu(conv2(pooled.x, pooled.edge_index, pooled.edge_attr))
        w2 = cp.normalized_cut(pooled.edge_index, pooled.edge_attr, pooled.x.size(0))
        cluster2 = cp.graclus(pooled.edge_index, w2, pooled.x.size(0), batch=pooled.batch)
        x3, batch3 = cp.max_pool_x(cluster2, x2, pooled.batch)
        out = cp.scatter_mean(x3, batch3, dim=0)
        assert out.shape == (4, 10)
        wgt = torch.from_numpy(np.random.default_rng(4).standard_normal((4, 10)).astype(np.float32))
        (out * wgt.to(device)).sum().backward()
        weights = [m.weight for c in (conv1, conv2) for m in (c.fc, c.fc_edge_attr, c.fc_attention)]
        labels = (cluster.cpu(), cluster2.cpu())
        ref32, pei = _recipe_oracle(torch.float32, hb, weights, labels[0], labels[1], wgt)
        assert torch.equal(pooled.edge_index.cpu(), pei)           # (cluster2 labels the same pooled graph in both)
        ref64 = []

        def arbiter(i):
            if not ref64:
                ref64.extend(_recipe_oracle(torch.float64, hb, weights, labels[0], labels[1], wgt)[0])
            return ref64[i]
        stats = new_stats()
        got = [out.detach().cpu().numpy(), conv1.fc.weight.grad.cpu().numpy(), conv2.fc.weight.grad.cpu().numpy()]
        for i, name in enumerate(("scatter_mean", "grad conv1.fc.weight", "grad conv2.fc.weight")):
            assert np.abs(ref32[i]).max() > 1e-3, name                      # (not a comparison of zeros)
            check("recipe " + name, got[i], ref32[i], lambda i=i: arbiter(i), stats)
        assert_arbiter_rate(stats, "recipe")
    finally:
        cp._API = None
