"""Offline community detection on the device: the reference's ``PreCluster`` /
``community_detection(..., method='mcl')`` (DataSet.py:45-88, community_pooling.py:95-158) for
whole batches of graphs at once.

The reference runs Markov clustering (package ``markov-clustering``, default parameters) on the
unweighted INTERNAL-contact graph of every complex, pools that graph with the resulting clusters,
clusters the pooled graph again, and stores both label vectors with the dataset
(``clustering/mcl/depth_0`` and ``depth_1``); training only reads them back.  ``precluster`` does the
same for a ``Batch``: one workgroup per graph, dense fp64 (``drgnn_mcl``), pooling through the
topology builder.  Pinned on the fixture's stored labels (all graphs, both depths, exact) and, against
``oracle/mcl_ref.py``, on the named and random graphs of ``tests/mcl_check.py`` (labels and iteration count).
Markov clustering is not a stable function of its input: on symmetric graphs (cycles, for one) rounding
decides ties, so labels and iteration count there depend on the summation order and are only checked to be in
range and the same on every launch.  ``mcl_labels`` returns ``info`` (iterations used, negative when a graph
did not converge within 100), but neither ``precluster`` nor ``PreCluster`` nor ``community_detection`` looks at
it: a graph that did not converge gets the labels of its last iterate, silently.

``method='louvain'`` (the reference's python-louvain ``best_partition``) runs a deterministic Louvain
(``drgnn_louvain``, one 64-lane workgroup per graph, exact int64 arithmetic) through the same pooling path.  It
differs from python-louvain in two deliberate ways: nodes are visited in id order with ties going to the smallest
community id (python-louvain draws random visiting orders), and labels are numbered by first appearance over the
node ids (python-louvain numbers them through a set).  So the same input always gives the same labels.
"""
import types

import torch

from . import _lib
from .topology import Topology

__all__ = ["mcl_labels", "louvain_labels", "precluster", "community_detection_mcl", "community_detection_louvain",
           "PreCluster"]


def _ptr_from_counts(counts, device):
    ptr = torch.zeros(counts.numel() + 1, dtype=torch.int32, device=device)
    ptr[1:] = counts.cumsum(0).to(torch.int32)
    return ptr


def mcl_labels(edge_index, node_ptr, edge_ptr, api=None):
    """Markov clustering of B graphs given as one block-diagonal edge list.
    edge_index int64 [2,E] (global node ids, grouped by graph), node_ptr / edge_ptr int32 [B+1].
    Returns (labels int64 [N], iterations int32 [B])."""
    api = api or _lib.get()
    if api is _lib._API:
        _lib.require_device(edge_index, node_ptr, edge_ptr)
    dev = node_ptr.device
    sizes = (node_ptr[1:] - node_ptr[:-1]).to(torch.int64)
    mat_ptr = torch.zeros(sizes.numel() + 1, dtype=torch.int64, device=dev)
    mat_ptr[1:] = (sizes * sizes).cumsum(0)
    total = int(mat_ptr[-1])                      # offline step: a host sync is fine
    n_nodes = int(node_ptr[-1])
    B = sizes.numel()
    mat = torch.empty(max(3 * total, 1), dtype=torch.float64, device=dev)
    iscr = torch.empty(max(4 * n_nodes, 1), dtype=torch.int32, device=dev)
    labels = torch.zeros(n_nodes, dtype=torch.int64, device=dev)
    info = torch.zeros(max(B, 1), dtype=torch.int32, device=dev)
    edge_index = edge_index.to(torch.int64).contiguous()
    api.mcl(edge_index, edge_index.size(1), node_ptr.contiguous(), edge_ptr.contiguous(), mat_ptr, B, mat, iscr,
            labels, info, _lib.current_stream(labels))
    return labels, info[:B]


def community_detection_mcl(edge_index, num_nodes, api=None):
    """One graph: ``community_detection(edge_index, num_nodes, method='mcl')``."""
    dev = edge_index.device
    node_ptr = torch.tensor([0, num_nodes], dtype=torch.int32, device=dev)
    edge_ptr = torch.tensor([0, edge_index.size(1)], dtype=torch.int32, device=dev)
    return mcl_labels(edge_index, node_ptr, edge_ptr, api=api)[0]


def louvain_labels(edge_index, node_ptr, edge_ptr, api=None):
    """Deterministic Louvain of B graphs given as one block-diagonal edge list (unweighted: each distinct
    pair has weight 1, whatever its direction or repetition).
    edge_index int64 [2,E] (global node ids, grouped by graph), node_ptr / edge_ptr int32 [B+1].
    Returns (labels int64 [N] per-graph local, consecutive in order of first appearance; info int32 [B,2] =
    (recorded levels, total passes); modularity float64 [B]).
    Each graph's slice is first reduced to one entry per unordered pair: the kernel's LDS carve grows with the
    entries of the largest slice, and lists that give every pair in both directions (internal_edge_index) would
    otherwise halve the graph size it takes (1 024 nodes with 4 096 pairs fit either way)."""
    api = api or _lib.get()
    if api is _lib._API:
        _lib.require_device(edge_index, node_ptr, edge_ptr)
    dev = node_ptr.device
    B = node_ptr.numel() - 1
    n_nodes = int(node_ptr[-1])                   # offline step: host syncs are fine
    pairs, edge_ptr = _distinct_pairs(edge_index.to(torch.int64), node_ptr, edge_ptr)
    max_nodes = int((node_ptr[1:] - node_ptr[:-1]).max()) if B > 0 else 0
    max_edges = int((edge_ptr[1:] - edge_ptr[:-1]).max()) if B > 0 else 0
    labels = torch.zeros(n_nodes, dtype=torch.int64, device=dev)
    info = torch.zeros((max(B, 1), 2), dtype=torch.int32, device=dev)
    modularity = torch.zeros(max(B, 1), dtype=torch.float64, device=dev)
    api.louvain(pairs, pairs.size(1), node_ptr.contiguous(), edge_ptr, B, max_nodes, max_edges, labels, info,
                modularity, _lib.current_stream(labels))
    return labels, info[:B], modularity[:B]


def _distinct_pairs(edge_index, node_ptr, edge_ptr):
    """(pairs int64 [2,P] = (min, max) of every distinct unordered pair, grouped by graph; edge_ptr int32 [B+1] of
    them).  An entry with an end outside its own slice's graph is dropped, as the kernel drops it."""
    dev = node_ptr.device
    B = node_ptr.numel() - 1
    n_nodes = int(node_ptr[-1])
    nptr, eptr = node_ptr.to(torch.int64), edge_ptr.to(torch.int64)
    g = torch.searchsorted(eptr[1:], torch.arange(edge_index.size(1), device=dev), right=True)
    u, v = edge_index[0], edge_index[1]
    lo_g, hi_g = nptr[:-1][g], nptr[1:][g]
    keep = (u >= lo_g) & (u < hi_g) & (v >= lo_g) & (v < hi_g)
    lo, hi = torch.minimum(u, v)[keep], torch.maximum(u, v)[keep]
    key = torch.unique(lo * max(n_nodes, 1) + hi)            # sorted: graph by graph, as node ids are
    lo, hi = key // max(n_nodes, 1), key % max(n_nodes, 1)
    counts = torch.bincount(torch.searchsorted(nptr[1:], lo, right=True), minlength=B)
    return torch.stack((lo, hi)).contiguous(), _ptr_from_counts(counts[:B], dev)


def community_detection_louvain(edge_index, num_nodes, api=None):
    """One graph: ``community_detection(edge_index, num_nodes, method='louvain')``."""
    dev = edge_index.device
    node_ptr = torch.tensor([0, num_nodes], dtype=torch.int32, device=dev)
    edge_ptr = torch.tensor([0, edge_index.size(1)], dtype=torch.int32, device=dev)
    return louvain_labels(edge_index, node_ptr, edge_ptr, api=api)[0]


def _labeller(method):
    """mcl_labels or louvain_labels: both return the labels first"""
    labellers = {'mcl': mcl_labels, 'louvain': louvain_labels}
    if method.lower() not in labellers:
        raise ValueError("clustering method %r: 'mcl' or 'louvain'" % (method,))
    return labellers[method.lower()]


def precluster(batch, method='mcl', api=None, with_cluster_ptr=False):
    """(cluster0 [N], cluster1 [sum C0]) of a Batch that carries ``internal_edge_index``: what
    PreCluster would store as clustering/<method>/depth_0 and depth_1 for each of its graphs (per-graph
    local ids, concatenated in graph order).  ``with_cluster_ptr``: also the int32 [B+1] offsets of the graphs'
    depth-0 clusters in cluster1 (the builder's CPTR0), on the device."""
    labeller = _labeller(method)
    api = api or _lib.get()
    iei = batch.internal_edge_index.to(torch.int64).contiguous()
    bvec = batch.batch
    dev = bvec.device
    B = getattr(batch, "num_graphs", None) or (int(bvec.max()) + 1)
    node_ptr = _ptr_from_counts(torch.bincount(bvec, minlength=B), dev)
    edge_ptr = _ptr_from_counts(torch.bincount(bvec[iei[0]], minlength=B), dev)
    d0 = labeller(iei, node_ptr, edge_ptr, api=api)[0]
    # pool the internal-contact graph with depth_0 (community_pooling on internal edges, DataSet.py:81)
    shadow = types.SimpleNamespace(edge_index=iei, edge_attr=None, batch=bvec, cluster0=d0, cluster1=None)
    shadow.__dict__["_num_graphs"] = B
    topo = Topology.from_batch(shadow, api=api, with_level1=False, need_weights=False)
    topo.check()
    c0, e1, _ = topo.totals()
    pooled = torch.empty((2, e1), dtype=torch.int64, device=dev)
    api.pooled_edges_export(topo.ws_i32, None, topo.n_nodes, topo.n_edges, B, e1, pooled, None,
                            _lib.current_stream(pooled))
    node_ptr1 = topo.array("CPTR0")[:B + 1].clone()
    edge_ptr1 = topo.array("E1PTR")[:B + 1].clone()
    d1 = labeller(pooled, node_ptr1, edge_ptr1, api=api)[0]
    return (d0, d1, node_ptr1) if with_cluster_ptr else (d0, d1)


def PreCluster(dataset, method='mcl', batch_size=64, device=None, api=None):
    """Pre-clusters the nodes of every graph of a ``GraphDataSet`` and attaches the labels to its
    store as ``clustering/<method>/depth_0`` and ``depth_1`` (reference DataSet.py:45-88, which
    writes them into the HDF5); ``method`` is 'mcl' or 'louvain', and the other method's groups are left as
    they are.  Call ``store.save_native(path)`` / ``save_npz(path)`` on ``dataset.stores`` to persist."""
    from .data import Batch
    _labeller(method)                              # an unknown method: ValueError before any work
    api = api or _lib.get()
    if device is None:
        device = 'cuda' if api is _lib._API or torch.cuda.is_available() else 'cpu'
    where = [dataset.store_of(i) for i in range(len(dataset))]       # (store, mol) per entry: several files allowed
    for lo in range(0, len(where), batch_size):
        chunk = where[lo:lo + batch_size]
        graphs = [dataset.load_one_graph(m, st) for st, m in chunk]
        for g in graphs:
            g.cluster0 = None
            g.cluster1 = None
        batch = Batch.from_data_list(graphs).to(device)
        d0, d1 = precluster(batch, method=method, api=api)
        d0, d1 = d0.cpu().numpy(), d1.cpu().numpy()
        n_off = c_off = 0
        for (st, m), g in zip(chunk, graphs):
            n = g.num_nodes
            lab0 = d0[n_off:n_off + n]
            c = int(len(set(lab0.tolist())))
            st.set(m, "clustering/%s/depth_0" % method.lower(), lab0.copy())
            st.set(m, "clustering/%s/depth_1" % method.lower(), d1[c_off:c_off + c].copy())
            n_off += n
            c_off += c
    return dataset
