"""What a later launch reads is stored write-through (out_store, drgnn_rt.h): the builder's tiles and index arrays, the
step's gradient slabs, head rows and readout.  These checks run the shapes at which a widened or re-typed store can go
wrong -- graphs of 1 / 63 / 65 / 200 nodes with 1 / 3 / 5 / 32 / 33 features, odd and zero edge counts, a first graph with odd
node / edge / cluster counts (the int32 arrays of the graphs behind it then start at addresses that are not multiples of 8
bytes) and a graph without edges -- and compare bit for bit: the co-built workspace and tiles against an own-launch build,
the pipelined route against the route that builds every topology with a launch of its own, a recorded graph against eager
stepping.  Shared by test_gpu_store_policy.py (device) and test_emu_store_policy.py (host emulation: the index logic)."""
import numpy as np
import torch

from deeprank_gnn_amd.data import Batch, Data
from deeprank_gnn_amd.topology import Topology
from deeprank_gnn_amd.trainer import FusedTrainer

NODES = [1, 63, 65, 200]
FEATS = [1, 3, 5, 32, 33]
NETS = ["GINet", "sGAT", "FoutNet"]


def _net(net_name, n_feat):
    from deeprank_gnn_amd.ginet import GINet
    from deeprank_gnn_amd.sGAT import sGAT
    from deeprank_gnn_amd.foutnet import FoutNet
    return {"GINet": GINet, "sGAT": sGAT, "FoutNet": FoutNet}[net_name](n_feat, 1, 1)


def odd_edges(n):
    """an odd number of directed edges for n nodes (0 where a graph cannot have one)"""
    if n < 2:
        return 0
    return min(int(2.3 * n) | 1, (n * (n - 1) - 1) | 1)


def make_graph(seed, n, e, n_feat, odd_clusters=False, edge_seed=0):
    """n nodes, e distinct directed edges in no particular order (no self loops), depth-0 clusters of about four nodes with
    local labels in [0, C), depth-1 clusters over them.  ``edge_seed`` varies the edges alone."""
    rng = np.random.default_rng(977 * seed + 13)
    x = rng.standard_normal((n, n_feat)).astype(np.float32)
    y = np.float32(rng.uniform(0.0, 4.0))
    size = 4
    if odd_clusters:
        size = next(s for s in (4, 3, 5, 2, 1) if ((n + s - 1) // s) % 2 == 1)
    C = (n + size - 1) // size
    cluster0 = np.empty(n, dtype=np.int64)
    cluster0[rng.permutation(n)] = np.arange(n) // size
    cluster1 = np.empty(C, dtype=np.int64)
    cluster1[rng.permutation(C)] = np.arange(C) % max(1, min(5, C))
    erng = np.random.default_rng(7919 * seed + 31 * edge_seed + 5)
    assert e <= n * (n - 1)
    flat = erng.choice(n * (n - 1), size=e, replace=False) if e else np.zeros(0, dtype=np.int64)
    r = flat // max(n - 1, 1)
    c = flat % max(n - 1, 1)
    c = c + (c >= r)
    ei = np.stack([r, c]).astype(np.int64).reshape(2, e)
    ea = erng.uniform(0.5, 2.0, size=(e, 1)).astype(np.float32)
    g = Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei), edge_attr=torch.from_numpy(ea), y=torch.tensor([y]))
    g.cluster0 = torch.from_numpy(cluster0)
    g.cluster1 = torch.from_numpy(cluster1)
    return g


def make_batches(n, n_feat, edge_seed=0):
    """two mini-batches of three graphs for the case (n nodes, n_feat features)"""
    first = n if n % 2 else n - 1                   # odd node count; its edge and cluster counts are odd too
    a = [make_graph(1, first, odd_edges(first), n_feat, True, edge_seed),
         make_graph(2, n, odd_edges(n), n_feat, False, edge_seed),
         make_graph(3, 5, 0, n_feat, False, edge_seed)]                       # a graph without edges
    b = [make_graph(4, max(first - 2, 1), odd_edges(max(first - 2, 1)), n_feat, True, edge_seed),
         make_graph(5, 3, 0, n_feat, False, edge_seed),
         make_graph(6, n, odd_edges(n), n_feat, False, edge_seed)]
    return [Batch.from_data_list(a), Batch.from_data_list(b)]


def _trainer(net_name, n_feat, dev, api, seed=3):
    torch.manual_seed(seed)
    net = _net(net_name, n_feat).to(dev)
    kw = {} if api is None else {"api": api}
    return FusedTrainer(net, lr=0.01, seed=7, **kw)


def _topo(batch, net_name, api, build=True):
    kw = {} if api is None else {"api": api}
    t = Topology.from_batch(batch, need_weights=(net_name == "sGAT"), build=False, **kw)
    # (every word the builder does not write reads the same in two workspaces)
    for buf in (t.ws_i32, t.ws_f32, t.tiles):
        if buf is not None:
            buf.zero_()
    return t.rebuild() if build else t


def _same_workspace(got, want, what):
    for name in ("ws_i32", "ws_f32", "tiles"):
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), "%s: %s" % (what, name)
        if a is not None:
            # (bit patterns: a NaN would compare unequal to itself)
            assert torch.equal(a.view(torch.int32).cpu(), b.view(torch.int32).cpu()), "%s: %s differs" % (what, name)


def check_workspace(net_name, n, n_feat, dev, api=None):
    """Two pipelined steps over alternating workspaces: what each step co-builds equals an own-launch build of the same
    request, workspace and tiles, bit for bit."""
    batches = [b.to(dev) for b in make_batches(n, n_feat)]
    tr = _trainer(net_name, n_feat, dev, api)
    topos = [_topo(batches[0], net_name, api), _topo(batches[1], net_name, api, build=False)]
    for k in range(2):
        nxt = topos[1 - k]
        tr.train_step(batches[k], topo=topos[k], next_topo=nxt)
        assert nxt.status()[0] == 0, "builder status, step %d" % k
        own = _topo(batches[1 - k], net_name, api, build=False).rebuild(int(nxt.flags))
        _same_workspace(nxt, own, "step %d, flags %d" % (k, int(nxt.flags)))
        if k == 0:
            # the workspace step 1 builds into: cleared like a fresh one
            for buf in (topos[0].ws_i32, topos[0].ws_f32, topos[0].tiles):
                if buf is not None:
                    buf.zero_()
    assert np.isfinite(float(tr.loss))


def _state(tr):
    return [tr.flat_p.detach().cpu().clone(), tr.flat_g.detach().cpu().clone(), tr.loss.detach().cpu().clone().reshape(-1),
            tr.last_pred.detach().cpu().clone().reshape(-1)]


def _assert_same_state(a, b, what):
    for name, u, v in zip(("parameters", "gradients", "loss", "predictions"), a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "%s: %s differ" % (what, name)


def check_routes(net_name, n, n_feat, dev, api=None):
    """Two pipelined steps == two steps that build each topology with a launch of its own: parameters, gradients, loss and
    predictions, bit for bit."""
    batches = [b.to(dev) for b in make_batches(n, n_feat)]
    ta = _trainer(net_name, n_feat, dev, api)
    tb = _trainer(net_name, n_feat, dev, api)
    assert torch.equal(ta.flat_p, tb.flat_p)
    topos = [_topo(batches[0], net_name, api), _topo(batches[1], net_name, api, build=False)]
    for k in range(2):
        ta.train_step(batches[k], topo=topos[k], next_topo=topos[1 - k])
        tb.train_step(batches[k], topo=_topo(batches[k], net_name, api))
        _assert_same_state(_state(ta), _state(tb), "%s n=%d F=%d step %d" % (net_name, n, n_feat, k))
    assert np.isfinite(float(ta.loss))


def check_replay(dev, api=None, n=65, n_feat=5, replays=10, record=True):
    """A pair of pipelined steps over alternating workspaces, run once and then ``replays`` times more -- from a recorded graph
    (``record``) and eagerly -- while the edge list changes in place before every pair: the workspace step k + 1 reads is
    the one step k wrote; a step that read an older one would train on other edges.  Both against the route that builds
    every topology with a launch of its own from the edges that step's topology was built from."""
    pairs = replays + 1
    variants = [[b.to(dev) for b in make_batches(n, n_feat, edge_seed=v)] for v in range(pairs + 1)]

    def set_edges(batches, v):
        for b, src in zip(batches, variants[v]):
            b.edge_index.copy_(src.edge_index)

    def pipelined(recorded):
        batches = [b.clone() for b in variants[0]]
        tr = _trainer("GINet", n_feat, dev, api)
        topos = [_topo(batches[0], "GINet", api), _topo(batches[1], "GINet", api, build=False)]

        def pair():
            tr.train_step(batches[0], topo=topos[0], next_topo=topos[1])
            tr.train_step(batches[1], topo=topos[1], next_topo=topos[0])
        set_edges(batches, 1)
        pair()
        graph = None
        if recorded:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                pair()
        for r in range(1, pairs):
            set_edges(batches, r + 1)
            if graph is not None:
                graph.replay()
            else:
                pair()
        return _state(tr)

    def own_launch():
        # step j of the pipelined run reads the topology of edge list (j + 1) // 2: workspace 0 is first built from list 0,
        # then every pair r builds workspace 1 and, one step later, workspace 0 from list r + 1
        batches = [b.clone() for b in variants[0]]
        tr = _trainer("GINet", n_feat, dev, api)
        for j in range(2 * pairs):
            set_edges(batches, (j + 1) // 2)
            tr.train_step(batches[j & 1], topo=_topo(batches[j & 1], "GINet", api))
        return _state(tr)

    eager = pipelined(False)
    _assert_same_state(eager, own_launch(), "eager pipelined vs own-launch topologies")
    if record:
        _assert_same_state(pipelined(True), eager, "recorded graph vs eager")
