"""The stand-alone conv layers (csrc/drgnn_layers.h: GINetConvLayer / sGraphAttentionLayer / FoutLayer called directly) at the
widths and node counts where their kernels change path: output widths up to DRGNN_LAYER_MAXH = 128, more than 64 input
features, one input feature and one output, 1 / 64 / 65 / 130 nodes around the 64-row blocks.  Forward, x.grad and every
parameter gradient against the oracle's layer functions under tests/elementwise.py (float64 arbiter: the same functions on
float64 inputs).  Shared by test_emu_layers.py and test_gpu_layers.py."""
import numpy as np
import torch

from elementwise import assert_arbiter_rate, check, new_stats
from oracle import cpu_ref

SHAPES = [(100, 128), (70, 96), (3, 1)]          # (input features, output width)
NODES = [1, 64, 65, 130]
KINDS = ["ginet", "sgat", "fout"]


def layer_graph(n_nodes, n_feat, seed):
    """x [N, F], directed edges with duplicates and a self loop, one isolated node (node N // 2; the only node when N = 1)."""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((n_nodes, n_feat)).astype(np.float32))
    iso = n_nodes // 2
    others = np.array([i for i in range(n_nodes) if i != iso], dtype=np.int64)
    if others.size == 0:
        ei = np.zeros((2, 0), dtype=np.int64)
    else:
        ei = others[rng.integers(0, others.size, size=(2, 4 * n_nodes))]        # directed: (a, b) without (b, a)
        ei = np.concatenate([ei, ei[:, :7], np.array([[others[0]], [others[0]]])], axis=1)      # duplicates, a self loop
    ea = torch.from_numpy((0.5 + rng.random((ei.shape[1], 1))).astype(np.float32))
    return x, torch.from_numpy(ei), ea, iso


def _make(kind, n_feat, width):
    from deeprank_gnn_amd.ginet import GINetConvLayer
    from deeprank_gnn_amd.sGAT import sGraphAttentionLayer
    from deeprank_gnn_amd.foutnet import FoutLayer
    if kind == "ginet":
        lay = GINetConvLayer(n_feat, width, 1)
        return lay, [lay.fc.weight], ["fc.weight"]
    if kind == "sgat":
        lay = sGraphAttentionLayer(n_feat, width)
        return lay, [lay.weight, lay.bias], ["weight", "bias"]
    lay = FoutLayer(n_feat, width)
    return lay, [lay.Wc, lay.Wn, lay.bias], ["Wc", "Wn", "bias"]


def _oracle(kind, lay, x, ei, ea, params, wgt, dtype):
    """(out, grad x, parameter grads) of the oracle's layer function in ``dtype``."""
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    rp = [p.detach().cpu().clone().to(dtype).requires_grad_(True) for p in params]
    if kind == "ginet":
        ref = cpu_ref.ginet_conv(xr, ei, ea.to(dtype), rp[0], lay.fc_edge_attr.weight.detach().cpu().to(dtype),
                                 lay.fc_attention.weight.detach().cpu().to(dtype))
    elif kind == "sgat":
        ref = cpu_ref.sgat_conv(xr, ei, ea.to(dtype), *rp)
    else:
        ref = cpu_ref.fout_conv(xr, ei, *rp, looped=False)
    (ref * wgt.to(dtype)).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return [ref.detach().numpy(), zero(xr).numpy()] + [zero(p).numpy() for p in rp]


def check_layer(kind, n_feat, width, n_nodes, device, stats=None):
    own = stats is None
    stats = new_stats() if own else stats
    torch.manual_seed(100 * n_feat + width)
    x0, ei, ea, iso = layer_graph(n_nodes, n_feat, seed=n_nodes + n_feat)
    lay, params, names = _make(kind, n_feat, width)
    wgt = torch.from_numpy(np.random.default_rng(3).standard_normal((n_nodes, width)).astype(np.float32))
    ref32 = _oracle(kind, lay, x0, ei, ea, params, wgt, torch.float32)
    ref64 = []

    def arbiter(i):
        if not ref64:
            ref64.extend(_oracle(kind, lay, x0, ei, ea, params, wgt, torch.float64))
        return ref64[i]
    lay = lay.to(device)
    params = [lay.fc.weight] if kind == "ginet" else list(lay.parameters())
    x = x0.detach().clone().to(device).requires_grad_(True)
    out = lay(x, ei.to(device)) if kind == "fout" else lay(x, ei.to(device), ea.to(device))
    (out * wgt.to(device)).sum().backward()
    where = "%s layer F=%d H=%d N=%d" % (kind, n_feat, width, n_nodes)
    got = [out.detach().cpu().numpy(), x.grad.cpu().numpy()] + [p.grad.cpu().numpy() for p in params]
    for i, name in enumerate(["out", "grad x"] + ["grad " + n for n in names]):
        check("%s %s" % (where, name), got[i], ref32[i], lambda i=i: arbiter(i), stats)
    # the isolated node: the bias row (sGAT), NaN (FoutLayer: mean of no neighbour), zeros (GINet)
    row = got[0][iso]
    if kind == "fout":
        assert np.isnan(row).all()
    elif kind == "sgat":
        np.testing.assert_array_equal(row, lay.bias.detach().cpu().numpy())
    else:
        assert not row.any()
    if kind == "ginet":
        assert float(lay.fc_attention.weight.grad.abs().max()) == 0.0 and float(lay.fc_edge_attr.weight.grad.abs().max()) == 0.0
    if own:
        assert_arbiter_rate(stats, where)
    return stats


def check_layers(kind, n_feat, width, device):
    """every node count of NODES for one layer shape; prints the arbiter count"""
    stats = new_stats()
    for n_nodes in NODES:
        check_layer(kind, n_feat, width, n_nodes, device, stats)
    assert_arbiter_rate(stats, "%s layer F=%d H=%d" % (kind, n_feat, width))
    print("LAYER %-8s F=%-3d H=%-3d nodes %s elements=%-6d arbiter=%d" % (kind, n_feat, width, NODES, stats["elements"], stats["arbiter"]))


def check_too_wide(kind, device):
    """H = 129 > DRGNN_LAYER_MAXH: DrgnnError (DRGNN_E_WIDTH) from the layer module, and from the library's forward and backward
    entry points with valid buffers of that width -- nothing launched: every output buffer keeps the 7s it was filled with
    (conv_layer_fill returns before the first kernel of either entry point)."""
    import pytest
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.functional import _fill_conv, _fill_grads
    from deeprank_gnn_amd.topology import Topology
    n_nodes, n_feat, width = 65, 10, 129
    x, ei, ea, _ = layer_graph(n_nodes, n_feat, seed=1)
    lay, _, _ = _make(kind, n_feat, width)
    lay = lay.to(device)
    x, ei, ea = x.to(device), ei.to(device), ea.to(device)
    with pytest.raises(_lib.DrgnnError, match="unsupported width"):
        lay(x, ei) if kind == "fout" else lay(x, ei, ea)
    api = _lib.get()
    code = {"ginet": _lib.GINET, "sgat": _lib.SGAT, "fout": _lib.FOUT}[kind]
    params = tuple(p.detach() for p in ([lay.fc.weight] if kind == "ginet" else lay.parameters()))
    topo = Topology.single_graph(ei, ea if kind == "sgat" else None, n_nodes, api=api)
    sevens = lambda *shape: torch.full(shape, 7.0, device=device)
    hc = width if kind == "ginet" else 2 * width
    cp, cg = _lib.ConvParams(), _lib.ConvGrads()
    _fill_conv(cp, code, params, n_feat, width)
    u, out = sevens(n_nodes, hc), sevens(n_nodes, width)
    stream = _lib.current_stream(x)
    with pytest.raises(_lib.DrgnnError, match="unsupported width"):
        api.conv_layer_forward(code, x, n_feat, width, cp, topo.ws_i32, topo.ws_f32, topo.n_edges, u, out, stream)
    grads = tuple(sevens(*p.shape) for p in params)
    _fill_grads(cg, code, grads, n_feat, width)
    du, gx = sevens(n_nodes, hc), sevens(n_nodes, n_feat)
    partials = sevens(api.conv_layer_slabs(n_nodes), api.conv_layer_partial_elems(code, n_feat, width))
    with pytest.raises(_lib.DrgnnError, match="unsupported width"):
        api.conv_layer_backward(code, x, n_feat, width, cp, topo.ws_i32, topo.ws_f32, topo.n_edges, sevens(n_nodes, width), du,
                                partials, cg, gx, stream)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    for t in (u, out, du, gx, partials) + grads:
        assert bool((t == 7.0).all())
