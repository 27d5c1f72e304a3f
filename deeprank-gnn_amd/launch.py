"""Launch set-up of the fused step kernels, shared by their front ends: FusedTrainer (trainer.py), the drop-in
``model(batch)`` boundary StepEngine (fused_autograd.py), and Ensemble / Cohort (ensemble.py, cohort.py).

What a launch of drgnn_net_train_step / drgnn_net_train_step_cached / drgnn_ens_predict_cached /
drgnn_cohort_train_step_cached is handed is decided here once: where a net's parameters sit (NetLayout), its head descriptor,
which TOPO_* flags of a workspace the launch may rely on, the launch hints, the exchange words, whether a plan is a fused
launch at all, and whether a set's targets suit the task.  What K members of one net over packed storage are (their nets,
trainers, [K, P] buffers and member tables) lives in members.py.
"""
import torch

from . import _lib

HEAD = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


class NetLayout(object):
    """One of the three reference nets as the fused kernels see it: ``kind``, ``n_branch``, ``convs`` (the conv modules in
    kernel order), the ``offset`` of every parameter in one flat buffer in ``named_parameters`` order and their ``total``,
    the offset of the FC head (one contiguous block: the head's gradient is written as one), the ``live`` conv parameters,
    the ``dead`` (offset, size) ranges no kernel writes a gradient for, and the head's R / H / O."""

    def __init__(self, net):
        name = type(net).__name__
        if name == "GINet":
            self.kind, self.n_branch, self.convs = _lib.GINET, 2, [net.conv1, net.conv2, net.conv1_ext, net.conv2_ext]
        elif name == "sGAT":
            self.kind, self.n_branch, self.convs = _lib.SGAT, 1, [net.conv1, net.conv2]
        elif name == "FoutNet":
            self.kind, self.n_branch, self.convs = _lib.FOUT, 1, [net.conv1, net.conv2]
        else:
            raise TypeError("the fused step drives GINet / sGAT / FoutNet, not %s" % name)
        named = list(net.named_parameters())
        self.offset, off = {}, 0
        for n, p in named:
            self.offset[n] = off
            off += p.numel()
        self.total = off
        lookup = dict(named)
        self.head_offset = expect = self.offset[HEAD[0]]
        for n in HEAD:
            if self.offset[n] != expect:
                raise _lib.DrgnnError("unexpected parameter order for the FC head")
            expect += lookup[n].numel()
        self.live = tuple(p for c in self.convs for p in c.live_parameters())
        skip = {id(p) for p in self.live} | {id(lookup[n]) for n in HEAD}
        # parameters no kernel writes a gradient for (GINetConvLayer's attention: identically zero, ginet.py:63-66)
        self.dead = [(self.offset[n], p.numel()) for n, p in named if id(p) not in skip]
        self.R, self.H, self.O = net.fc1.in_features, net.fc1.out_features, net.fc2.out_features

    def bind(self, net, flat_p, flat_g=None):
        """Make ``net``'s parameters views of ``flat_p`` at their offsets (their ``.grad`` views of ``flat_g``); no copy."""
        for name, p in net.named_parameters():
            off, n = self.offset[name], p.numel()
            p.data = flat_p[off:off + n].view(p.shape)
            if flat_g is not None:
                p.grad = flat_g[off:off + n].view(p.shape)


def head_desc(net, task, train, p_drop, seed, transform_sigmoid=False, class_w=None, drop_mask=None):
    """drgnn_head_desc of ``net``'s FC head.  ``drop_mask`` (test hook, drgnn_head_desc.drop_mask): an explicit [B, H] 0 / 1
    mask instead of the hash stream."""
    hd = _lib.HeadDesc()
    hd.R, hd.H, hd.O = net.fc1.in_features, net.fc1.out_features, net.fc2.out_features
    hd.task, hd.train, hd.p_drop, hd.seed = task, int(train), float(p_drop), seed
    hd.transform_sigmoid = int(transform_sigmoid)
    hd.w1, hd.b1 = net.fc1.weight.data_ptr(), net.fc1.bias.data_ptr()
    hd.w2, hd.b2 = net.fc2.weight.data_ptr(), net.fc2.bias.data_ptr()
    hd.class_w = None if class_w is None else class_w.data_ptr()
    if drop_mask is not None:
        assert drop_mask.dtype == torch.float32 and drop_mask.is_contiguous() and drop_mask.shape[-1] == hd.H
    hd.drop_mask = None if drop_mask is None else drop_mask.data_ptr()
    return hd


def fused(plan, family=None):
    """True when ``plan`` is a launch of a fused step kernel of ``family`` (None: any family) within a workgroup's LDS."""
    ok = plan.family != _lib.STEP_FAMILY_NONE if family is None else plan.family == family
    return ok and 0 < plan.lds_bytes <= _lib.LDS_LIMIT


def wrong_targets(regression, y):
    """None when the targets ``y`` of a resident set suit the task (float32 for regression, int64 class indices), else the
    message of the callers that raise"""
    want = torch.float32 if regression else torch.int64
    return None if (y is not None and y.dtype == want) else "the set's targets must be %s for this task" % want


# -- topology flags ---------------------------------------------------------------------------------------------------------
def tiles_match(kind, topo):
    """The aggregation tiles of a workspace built WITH edge weights are weighted sums (what sGAT starts from); GINet /
    FoutNet start from plain sums: a workspace of the other flavour is stepped without its tiles."""
    return (getattr(topo, "ws_f32", None) is not None) == (kind == _lib.SGAT)


def _aligned(x):
    return x.shape[1] % 4 != 0 or x.data_ptr() % 16 == 0


def usable_flags(kind, topo, x=None, reform=None):
    """The TOPO_* flags of ``topo`` as a launch of a ``kind`` net may rely on them: TILES only with tiles of this kind's
    flavour that were formed from the ``x`` the launch steps (a Topology bakes the neighbour sums of its ``x`` in at build
    time: another tensor, or the same one modified in place since, makes them stale) in 16-byte aligned memory.

    ``reform``: form stale tiles again from ``x`` first (own launch, same stream).  The two front ends that step collated
    mini-batches do this differently, and each one's launches depend on its own rule:
      "full"  FusedTrainer: only tiles the build held, by a full build (``full_flags``).  It steps workspaces its caller
              built or co-built with the flags it asked for, and a workspace built without tiles stays without them.
      "keep"  StepEngine: any tiles of the workspace, keeping the build's other flags (lean).  It owns the workspace of the
              batch (``topology_for``), which leaves out the tiles the builder cannot stage unless the lean plan takes them:
              these are formed here, on the first call for the batch."""
    flags = int(getattr(topo, "flags", 0))
    tiles = getattr(topo, "tiles", None)
    if tiles is None or not tiles_match(kind, topo):
        return flags & ~_lib.TOPO_TILES
    if x is None:
        return flags
    tx = getattr(topo, "x", None)
    if (flags & _lib.TOPO_TILES) and tx is not None and tx.data_ptr() == x.data_ptr() and \
            tuple(tx.shape) == tuple(x.shape) and _aligned(x) and getattr(topo, "_tiles_x_version", None) == x._version:
        return flags
    if reform is not None and (reform == "keep" or flags & _lib.TOPO_TILES) and tuple(tx.shape) == tuple(x.shape) and \
            _aligned(x) and getattr(topo, "_inputs", None) is not None:
        topo.x = x
        topo.rebuild(topo.full_flags() if reform == "full" else flags | _lib.TOPO_TILES)
        return usable_flags(kind, topo, x)
    return flags & ~_lib.TOPO_TILES


def cached_flags(kind, cache):
    """(flags, tiles) of a launch over the cached set ``cache`` (resident.TopologyCache): the set's tiles of this kind's
    flavour, when its node rows are 16-byte aligned."""
    flags = int(getattr(cache.topo, "flags", 0))
    tiles = cache.tiles_for(kind == _lib.SGAT) if (flags & _lib.TOPO_TILES) else None
    if tiles is None or not _aligned(cache.set.x):
        return flags & ~_lib.TOPO_TILES, None
    return flags, tiles


# -- hints and exchange words -----------------------------------------------------------------------------------------------
def batch_hints(batch, topo, flags, plan, from_topo=False):
    """(StepHints, keep-alive) of a launch over a collated mini-batch.  Up to 64 graphs the host copies of its offsets
    (Batch.from_data_list / the resident set record them) travel in the launch arguments, so a workgroup need not fetch them
    from the workspace first.  ``from_topo``: a batch object that records none takes those Topology.from_batch derived."""
    bd = getattr(batch, "__dict__", {})
    hn, he = bd.get("_host_node_ptr"), bd.get("_host_edge_ptr")
    if hn is None and from_topo:
        hn, he = getattr(topo, "host_node_ptr", None), getattr(topo, "host_edge_ptr", None)
    tiles = getattr(topo, "tiles", None) if (flags & _lib.TOPO_TILES) else None
    B = topo.n_graphs
    if hn is not None and he is not None and len(hn) == B + 1 and B <= 64:
        return _lib.step_hints(node_ptr=hn, edge_ptr=he, topo_flags=flags, tiles=tiles, plan=plan)
    return _lib.step_hints(topo_flags=flags, tiles=tiles, plan=plan)


def set_hints(gset, ids, flags, tiles, plan, next_ids=None):
    """(StepHints, keep-alive) of a launch over the graphs ``ids`` of the resident set ``gset``; ``next_ids``: the next
    mini-batch's graph numbers (device int32), prefetched by spare workgroups.  (Beyond 64 graphs the offsets no longer
    travel in the kernel arguments, but the library still range-checks the ids.)"""
    return _lib.step_hints(set_node_ptr=gset.node_ptr, set_edge_ptr=gset.edge_ptr, ids=ids, topo_flags=flags, tiles=tiles,
                           plan=plan, next_ids=next_ids)


class ExchangeWords(object):
    """Exchange words of the fused step launches: ONE buffer per batch size, grown to the largest need seen (the words carry
    the step index as a tag, so stale ones are harmless; the launch is told the stride through its bounds)."""

    def __init__(self, n_branch, H):
        self.n_branch, self.H, self.bufs = n_branch, H, {}

    def get(self, plan, B, device):
        words = int(plan.xchg_words)
        if words <= 0 and self.n_branch == 1:
            return None
        words = max(words, self.n_branch * max(self.H, 32))
        buf = self.bufs.get(B)
        if buf is None or buf.shape[1] < words:
            buf = self.bufs[B] = torch.zeros((max(B, 1), words), dtype=torch.int64, device=device)
        return buf

    def zero(self):
        """Forget every tag (those of an earlier run must not match again)."""
        for buf in self.bufs.values():
            buf.zero_()
