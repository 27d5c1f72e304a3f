"""The Adam update on every path against a float64 restatement of torch.optim.Adam's single-tensor formula.

Every update launch leaves the summed fp32 gradient it consumed in ``flat_g`` (k_adam reads it from there), so after any
optimisation step the device holds the state before (snapshot), the exact gradient Adam used and the state after: the
optimiser is checked ALONE, at a few fp32 ulps, without the gradient's own parity error in the comparison.  Shared by the
emulated (CPU) and the MI355X tests: every check takes ``device`` and ``api``.

The bounds (``u = 2**-24``, ``c = 16``):

    |m' - ref| <= c u (|g| + |m|)
    |v' - ref| <= c u v'_ref
    |p' - ref| <= u |p| + c u |p - p'_ref|

With weight decay the gradient is ``g + wd p``, a sum that can cancel: the scale of the first line is then
``|g| + wd |p| + |m|``, and the second carries the one rounding of ``(float)wd`` (an error of ``d = u wd |p|`` in the sum)
through the square, ``(1 - b2) (2 |g + wd p| d + d^2)``.  Without weight decay both terms vanish.

``c`` is a count of individually rounded fp32 operations (``fp contract(off)``: every product and sum rounds once), not a
fit to what the kernel gives.  Per output, casts of the double scalars included:

    m'  (float)wd, fma(wd, p, g) | g - m, (float)(1 - b1), product, sum                               6
    v'  g twice (2 roundings each with weight decay) | (float)b2, b2 v, (float)(1 - b2), two products, sum   10
    p'  sqrtf, (float)sqrt(bc2), quotient, + eps ((float)eps), m' / denom, (float)(lr / bc1), product,
        and the final difference (the u |p| term)                                                      9

each error relative to a term no larger than the scale on the right-hand side, so every output stays under 16.

The count for p' starts at the moments the step STORED: its reference is the float64 update formula applied to the fp32
``m'`` and ``v'`` the kernel wrote, which are pinned to float64 by their own lines.  Against the float64 chain from the old
moments no operation count bounds p': the lerp's subtraction cancels (g near -9 m at beta1 = 0.9, |m| >> |g| at beta1 = 0),
m' keeps an absolute error of a few u (|g| + |m|) and that is then an arbitrary multiple of the update.  A wrong eps, bias
correction, learning rate or operation order shows in the p' line, a wrong moment formula in its own.

``TINY = 2**-126`` (the smallest normal fp32) is added to every bound: a real gradient element below ~1e-17 squares into
the subnormal range, where fp32 keeps no relative precision (or flushes to zero).  The synthetic inputs stay clear of it
and assert so.
"""
import copy

import numpy as np
import torch

import deeprank_gnn_amd.synthetic as synth
from deeprank_gnn_amd.data import Batch
from deeprank_gnn_amd.foutnet import FoutNet
from deeprank_gnn_amd.ginet import GINet
from deeprank_gnn_amd.launch import NetLayout
from deeprank_gnn_amd.resident import ResidentGraphSet
from deeprank_gnn_amd.sGAT import sGAT
from deeprank_gnn_amd.trainer import FusedTrainer

U = 2.0 ** -24
C = 16.0
TINY = 2.0 ** -126
GUARD, SENTINEL = 64, -12345.0

NETS = {"GINet": GINet, "sGAT": sGAT, "FoutNet": FoutNet}
# (lr, betas, eps, weight_decay)
HYPER = [(0.01, (0.9, 0.999), 1e-8, 0.0),
         (0.1, (0.5, 0.9), 1e-3, 0.0),
         (1e-3, (0.0, 0.999), 1e-8, 0.0),          # beta1 = 0: bc1 = 1
         (0.01, (0.9, 0.999), 1e-8, 0.05)]
T0 = [0, 1, 9, 999, 10 ** 7]                       # at 10**7 both bias corrections are exactly 1
SIZES = [1, 255, 256, 257, 4273, 10697]            # the 256-thread tail; the sGAT and GINet parameter counts
PATHS = ["fused", "pair", "cached", "epoch"]
# (net, task, outputs) of the trainer-path checks: regression for all three nets, GINet classification with O = 2
PATH_NETS = [("GINet", "reg", 1), ("sGAT", "reg", 1), ("FoutNet", "reg", 1), ("GINet", "class", 2)]


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64)


def bias_corrections(t, betas):
    return 1.0 - betas[0] ** t, 1.0 - betas[1] ** t


def update_ref64(p, m1, v1, t, lr, betas, eps):
    """the parameter line alone, float64:  p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)"""
    bc1, bc2 = bias_corrections(t, betas)
    return p - lr / bc1 * (m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps))


def adam_ref64(p, m, v, g, t, lr, betas, eps, weight_decay):
    """torch.optim.Adam (_single_tensor_adam; no amsgrad, maximize=False) in numpy float64.  ``t``: the step index Adam uses,
    starting at 1; the hyper-parameters enter as Python doubles, as in torch.  Returns (p', m', v')."""
    p, m, v, g = (np.asarray(a, dtype=np.float64) for a in (p, m, v, g))
    b1, b2 = betas
    g = g + weight_decay * p
    m1 = m + (g - m) * (1.0 - b1)
    v1 = b2 * v + (1.0 - b2) * g * g
    return update_ref64(p, m1, v1, t, lr, betas, eps), m1, v1


def one_step_bounds(p, m, g, ref, hyper):
    """(bound of p', of m', of v') for a step from (p, m, .) with gradient g whose float64 result is ``ref``"""
    wd, b2 = hyper[3], hyper[1][1]
    p1, _, v1 = ref
    # weight decay: g + wd p can cancel, and the ONE rounding of (float)wd is relative to wd |p|, not to the sum
    d = U * wd * np.abs(p)
    return (U * np.abs(p) + C * U * np.abs(p - p1) + TINY,
            C * U * (np.abs(g) + wd * np.abs(p) + np.abs(m)) + TINY,
            C * U * v1 + (1.0 - b2) * (2.0 * np.abs(g + wd * p) * d + d * d) + TINY)


def assert_adam_step(before, g, after, t, hyper, mask=None, what=""):
    """``before`` / ``after``: (param, exp_avg, exp_avg_sq) around ONE update that used gradient ``g`` and step index ``t``;
    ``hyper``: (lr, betas, eps, weight_decay).  ``mask``: the elements to compare (default: all)."""
    lr, betas, eps, wd = hyper
    p, m, v = (_f64(a) for a in before)
    p1, m1, v1 = (_f64(a) for a in after)
    g = _f64(g)
    assert t >= 1
    for name, a in (("param", p1), ("exp_avg", m1), ("exp_avg_sq", v1)):
        assert np.isfinite(a).all(), "%s: %s is not finite after step %d" % (what, name, t)
    ref = adam_ref64(p, m, v, g, t, lr, betas, eps, wd)
    _, bm, bv = one_step_bounds(p, m, g, ref, hyper)
    # p' from the moments the step stored (module docstring)
    p_ref = update_ref64(p, m1, v1, t, lr, betas, eps)
    bp = U * np.abs(p) + C * U * np.abs(p - p_ref) + TINY
    sel = np.ones(p.shape, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    for name, got, want, bound in (("exp_avg", m1, ref[1], bm), ("exp_avg_sq", v1, ref[2], bv), ("param", p1, p_ref, bp)):
        err = np.abs(got - want)
        bad = sel & ~(err <= bound)
        if bad.any():
            i = int(np.argmax(np.where(bad, err / bound, 0.0)))
            raise AssertionError(
                "%s: %s off at %d of %d elements, t=%d hyper=%r; worst at [%d]: got %.9g want %.9g, error %.3g = %.1f x "
                "the bound %.3g (p=%.9g m=%.9g v=%.9g g=%.9g)" % (what, name, int(bad.sum()), int(sel.sum()), t, hyper, i,
                                                                 got[i], want[i], err[i], err[i] / bound[i], bound[i],
                                                                 p[i], m[i], v[i], g[i]))
    if wd == 0.0:
        idle = sel & (g == 0.0) & (m == 0.0) & (v == 0.0)
        for name, a, b in (("param", before[0], after[0]), ("exp_avg", before[1], after[1]), ("exp_avg_sq", before[2], after[2])):
            a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
            assert np.array_equal(a.view(np.int32)[idle], b.view(np.int32)[idle]), \
                "%s: %s of an element with zero gradient and zero moments changed" % (what, name)
    return ref


# ---- the kernel alone -----------------------------------------------------------------------------------------------
def synthetic_gradient(rng, n):
    """random signs, magnitudes log-uniform in [1e-15, 1e3], about 5 % exact zeros"""
    g = np.sign(rng.random(n) - 0.5) * 10.0 ** rng.uniform(-15.0, 3.0, n)
    g[rng.random(n) < 0.05] = 0.0
    return g.astype(np.float32)


def assert_above_underflow(g, p, hyper):
    """(1 - b2) g^2 is a normal fp32 number (or exactly 0) for every element: fp32 and the float64 reference then agree about
    underflow"""
    ge = g.astype(np.float64) + hyper[3] * p.astype(np.float64)
    term = (1.0 - hyper[1][1]) * ge * ge
    assert ((term == 0.0) | (term >= 4.0 * TINY)).all()


def check_adam_kernel(device, api, n, hyper, t0, steps=3, seed=0):
    """``api.adam_step`` (k_adam) on synthetic flat buffers: ``steps`` consecutive updates with a fresh gradient each, every
    one checked on its own; the final state against the float64 trajectory fed the same gradients; guard regions behind
    param, exp_avg and exp_avg_sq untouched."""
    lr, betas, eps, wd = hyper
    rng = np.random.default_rng(seed * 1000003 + n * 31 + t0 % 1009)
    p0 = rng.standard_normal(n).astype(np.float32)
    if t0 == 0:
        m0, v0 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        g0 = synthetic_gradient(rng, n)
        m0 = (g0 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
        v0 = (np.maximum(np.abs(g0), 1e-15) * rng.uniform(0.1, 3.0, n)).astype(np.float32) ** 2
        assert (v0 >= 4.0 * TINY).all()

    def guarded(a):
        buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=device)
        buf[:n] = torch.from_numpy(a)
        return buf
    P, M, V = guarded(p0), guarded(m0), guarded(v0)
    G = torch.zeros(n, dtype=torch.float32, device=device)
    step = torch.full((1,), t0, dtype=torch.int32, device=device)
    traj = tuple(a.astype(np.float64) for a in (p0, m0, v0))
    # accumulated bounds along the float64 trajectory: the one-step bounds of the moments add up (each later step shrinks an
    # earlier error by beta < 1), and a moment's accumulated error moves that step's update by, to first order,
    # |update| (E_m / |m'| + E_v / (2 v'))
    acc_p, acc_m, acc_v = np.zeros(n), np.zeros(n), np.zeros(n)
    for k in range(1, steps + 1):
        g = synthetic_gradient(rng, n)
        before = tuple(a[:n].clone() for a in (P, M, V))
        assert_above_underflow(g, before[0].cpu().numpy(), hyper)
        G.copy_(torch.from_numpy(g))
        step.fill_(t0 + k)                            # "*step must already count this update"
        api.adam_step(P[:n], G, M[:n], V[:n], step, lr, betas[0], betas[1], eps, wd, _stream(P))
        after = tuple(a[:n].clone() for a in (P, M, V))
        assert_adam_step(before, g, after, t0 + k, hyper, what="adam_step n=%d step %d" % (n, k))
        ref = adam_ref64(traj[0], traj[1], traj[2], g, t0 + k, lr, betas, eps, wd)
        bp, bm, bv = one_step_bounds(traj[0], traj[1], g, ref, hyper)
        acc_m, acc_v = acc_m + bm, acc_v + bv
        upd = np.abs(traj[0] - ref[0])
        with np.errstate(divide="ignore", invalid="ignore"):
            moved = upd * (np.where(ref[1] != 0.0, acc_m / np.abs(ref[1]), 0.0) + np.where(ref[2] != 0.0, 0.5 * acc_v / ref[2], 0.0))
        acc_p = acc_p + bp + moved
        traj = ref
    # "3 x the one-step bound": the three one-step bounds of the trajectory, summed
    for name, got, want, bound in (("param", P, traj[0], acc_p), ("exp_avg", M, traj[1], acc_m), ("exp_avg_sq", V, traj[2], acc_v)):
        err = np.abs(_f64(got[:n]) - want)
        assert (err <= bound).all(), "%s after %d steps: worst %.3g x the accumulated bound (n=%d t0=%d %r)" % (
            name, steps, float(np.max(err / bound)), n, t0, hyper)
    for name, buf in (("param", P), ("exp_avg", M), ("exp_avg_sq", V)):
        assert bool((buf[n:] == SENTINEL).all()), "adam_step wrote behind %s[%d]" % (name, n)
    assert int(step) == t0 + steps


def _stream(t):
    from deeprank_gnn_amd import _lib
    return _lib.current_stream(t)


# ---- a real step on every path --------------------------------------------------------------------------------------
def small_graphs(n_graphs=3, n_feat=5, first=0):
    """ragged graphs of 20 - 30 nodes"""
    sizes = [21, 26, 30, 23, 28, 25]
    return [synth.make_graph(first + i, n_nodes=sizes[i % 6], n_pairs=34 + 5 * (i % 3), n_feat=n_feat, n_c1=3, n_internal=12)
            for i in range(n_graphs)]


def make_case(net_name, task, n_out, device, api, hyper, n_graphs=3, seed=0, net=None):
    """(trainer, graphs, collated batch, resident set) of one trainer-path case: dropout 0"""
    torch.manual_seed(seed)
    graphs = small_graphs(n_graphs)
    if task == "class":
        for i, g in enumerate(graphs):
            g.y = torch.tensor([i % n_out])
    if net is None:
        net = NETS[net_name](5, n_out, 1)
    if hasattr(net, "dropout"):
        net.dropout = 0.0
    lr, betas, eps, wd = hyper
    tr = FusedTrainer(net.to(device), lr=lr, betas=betas, eps=eps, weight_decay=wd, task=task, seed=3, api=api)
    batch = Batch.from_data_list(graphs).to(device)
    rs = ResidentGraphSet(graphs, device, api=api)
    if task == "class":
        rs.set_targets(torch.tensor([i % n_out for i in range(n_graphs)]))
    return tr, graphs, batch, rs


def snapshot(tr):
    return tuple(a.detach().clone() for a in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq))


def live_mask(tr):
    """elements of the flat buffers that belong to a parameter with a gradient (all but NetLayout.dead)"""
    mask = np.ones(tr.flat_p.numel(), dtype=bool)
    for off, n in tr.layout.dead:
        mask[off:off + n] = False
    return mask


def step_on_path(tr, path, batch, rs, ids):
    """one optimisation step on ``path``; returns what the entry point returned"""
    if path in ("fused", "pair"):
        tr.fused_step = path == "fused"
        return tr.train_step(batch)
    need_w = isinstance(tr.net, sGAT)
    if path == "cached":
        return tr.train_step_cached(rs.topology_cache(need_weights=need_w), ids)
    assert path == "epoch"
    return tr.train_epoch(rs, ids, len(ids))          # ONE mini-batch: flat_g is that step's


def check_trainer_paths(net_name, device, api, path, hyper, t0, task="reg", n_out=1):
    """Two consecutive real steps on ``path`` from step counter ``t0``: snapshot, step, assert_adam_step with the gradient
    the update left in flat_g.

    Weight decay: compared on the live parameters only -- torch.optim.Adam skips a parameter without a gradient, while
    k_adam sees a zero gradient for GINet's dead attention parameters and decays them.  ``train_epoch`` answers None with
    weight decay (NeuralNet then steps mini-batch by mini-batch) and must change nothing."""
    tr, graphs, batch, rs = make_case(net_name, task, n_out, device, api, hyper)
    wd = hyper[3]
    tr.step.fill_(t0)                                 # as load_optimizer_state_dict does
    mask = live_mask(tr)
    if net_name == "GINet":
        assert not mask.all()
    ids = list(range(len(graphs)))
    if path == "fused":
        from deeprank_gnn_amd import _lib
        from deeprank_gnn_amd.topology import Topology
        topo = Topology.from_batch(batch, need_weights=(tr.kind == _lib.SGAT), api=api)
        assert tr._can_fuse(topo, 5, None, True, batch.x)
    for k in (1, 2):
        before = snapshot(tr)
        got = step_on_path(tr, path, batch, rs, ids)
        if path == "epoch" and wd != 0.0:
            assert got is None
            assert int(tr.step) == t0
            assert all(torch.equal(a, b) for a, b in zip(before, snapshot(tr)))
            continue
        assert got is not None
        assert int(tr.step) == t0 + k, "%s: step counter %d after %d steps from %d" % (path, int(tr.step), k, t0)
        assert bool(torch.isfinite(tr.loss).all())
        what = "%s %s %s step %d" % (net_name, task, path, k)
        assert_adam_step(before, tr.flat_g, snapshot(tr), t0 + k, hyper, mask=(mask if wd != 0.0 else None), what=what)
        g = tr.flat_g.detach().cpu().numpy()
        assert np.any(g[mask] != 0.0), what + ": the step left no gradient in flat_g"
        if wd == 0.0:
            dead = torch.from_numpy(~mask).to(tr.flat_p.device)
            assert all(torch.equal(a[dead], b[dead]) for a, b in zip(before, snapshot(tr))), what + ": dead parameters moved"
        else:
            assert not torch.equal(before[0], tr.flat_p)


def check_epoch_of_many(net_name, device, api, hyper):
    """train_epoch over 3 mini-batches of 2 graphs == three train_step_cached calls, bit for bit (parameters, both moments,
    step words): the lr / betas / eps copied into the epoch plan are the trainer's"""
    a, graphs, _, rs = make_case(net_name, "reg", 1, device, api, hyper, n_graphs=6)
    b = FusedTrainer(copy.deepcopy(a.net), lr=hyper[0], betas=hyper[1], eps=hyper[2], task="reg", seed=3, api=api)
    assert torch.equal(a.flat_p, b.flat_p)
    order = [4, 1, 5, 0, 2, 3]
    got = a.train_epoch(rs, order, 2, cached=True)
    assert got is not None
    cache = rs.topology_cache(need_weights=net_name == "sGAT")
    losses = [float(b.train_step_cached(cache, order[lo:lo + 2])) for lo in (0, 2, 4)]
    assert got[0].cpu().tolist() == losses
    for name in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.step2[:2].cpu().tolist() == b.step2[:2].cpu().tolist() == [3, 3]
    assert not torch.equal(a.exp_avg, torch.zeros_like(a.exp_avg))


# ---- resume ---------------------------------------------------------------------------------------------------------
def _torch_params(tr):
    """CPU copies of the net's parameters, in named_parameters order"""
    return [torch.nn.Parameter(p.detach().cpu().clone()) for p in tr.net.parameters()]


def _flat(tr, tensors):
    out = np.zeros(tr.flat_p.numel(), dtype=np.float32)
    for (name, p), t in zip(tr.net.named_parameters(), tensors):
        if t is not None:
            out[tr.offset[name]:tr.offset[name] + p.numel()] = t.detach().cpu().numpy().reshape(-1)
    return out


def check_resume(net_name, device, api):
    """(a) 3 steps, state into a fresh net and trainer, 3 more == 6 uninterrupted, bit for bit;  (b) the trainer's state
    resumed by torch.optim.Adam: its next step agrees with the trainer's within assert_adam_step's bounds (both sides against
    the same float64 reference; torch's ``value * t1 / t2`` order and its lerp stay inside c);  (c) a torch Adam state at
    step 7 with non-default lr / betas / eps resumed by the trainer: the next step uses t = 8 and those hyper-parameters."""
    hyper = HYPER[1]
    # (a)
    one, _, batch, _ = make_case(net_name, "reg", 1, device, api, hyper)
    twin = FusedTrainer(copy.deepcopy(one.net), lr=hyper[0], betas=hyper[1], eps=hyper[2], task="reg", seed=3, api=api)
    for _ in range(3):
        one.train_step(batch)
    fresh = NETS[net_name](5, 1, 1)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in one.net.state_dict().items()})
    if hasattr(fresh, "dropout"):
        fresh.dropout = 0.0
    two = FusedTrainer(fresh.to(device), task="reg", seed=3, api=api)
    two.load_optimizer_state_dict(one.optimizer_state_dict())
    assert (two.lr, tuple(two.betas), two.eps, two.weight_decay) == (hyper[0], hyper[1], hyper[2], 0.0)
    assert int(two.step) == 3
    for _ in range(3):
        two.train_step(batch)
    for _ in range(6):
        twin.train_step(batch)
    for name in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(two, name), getattr(twin, name)), "resumed run differs from the uninterrupted one: " + name
    assert int(two.step) == int(twin.step) == 6
    assert float(two.loss) == float(twin.loss)

    # (b) torch resumes the trainer
    params = _torch_params(twin)
    opt = torch.optim.Adam(params)
    opt.load_state_dict(twin.optimizer_state_dict())
    before = snapshot(twin)
    twin.train_step(batch)
    g = twin.flat_g.detach().cpu()
    for (name, p), q in zip(twin.net.named_parameters(), params):
        off = twin.offset[name]
        q.grad = g[off:off + p.numel()].reshape(p.shape).clone()
    opt.step()
    after_torch = (_flat(twin, params), _flat(twin, [opt.state[q]["exp_avg"] for q in params]),
                   _flat(twin, [opt.state[q]["exp_avg_sq"] for q in params]))
    assert all(int(float(opt.state[q]["step"])) == 7 for q in params)
    ref = assert_adam_step(before, g, after_torch, 7, hyper, what=net_name + " torch.optim.Adam resumed from the trainer")
    assert_adam_step(before, g, snapshot(twin), 7, hyper, what=net_name + " trainer, step 7")
    _, bm, bv = one_step_bounds(_f64(before[0]), _f64(before[1]), _f64(g), ref, hyper)
    for got, want, bound in zip(snapshot(twin)[1:], after_torch[1:], (bm, bv)):
        assert (np.abs(_f64(got) - _f64(want)) <= 2.0 * bound).all()

    # (c) the trainer resumes torch
    torch.manual_seed(5)
    net = NETS[net_name](5, 1, 1)
    if hasattr(net, "dropout"):
        net.dropout = 0.0
    lay = NetLayout(net)
    named = dict(net.named_parameters())
    live = {id(p) for name, p in named.items() if not any(off == lay.offset[name] for off, _ in lay.dead)}
    plist = list(net.parameters())
    theirs = (0.03, (0.8, 0.95), 1e-5, 0.0)
    opt = torch.optim.Adam(plist, lr=theirs[0], betas=theirs[1], eps=theirs[2])
    for _ in range(7):
        for p in plist:            # (no gradient, hence no state, for a parameter the net never uses: as in a reference run)
            p.grad = torch.randn_like(p) * 0.1 if id(p) in live else None
        opt.step()
    sd = opt.state_dict()
    for p in plist:
        p.grad = None
    tr, _, batch, _ = make_case(net_name, "reg", 1, device, api, HYPER[0], net=net)
    tr.load_optimizer_state_dict(sd)
    assert int(tr.step) == 7
    assert (tr.lr, tuple(tr.betas), tr.eps) == theirs[:3]
    m_theirs = _flat(tr, [opt.state[p]["exp_avg"] if p in opt.state else None for p in plist])
    assert np.array_equal(tr.exp_avg.cpu().numpy(), m_theirs) and np.any(m_theirs != 0.0)
    for path in ("fused", "pair"):
        t = int(tr.step)
        before = snapshot(tr)
        step_on_path(tr, path, batch, None, None)
        assert int(tr.step) == t + 1
        assert_adam_step(before, tr.flat_g, snapshot(tr), t + 1, theirs, what="%s resumed from torch, %s" % (net_name, path))
