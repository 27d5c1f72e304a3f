"""Decoupled weight decay (AdamW), gradient-norm clipping and learning-rate tables on every native training path, against
float64 restatements of torch's formulas.  The method is adam_check.py's: after a step the device holds the state before
(snapshot), the gradient the optimiser consumed (``flat_g``) and the state after, so each option is checked alone, a few
fp32 ulps from float64.  Shared by the emulated (CPU) and the MI355X tests: every check takes ``device`` and ``api``.

The bounds (``u = 2**-24``, ``c = 16``, ``TINY`` as in adam_check), each an operation count:

    decay     p_dec = p (1 - lr_t w) in float64; the moments on assert_adam_step's lines with wd = 0 (the gradient is not
              touched); |p' - ref(p_dec, m', v')| <= 3 u |p| + c u |p_dec - ref| + TINY: the cast of the factor, the
              product and the final difference are the 3 u |p|, the rest is adam_check's count.  Dead ranges keep their
              bits (parameters and both moments); a live element with g = m = v = 0 decays.
    clipping  a twin without clipping takes the same step: its flat_g is the unclipped g (same kernels, same bits).
              N64 = sqrt(sum g^2) in numpy float64; |grad_norm - N64| <= 2 u N64 (the fp32 store; the double chain is far
              below u).  c = 0.5 N64 (active): |flat_g - g s64| <= 2 u |g| s64 + TINY (the cast of s, one product);
              c = 2 N64 (inactive): flat_g bit-equal to the twin's.  assert_adam_step holds as it stands on the flat_g left.
    schedule  step k passes assert_adam_step with lr = table[min(t, n) - 1].
"""
import copy

import numpy as np
import torch

import adam_check as ac
from adam_check import C, GUARD, SENTINEL, TINY, U, _f64
from deeprank_gnn_amd import _lib
from deeprank_gnn_amd.data import Batch
from deeprank_gnn_amd.resident import ResidentGraphSet
from deeprank_gnn_amd.trainer import FusedTrainer, schedule_from_torch

BASE = (0.01, (0.9, 0.999), 1e-8)                    # lr, betas, eps
DECAY = 0.05
TABLE = [0.02, 0.013, 0.007, 0.004, 0.0025]          # 5 distinct rates
OPTIONS = ["decay", "clip_active", "clip_inactive", "schedule", "schedule_late"]


# ---- float64 references --------------------------------------------------------------------------------------------
def assert_adamw_step(before, g, after, t, lr, betas, eps, w, mask=None, what=""):
    """One AdamW update (decoupled decay ``w``, learning rate ``lr`` of this step) that used gradient ``g``."""
    p, m, v = (_f64(a) for a in before)
    p1, m1, v1 = (_f64(a) for a in after)
    g = _f64(g)
    hyper0 = (lr, betas, eps, 0.0)
    ref = ac.adam_ref64(p, m, v, g, t, lr, betas, eps, 0.0)
    _, bm, bv = ac.one_step_bounds(p, m, g, ref, hyper0)
    p_dec = p * (1.0 - lr * w)
    p_ref = ac.update_ref64(p_dec, m1, v1, t, lr, betas, eps)
    bp = 3.0 * U * np.abs(p) + C * U * np.abs(p_dec - p_ref) + TINY
    sel = np.ones(p.shape, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    for name, got, want, bound in (("exp_avg", m1, ref[1], bm), ("exp_avg_sq", v1, ref[2], bv), ("param", p1, p_ref, bp)):
        assert np.isfinite(got).all(), "%s: %s is not finite" % (what, name)
        err = np.abs(got - want)
        bad = sel & ~(err <= bound)
        if bad.any():
            i = int(np.argmax(np.where(bad, err / bound, 0.0)))
            raise AssertionError("%s: %s off at %d of %d elements, t=%d lr=%r w=%r; worst at [%d]: got %.9g want %.9g, error "
                                 "%.3g = %.1f x the bound (p=%.9g g=%.9g)" % (what, name, int(bad.sum()), int(sel.sum()), t, lr,
                                                                             w, i, got[i], want[i], err[i], err[i] / bound[i],
                                                                             p[i], g[i]))
    # a live element at rest decays, and by the factor alone
    idle = sel & (g == 0.0) & (m == 0.0) & (v == 0.0) & (p != 0.0)
    if w != 0.0 and idle.any():
        assert (p1[idle] != p[idle]).all(), what + ": a live element with zero gradient and moments did not decay"


def bits_equal(a, b):
    a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def assert_clip(g_unclipped, g_left, norm_word, c, what=""):
    """``g_left``: what the step left in flat_g; ``norm_word``: the float it left in grad_norm.  Returns True when active."""
    g = _f64(g_unclipped)
    N64 = float(np.sqrt(np.sum(g * g)))
    got = float(_f64(norm_word).reshape(-1)[0])
    print("%s: grad_norm %.9g, float64 %.9g, off by %.3g u" % (what, got, N64, abs(got - N64) / (U * N64)))
    assert abs(got - N64) <= 2.0 * U * N64, "%s: grad_norm %.9g against %.9g" % (what, got, N64)
    s64 = c / (N64 + 1e-6)
    assert abs(s64 - 1.0) > 0.25, "the threshold must leave no doubt about the branch"
    if s64 >= 1.0:
        assert bits_equal(g_left, g_unclipped), what + ": an inactive clip changed the gradient"
        return False
    err = np.abs(_f64(g_left) - g * s64)
    bound = 2.0 * U * np.abs(g) * s64 + TINY
    print("%s: clipped gradient worst %.3g x the bound" % (what, float(np.max(err / bound))))
    assert (err <= bound).all(), "%s: clipped gradient off, worst %.3g x the bound" % (what, float(np.max(err / bound)))
    return True


# ---- the flat kernel alone -------------------------------------------------------------------------------------------
class Record(object):
    """a drgnn_optim record over buffers of ``device`` (kept alive here)"""

    def __init__(self, api, device, n, lr=BASE[0], betas=BASE[1], eps=BASE[2], weight_decay=0.0, decoupled=False,
                 max_grad_norm=None, table=None, dead=()):
        o = self.o = _lib.Optim()
        o.lr, o.beta1, o.beta2, o.eps = lr, betas[0], betas[1], eps
        o.weight_decay, o.decoupled = weight_decay, int(decoupled)
        self.norm = torch.full((1 + GUARD,), SENTINEL, dtype=torch.float32, device=device)
        if table is not None:
            self.table = torch.tensor(table, dtype=torch.float64).to(device)
            o.lr_table, o.lr_n = self.table.data_ptr(), len(table)
        if max_grad_norm is not None:
            cap = api.optim_norm_words(n)
            self.cap = cap
            self.words = torch.full((cap + GUARD,), SENTINEL, dtype=torch.float64, device=device)
            o.clip, o.max_grad_norm, o.norm_words, o.norm_cap = 1, max_grad_norm, self.words.data_ptr(), cap
            o.norm_out = self.norm.data_ptr()
        o.n_dead = len(dead)
        for i, (off, ln) in enumerate(dead):
            o.dead_off[i], o.dead_len[i] = off, ln

    def assert_guards(self):
        assert bool((self.norm[1:] == SENTINEL).all()), "the norm word's neighbours were written"
        if hasattr(self, "words"):
            assert bool((self.words[self.cap:] == SENTINEL).all()), "norm words written behind the scratch"


def _flat_state(rng, n, t0, device):
    p0 = rng.standard_normal(n).astype(np.float32)
    if t0 == 0:
        m0, v0 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        g0 = ac.synthetic_gradient(rng, n)
        m0 = (g0 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
        v0 = (np.maximum(np.abs(g0), 1e-15) * rng.uniform(0.1, 3.0, n)).astype(np.float32) ** 2

    def guarded(a):
        buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=device)
        buf[:n] = torch.from_numpy(a)
        return buf
    return guarded(p0), guarded(m0), guarded(v0)


def _assert_flat_guards(n, bufs):
    for name, buf in bufs:
        assert bool((buf[n:] == SENTINEL).all()), "adam_step_opt wrote behind %s[%d]" % (name, n)


def check_flat_decay(device, api, n, t0=0):
    """drgnn_adam_step_opt, AdamW: three steps on synthetic buffers; a dead range in the middle keeps its bits (gradient
    included), elements at rest decay; guards untouched"""
    lr, betas, eps = BASE
    rng = np.random.default_rng(77 + n)
    P, M, V = _flat_state(rng, n, t0, device)
    dead = [(n // 3, max(n // 5, 1))] if n >= 3 else []
    mask = np.ones(n, dtype=bool)
    for off, ln in dead:
        mask[off:off + ln] = False
    rec = Record(api, device, n, weight_decay=DECAY, decoupled=True, dead=dead)
    G = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=device)
    step = torch.full((1,), t0, dtype=torch.int32, device=device)
    for k in range(1, 4):
        g = ac.synthetic_gradient(rng, n)
        before = tuple(a[:n].clone() for a in (P, M, V))
        ac.assert_above_underflow(g, before[0].cpu().numpy(), (lr, betas, eps, 0.0))
        G[:n] = torch.from_numpy(g)
        step.fill_(t0 + k)
        api.adam_step_opt(P[:n], G[:n], M[:n], V[:n], step, rec.o, ac._stream(P))
        after = tuple(a[:n].clone() for a in (P, M, V))
        if t0 == 0 and k == 1 and n >= 255:
            # synthetic_gradient's zeros at zero moments: the "a live element at rest decays" line of assert_adamw_step has
            # elements to look at
            assert (mask & (g == 0.0)).any()
        assert_adamw_step(before, g, after, t0 + k, lr, betas, eps, DECAY, mask=mask, what="adam_step_opt n=%d step %d" % (n, k))
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), before, after):
            assert bits_equal(a.cpu().numpy()[~mask], b.cpu().numpy()[~mask]), "dead range of %s changed" % name
        assert bits_equal(G[:n], g), "AdamW touched the gradient"
        if mask.any():
            assert not bits_equal(before[0].cpu().numpy()[mask], after[0].cpu().numpy()[mask])
    _assert_flat_guards(n, (("param", P), ("exp_avg", M), ("exp_avg_sq", V), ("grad", G)))
    rec.assert_guards()
    assert int(step) == t0 + 3


def check_flat_clip(device, api, n, active, t0=1):
    """drgnn_adam_step_opt with clipping on synthetic buffers: the norm launch (one word per 256 elements) + the Adam launch"""
    lr, betas, eps = BASE
    hyper = (lr, betas, eps, 0.0)
    rng = np.random.default_rng(1234 + n)
    P, M, V = _flat_state(rng, n, t0, device)
    g = ac.synthetic_gradient(rng, n)
    if not np.any(g):
        g[0] = np.float32(0.37)
    N64 = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    c = (0.5 if active else 2.0) * N64
    rec = Record(api, device, n, max_grad_norm=c)
    G = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=device)
    G[:n] = torch.from_numpy(g)
    step = torch.full((1,), t0 + 1, dtype=torch.int32, device=device)
    before = tuple(a[:n].clone() for a in (P, M, V))
    api.adam_step_opt(P[:n], G[:n], M[:n], V[:n], step, rec.o, ac._stream(P))
    after = tuple(a[:n].clone() for a in (P, M, V))
    what = "adam_step_opt clip n=%d" % n
    assert assert_clip(g, G[:n], rec.norm[:1], c, what) == active
    ac.assert_above_underflow(G[:n].cpu().numpy(), before[0].cpu().numpy(), hyper)
    ac.assert_adam_step(before, G[:n], after, t0 + 1, hyper, what=what)
    _assert_flat_guards(n, (("param", P), ("exp_avg", M), ("exp_avg_sq", V), ("grad", G)))
    rec.assert_guards()


def check_flat_schedule(device, api, n, t0):
    """drgnn_adam_step_opt with a table: 7 steps from ``t0``, step t uses table[min(t, 5) - 1] whatever ``lr`` says"""
    _, betas, eps = BASE
    rng = np.random.default_rng(99 + n)
    P, M, V = _flat_state(rng, n, t0, device)
    rec = Record(api, device, n, lr=123.0, table=TABLE)
    G = torch.zeros(n, dtype=torch.float32, device=device)
    step = torch.full((1,), t0, dtype=torch.int32, device=device)
    for k in range(1, 8):
        t = t0 + k
        hyper = (TABLE[min(t, len(TABLE)) - 1], betas, eps, 0.0)
        g = ac.synthetic_gradient(rng, n)
        before = tuple(a[:n].clone() for a in (P, M, V))
        ac.assert_above_underflow(g, before[0].cpu().numpy(), hyper)
        G.copy_(torch.from_numpy(g))
        step.fill_(t)
        api.adam_step_opt(P[:n], G, M[:n], V[:n], step, rec.o, ac._stream(P))
        ac.assert_adam_step(before, g, tuple(a[:n].clone() for a in (P, M, V)), t, hyper, what="table n=%d t=%d" % (n, t))
    _assert_flat_guards(n, (("param", P), ("exp_avg", M), ("exp_avg_sq", V)))


# ---- a real step on every path ---------------------------------------------------------------------------------------
def make_case(net_name, task, n_out, device, api, n_graphs=3, seed=0, net=None, **options):
    """adam_check.make_case with the optimiser options as constructor keywords"""
    torch.manual_seed(seed)
    graphs = ac.small_graphs(n_graphs)
    if task == "class":
        for i, g in enumerate(graphs):
            g.y = torch.tensor([i % n_out])
    if net is None:
        net = ac.NETS[net_name](5, n_out, 1)
    if hasattr(net, "dropout"):
        net.dropout = 0.0
    lr, betas, eps = BASE
    tr = FusedTrainer(net.to(device), lr=lr, betas=betas, eps=eps, task=task, seed=3, api=api, **options)
    batch = Batch.from_data_list(graphs).to(device)
    rs = ResidentGraphSet(graphs, device, api=api)
    if task == "class":
        rs.set_targets(torch.tensor([i % n_out for i in range(n_graphs)]))
    return tr, graphs, batch, rs


def _step(tr, path, batch, rs, ids, t):
    got = ac.step_on_path(tr, path, batch, rs, ids)
    assert got is not None, path + ": the native path refused a configuration it must take"
    assert int(tr.step) == t, "%s: step counter %d, expected %d" % (path, int(tr.step), t)
    assert bool(torch.isfinite(tr.loss).all())


def check_path_option(net_name, device, api, path, option, task="reg", n_out=1):
    lr, betas, eps = BASE
    what = "%s %s %s %s" % (net_name, task, path, option)
    if option == "decay":
        tr, graphs, batch, rs = make_case(net_name, task, n_out, device, api, weight_decay=DECAY, decoupled_weight_decay=True)
        mask = ac.live_mask(tr)
        dead = torch.from_numpy(~mask).to(tr.flat_p.device)
        ids = list(range(len(graphs)))
        for k in (1, 2):
            before = ac.snapshot(tr)
            _step(tr, path, batch, rs, ids, k)
            after = ac.snapshot(tr)
            assert_adamw_step(before, tr.flat_g, after, k, lr, betas, eps, DECAY, mask=mask, what=what)
            assert all(torch.equal(a[dead], b[dead]) for a, b in zip(before, after)), what + ": dead parameters changed"
            assert np.any(tr.flat_g.cpu().numpy()[mask] != 0.0)
        return
    if option in ("clip_active", "clip_inactive"):
        twin, graphs, batch, rs = make_case(net_name, task, n_out, device, api)
        net = copy.deepcopy(twin.net)
        ids = list(range(len(graphs)))
        _step(twin, path, batch, rs, ids, 1)
        g = twin.flat_g.detach().cpu().numpy().copy()
        N64 = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        c = (0.5 if option == "clip_active" else 2.0) * N64
        tr, _, batch, rs = make_case(net_name, task, n_out, device, api, net=net, max_grad_norm=c)
        before = ac.snapshot(tr)
        _step(tr, path, batch, rs, ids, 1)
        assert assert_clip(g, tr.flat_g, tr.grad_norm, c, what) == (option == "clip_active")
        ac.assert_adam_step(before, tr.flat_g, ac.snapshot(tr), 1, (lr, betas, eps, 0.0), what=what)
        if option == "clip_inactive":
            assert all(torch.equal(a, b) for a, b in zip(ac.snapshot(tr), ac.snapshot(twin)))
        return
    t0 = 999 if option == "schedule_late" else 0
    tr, graphs, batch, rs = make_case(net_name, task, n_out, device, api, lr_schedule=TABLE)
    tr.step.fill_(t0)
    ids = list(range(len(graphs)))
    for k in range(1, 8 if t0 == 0 else 3):
        t = t0 + k
        before = ac.snapshot(tr)
        _step(tr, path, batch, rs, ids, t)
        assert tr.lr_at(t) == TABLE[min(t, 5) - 1]
        ac.assert_adam_step(before, tr.flat_g, ac.snapshot(tr), t, (TABLE[min(t, 5) - 1], betas, eps, 0.0), what=what)


# ---- all three together ------------------------------------------------------------------------------------------------
def all_options(net_name, device, api, n_graphs=3):
    """keywords of a trainer with the three options on, the clipping threshold half the first step's norm (active)"""
    probe, graphs, batch, _ = make_case(net_name, "reg", 1, device, api, n_graphs=n_graphs)
    probe.train_step(batch)
    N64 = float(np.sqrt(np.sum(probe.flat_g.detach().cpu().numpy().astype(np.float64) ** 2)))
    return dict(weight_decay=DECAY, decoupled_weight_decay=True, max_grad_norm=0.5 * N64, lr_schedule=TABLE)


def assert_same_state(a, b, what=""):
    for name in ("flat_p", "exp_avg", "exp_avg_sq", "flat_g"):
        assert torch.equal(getattr(a, name), getattr(b, name)), "%s: %s differs" % (what, name)
    assert a.step2[:2].cpu().tolist() == b.step2[:2].cpu().tolist()


def check_epoch_of_many(net_name, device, api):
    """train_epoch over 3 mini-batches of 2 == three train_step_cached calls, bit for bit, all options on"""
    opts = all_options(net_name, device, api, n_graphs=6)
    a, graphs, _, rs = make_case(net_name, "reg", 1, device, api, n_graphs=6, **opts)
    b = FusedTrainer(copy.deepcopy(a.net), lr=BASE[0], betas=BASE[1], eps=BASE[2], task="reg", seed=3, api=api, **opts)
    order = [4, 1, 5, 0, 2, 3]
    got = a.train_epoch(rs, order, 2, cached=True)
    assert got is not None
    cache = rs.topology_cache(need_weights=net_name == "sGAT")
    losses = [float(b.train_step_cached(cache, order[lo:lo + 2])) for lo in (0, 2, 4)]
    assert got[0].cpu().tolist() == losses
    assert_same_state(a, b, "epoch against cached steps")
    assert torch.equal(a.grad_norm, b.grad_norm) and float(a.grad_norm) > 0.0
    assert a.step2[:2].cpu().tolist() == [3, 3]
    # the rebuilt epoch: the same arithmetic on a topology built in the loop
    c = FusedTrainer(copy.deepcopy(b.net), lr=BASE[0], betas=BASE[1], eps=BASE[2], task="reg", seed=3, api=api, **opts)
    assert c.train_epoch(rs, order, 2) is not None and int(c.step) == 3


def check_resume(net_name, device, api):
    """3 steps, the state into a fresh net and trainer, 3 more == 6 uninterrupted, bit for bit; the dictionary carries the
    options and the rate of the next step; torch.optim.AdamW accepts it"""
    opts = all_options(net_name, device, api)
    one, _, batch, _ = make_case(net_name, "reg", 1, device, api, **opts)
    twin = FusedTrainer(copy.deepcopy(one.net), lr=BASE[0], betas=BASE[1], eps=BASE[2], task="reg", seed=3, api=api, **opts)
    for _ in range(3):
        one.train_step(batch)
    sd = one.optimizer_state_dict()
    group = sd["param_groups"][0]
    assert group["decoupled_weight_decay"] is True and group["max_grad_norm"] == opts["max_grad_norm"]
    assert group["lr_schedule"] == TABLE and group["initial_lr"] == BASE[0] and group["lr"] == TABLE[3]
    opt = torch.optim.AdamW([torch.nn.Parameter(p.detach().cpu().clone()) for p in one.net.parameters()])
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == TABLE[3] and opt.param_groups[0]["weight_decay"] == DECAY
    fresh = ac.NETS[net_name](5, 1, 1)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in one.net.state_dict().items()})
    if hasattr(fresh, "dropout"):
        fresh.dropout = 0.0
    two = FusedTrainer(fresh.to(device), task="reg", seed=3, api=api)
    two.load_optimizer_state_dict(sd)
    assert (two.lr, two.weight_decay, two.decoupled_weight_decay, two.max_grad_norm, two.lr_schedule) == (
        BASE[0], DECAY, True, opts["max_grad_norm"], TABLE)
    for _ in range(3):
        two.train_step(batch)
    for _ in range(6):
        twin.train_step(batch)
    assert_same_state(two, twin, "resumed against uninterrupted")
    assert int(two.step) == 6 and float(two.loss) == float(twin.loss)
    # a torch AdamW state loads as decoupled decay
    theirs = torch.optim.AdamW([torch.nn.Parameter(p.detach().cpu().clone()) for p in one.net.parameters()], lr=0.02,
                               weight_decay=0.1).state_dict()
    two.load_optimizer_state_dict(theirs)
    assert (two.lr, two.weight_decay, two.decoupled_weight_decay, two.max_grad_norm, two.lr_schedule) == (0.02, 0.1, True, None, None)
    # a default trainer's dictionary is unchanged
    plain = FusedTrainer(ac.NETS[net_name](5, 1, 1).to(device), task="reg", seed=3, api=api)
    keys = set(plain.optimizer_state_dict()["param_groups"][0])
    assert not keys & {"decoupled_weight_decay", "max_grad_norm", "lr_schedule", "initial_lr"}


def check_schedule_from_torch():
    """the helper records the group's rate before each optimiser step; ``every`` = mini-batches per epoch"""
    t = schedule_from_torch(lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=2, gamma=0.5), 0.01, 7)
    assert t == [0.01, 0.01, 0.005, 0.005, 0.0025, 0.0025, 0.00125]
    t = schedule_from_torch(lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.1), 1.0, 6, every=3)
    np.testing.assert_allclose(t, [1.0, 1.0, 1.0, 0.1, 0.1, 0.1], rtol=1e-15)


# ---- against torch end to end ----------------------------------------------------------------------------------------
def check_five_steps_against_torch(net_name, device, api, build):
    """the 5-step loop of test_five_native_steps_match_oracle_training with torch.optim.AdamW(weight_decay=0.05),
    clip_grad_norm_ and a StepLR on the torch side; that test's tolerances.  ``build(net_name, params)``: the net on
    ``device`` with dropout 0."""
    import torch.nn.functional as F
    import deeprank_gnn_amd.synthetic as synth
    from oracle import cpu_ref
    batch_cpu = synth.make_batch(0, 16, n_nodes=120, n_pairs=260)
    params = cpu_ref.init_params(net_name, 32, 1, 1, seed=9)
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.AdamW(list(leaves.values()), lr=0.01, weight_decay=0.05)
    make = lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=2, gamma=0.5)        # noqa: E731
    sched = make(opt)
    table = schedule_from_torch(make, 0.01, 5)
    kw = {"looped": False} if net_name == "FoutNet" else {}
    # the threshold: half the first gradient's norm, so that clipping acts
    pred = cpu_ref.FORWARD[net_name](leaves, batch_cpu, **kw)
    F.mse_loss(pred.reshape(-1), batch_cpu.y).backward()
    max_norm = 0.5 * float(torch.sqrt(sum((v.grad.double() ** 2).sum() for v in leaves.values() if v.grad is not None)))
    tr = FusedTrainer(build(net_name, params), lr=0.01, task="reg", api=api, weight_decay=0.05, decoupled_weight_decay=True,
                      max_grad_norm=max_norm, lr_schedule=table)
    batch = batch_cpu.clone().to(device)
    dead = [name for name in leaves if any(off == tr.offset[name] for off, _ in tr.layout.dead)]
    assert bool(dead) == (net_name == "GINet")
    clipped = 0
    for it in range(5):
        opt.zero_grad()
        pred = cpu_ref.FORWARD[net_name](leaves, batch_cpu, **kw)
        loss = F.mse_loss(pred.reshape(-1), batch_cpu.y)
        loss.backward()
        # the oracle's forward runs GINet's attention branch op for op, so autograd hands its parameters a gradient that is
        # identically zero where the reference trainer's model leaves None: as there, torch must skip them
        for name in dead:
            assert not leaves[name].grad.any()
            leaves[name].grad = None
        total = torch.nn.utils.clip_grad_norm_(list(leaves.values()), max_norm)
        assert opt.param_groups[0]["lr"] == table[it]
        opt.step()
        sched.step()
        got = tr.train_step(batch)
        np.testing.assert_allclose(float(got), float(loss.detach()), rtol=1e-4)
        np.testing.assert_allclose(float(tr.grad_norm), float(total), rtol=1e-4)
        clipped += float(total) > max_norm
    assert clipped >= 1
    sd = tr.net.state_dict()
    for k, v in leaves.items():
        np.testing.assert_allclose(sd[k].cpu().numpy(), v.detach().numpy(), rtol=1e-4, atol=1e-5, err_msg=k)


# ---- a recorded step (GPU only) -------------------------------------------------------------------------------------
def check_recorded_step(net_name, device, api, cached):
    """one step recorded into a hipGraph and replayed 4 times == 5 eager steps of a twin, bit for bit, all options on: the
    replays walk through the learning-rate table by the step words on the device"""
    opts = all_options(net_name, device, api)
    tr, graphs, batch, rs = make_case(net_name, "reg", 1, device, api, **opts)
    twin = FusedTrainer(copy.deepcopy(tr.net), lr=BASE[0], betas=BASE[1], eps=BASE[2], task="reg", seed=3, api=api, **opts)
    ids = list(range(len(graphs)))
    cache = rs.topology_cache(need_weights=net_name == "sGAT") if cached else None
    ids_dev = rs.upload_ids(np.asarray(ids, dtype=np.int32)) if cached else None

    def step(t):
        return t.train_step_cached(cache, ids, ids_dev) if cached else t.train_step(batch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(tr)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(tr)
    for _ in range(4):
        g.replay()
    torch.cuda.synchronize()
    for _ in range(5):
        step(twin)
    assert int(tr.step) == int(twin.step) == 5
    assert_same_state(tr, twin, "recorded against eager")
    assert torch.equal(tr.grad_norm, twin.grad_norm) and float(tr.loss) == float(twin.loss)


# ---- cohort ---------------------------------------------------------------------------------------------------------
TABLE_B = [0.015, 0.015, 0.003]


def check_cohort(net_name, device, api, expect_path):
    """K = 3 members with a decay (one 0), a clipping threshold (one None) and a table each (two different ones): every
    member bit-equal to a FusedTrainer of its own with the one-workgroup-per-graph layout; a member with an empty mini-batch in
    a step is untouched, its grad_norm word included"""
    from deeprank_gnn_amd import Cohort
    Net = ac.NETS[net_name]
    graphs = ac.small_graphs(6)
    probe, _, batch, _ = make_case(net_name, "reg", 1, device, api, n_graphs=6)
    probe.train_step(batch)
    c = 0.5 * float(np.sqrt(np.sum(probe.flat_g.detach().cpu().numpy().astype(np.float64) ** 2)))
    decay, clip, tables = [DECAY, 0.0, 0.02], [c, None, 4.0 * c], [TABLE, TABLE_B, TABLE]
    torch.manual_seed(21)
    sds = []
    for _ in range(3):
        net = Net(5, 1, 1)
        sds.append({k: v.clone() for k, v in net.state_dict().items()})
    rs = ResidentGraphSet(graphs, device, api=api)
    seeds = [40, 41, 42]
    coh = Cohort(Net, sds, lr=0.01, seeds=seeds, task="reg", device=device, api=api, weight_decay=decay,
                 decoupled_weight_decay=True, max_grad_norm=clip, lr_schedule=tables)
    for tr in coh.trainers:
        if hasattr(tr.net, "dropout"):
            tr.net.dropout = 0.0
    # member 1 (no decay, no clipping) sits out step 1; member 0 (decays, clips: its Adam step is the cohort's second launch)
    # sits out step 3 with a gradient, norm words and a grad_norm word left by its earlier steps; member 2 the last step
    rows = [[[0, 1, 2, 3], [4, 5, 1], [2, 0, 5, 3]],
            [[4, 5], [], [1, 2, 3]],
            [[1, 3, 5], [0, 2], [4, 0]],
            [[], [1, 2], [3]],
            [[2], [3, 4, 5, 0], [1, 5]],
            [[1, 2], [3], []]]

    def state(m):
        return (coh.params[m], coh.exp_avg[m], coh.exp_avg_sq[m], coh.grads[m], coh.step2[m], coh.grad_norm[m:m + 1],
                coh.losses[m:m + 1])
    cache = rs.topology_cache(need_weights=net_name == "sGAT")
    for s, row in enumerate(rows):
        before = [[t.detach().clone() for t in state(m)] for m in range(3)]
        coh.train_step(cache, row)
        assert coh.last_path == expect_path, coh.last_reason
        for m in range(3):
            if len(row[m]) == 0:
                assert all(torch.equal(a, b) for a, b in zip(before[m], state(m))), \
                    "member %d without a mini-batch in step %d was touched" % (m, s)
                if m != 1:
                    assert float(before[m][5]) > 0.0 and bool(before[m][3].any())     # (there was something to disturb)
            else:
                assert not torch.equal(before[m][0], coh.params[m])
    assert coh.step2[:, 0].cpu().tolist() == [5, 5, 5]
    norms = coh.grad_norm.cpu().tolist()
    assert norms[0] > 0.0 and norms[1] == 0.0 and norms[2] > 0.0
    for m in range(3):
        net = Net(5, 1, 1)
        net.load_state_dict(sds[m])
        if hasattr(net, "dropout"):
            net.dropout = 0.0
        tr = FusedTrainer(net.to(device), lr=0.01, task="reg", seed=seeds[m], api=api, weight_decay=decay[m],
                          decoupled_weight_decay=True, max_grad_norm=clip[m], lr_schedule=tables[m])
        tr.plan_overrides = {"force_wgs": 1}
        for row in rows:
            if len(row[m]):
                tr.train_step_cached(cache, row[m])
        for name, mine in (("flat_p", coh.params[m]), ("exp_avg", coh.exp_avg[m]), ("exp_avg_sq", coh.exp_avg_sq[m]),
                           ("flat_g", coh.grads[m])):
            assert torch.equal(mine, getattr(tr, name)), "member %d: %s differs from a trainer of its own" % (m, name)
        assert torch.equal(coh.step2[m, :2], tr.step2[:2])
        assert torch.equal(coh.grad_norm[m:m + 1], tr.grad_norm) and torch.equal(coh.losses[m:m + 1], tr.loss)


# ---- coupled L2 with an option on -----------------------------------------------------------------------------------
def check_flat_coupled(device, api, n, t0=1):
    """drgnn_adam_step_opt with coupled weight decay (decoupled = 0) next to clipping and a table: the clipped gradient
    enters g + wd p as torch's Adam(weight_decay=) sees it after clip_grad_norm_, the rate is the table's; no dead ranges
    (coupled L2 decays every element, as drgnn_adam_step does)"""
    _, betas, eps = BASE
    rng = np.random.default_rng(4321 + n)
    P, M, V = _flat_state(rng, n, t0, device)
    G = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=device)
    step = torch.full((1,), t0, dtype=torch.int32, device=device)
    for k, active in ((1, True), (2, False)):
        t = t0 + k
        hyper = (TABLE[min(t, len(TABLE)) - 1], betas, eps, DECAY)
        g = ac.synthetic_gradient(rng, n)
        if float(np.sqrt(np.sum(g.astype(np.float64) ** 2))) < 1e-3:
            g[0] = np.float32(0.37)        # (the 1e-6 of c / (N + 1e-6) must not decide the branch)
        c = (0.5 if active else 2.0) * float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        rec = Record(api, device, n, lr=123.0, weight_decay=DECAY, decoupled=False, max_grad_norm=c, table=TABLE)
        G[:n] = torch.from_numpy(g)
        step.fill_(t)
        before = tuple(a[:n].clone() for a in (P, M, V))
        api.adam_step_opt(P[:n], G[:n], M[:n], V[:n], step, rec.o, ac._stream(P))
        what = "coupled + clip + table n=%d t=%d" % (n, t)
        assert assert_clip(g, G[:n], rec.norm[:1], c, what) == active
        ac.assert_above_underflow(G[:n].cpu().numpy(), before[0].cpu().numpy(), hyper)
        ac.assert_adam_step(before, G[:n], tuple(a[:n].clone() for a in (P, M, V)), t, hyper, what=what)
        rec.assert_guards()
    _assert_flat_guards(n, (("param", P), ("exp_avg", M), ("exp_avg_sq", V), ("grad", G)))


def check_path_coupled(net_name, device, api, path):
    """coupled L2 + clipping + a table on a trainer path: the sums launch, then the flat Adam launch; train_epoch still
    answers None and changes nothing.  Compared on the live parameters, as adam_check does for coupled decay; the dead ones
    decay too (no gradient: by wd p alone)."""
    _, betas, eps = BASE
    twin, graphs, batch, rs = make_case(net_name, "reg", 1, device, api)
    net = copy.deepcopy(twin.net)
    ids = list(range(len(graphs)))
    twin.train_step(batch)
    g = twin.flat_g.detach().cpu().numpy().copy()
    c = 0.5 * float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    tr, _, batch, rs = make_case(net_name, "reg", 1, device, api, net=net, weight_decay=DECAY, max_grad_norm=c, lr_schedule=TABLE)
    mask = ac.live_mask(tr)
    before = ac.snapshot(tr)
    got = ac.step_on_path(tr, path, batch, rs, ids)
    if path == "epoch":
        assert got is None and int(tr.step) == 0
        assert all(torch.equal(a, b) for a, b in zip(before, ac.snapshot(tr)))
        return
    what = "%s %s coupled + clip + table" % (net_name, path)
    assert int(tr.step) == 1
    if path != "pair":           # (the launch pair sums in another order: its unclipped gradient is not the twin's bits)
        assert assert_clip(g, tr.flat_g, tr.grad_norm, c, what)
    ac.assert_adam_step(before, tr.flat_g, ac.snapshot(tr), 1, (TABLE[0], betas, eps, DECAY), mask=mask, what=what)
    if not mask.all():
        dead = torch.from_numpy(~mask).to(tr.flat_p.device)
        assert not torch.equal(before[0][dead], tr.flat_p[dead]), what + ": coupled L2 must decay the dead parameters too"
