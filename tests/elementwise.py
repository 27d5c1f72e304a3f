"""Element-wise float comparison used by every GPU parity test that touches a pinned golden or the oracle.

Rule (north_star: 1e-4 fp32):  |got - ref| <= 1e-4 + 1e-4 |ref|  for EVERY element -- no scaling by the tensor's
maximum.  fp32 caveat, stated rather than hidden: a gradient element is a sum of ~10^4 products; the reference
(torch CPU fp32) and the kernel associate that sum differently, so an element that is a cancellation residue may differ
by more than 1e-4 of the ELEMENT while both sit within fp32 round-off of the exact value.  For an element that misses
the strict test the same oracle evaluated in float64 is the arbiter: the kernel must be within 1e-4 + 1e-4 |ref64| of
it, or at least as close to it as the fp32 reference itself is (x4) -- never looser than what fp32 arithmetic of the
reference can resolve.  The number of arbitrated elements is ASSERTED to stay below 0.1 % (assert_arbiter_rate).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref

TOL = 1e-4
ARBITER_MAX_FRACTION = 1e-3


def new_stats():
    return {"elements": 0, "arbiter": 0}


def oracle64(net_name, params, batch_cpu, target=None, task="reg", trace=None, **fw):
    """(pred, loss, grads) of oracle/cpu_ref.py evaluated in float64 on the same inputs (the arbiter)."""
    p64 = {k: v.double() for k, v in params.items()}
    b64 = batch_cpu.clone()
    for key in ("x", "edge_attr", "pos", "y", "internal_edge_attr"):
        v = getattr(b64, key, None)
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(b64, key, v.double())
    tgt = b64.y if target is None else target
    if torch.is_tensor(tgt) and tgt.is_floating_point():
        tgt = tgt.double()
    if trace is not None:
        fw = dict(fw, trace=trace)
    return cpu_ref.loss_and_grads(net_name, p64, b64, tgt, task=task, **fw)


def check(name, got, ref32, ref64_fn, stats):
    """got vs the fp32 reference element by element; ref64_fn() -> the float64 arbiter (evaluated lazily)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref32, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    nan_mismatch = np.isnan(got) != np.isnan(ref)
    assert not nan_mismatch.any(), "%s: NaN pattern differs at %s" % (name, np.argwhere(nan_mismatch)[:4].tolist())
    both = ~np.isnan(ref)
    bad = both & (np.abs(got - ref) > TOL + TOL * np.abs(ref))
    stats["elements"] += got.size
    if not bad.any():
        return
    ref64 = np.asarray(ref64_fn(), dtype=np.float64).reshape(ref.shape)
    err_kernel = np.abs(got - ref64)
    err_ref32 = np.abs(ref - ref64)
    ok = (err_kernel <= TOL + TOL * np.abs(ref64)) | (err_kernel <= 4.0 * err_ref32 + 1e-7)
    stats["arbiter"] += int(bad.sum())
    fail = bad & ~ok
    if fail.any():
        worst = int(np.argmax(np.where(fail, err_kernel, 0.0)))
        raise AssertionError("%s: element %d got %.9g, fp32 reference %.9g, fp64 oracle %.9g (%d of %d elements fail)" %
                             (name, worst, got.flat[worst], ref.flat[worst], ref64.flat[worst], int(fail.sum()), got.size))


def assert_arbiter_rate(stats, what=""):
    limit = max(1, int(ARBITER_MAX_FRACTION * stats["elements"]))
    assert stats["arbiter"] <= limit, ("%s: %d of %d elements needed the float64 arbiter (limit %d = 0.1 %%)" %
                                       (what, stats["arbiter"], stats["elements"], limit))


class Lazy64:
    """Evaluates the float64 oracle once, on first use."""

    def __init__(self, net_name, params, batch_cpu, target=None, task="reg", want_trace=False, **fw):
        self.args = (net_name, params, batch_cpu, target, task)
        self.fw = fw
        self.want_trace = want_trace
        self.trace = {} if want_trace else None
        self.val = None

    def get(self):
        if self.val is None:
            n, p, b, t, task = self.args
            self.val = oracle64(n, p, b, target=t, task=task, trace=self.trace, **self.fw)
        return self.val

    def pred(self):
        return self.get()[0].numpy()

    def loss(self):
        return float(self.get()[1])

    def grad(self, k):
        return self.get()[2][k].numpy()

    def traced(self, k):
        self.get()
        return self.trace[k].detach().numpy()


def check_step(where, lazy, loss, pred, grads, ref_loss, ref_pred, ref_grads, stats=None):
    """loss / predictions / every gradient of one training step vs (ref_*) with `lazy` as the arbiter."""
    own = stats is None
    stats = new_stats() if own else stats
    check(where + " loss", float(loss), float(ref_loss), lazy.loss, stats)
    check(where + " pred", np.asarray(pred).reshape(-1), np.asarray(ref_pred).reshape(-1), lambda: lazy.pred().reshape(-1), stats)
    assert set(grads) == set(ref_grads), (sorted(grads), sorted(ref_grads))
    for k in sorted(grads):
        check(where + " grad " + k, grads[k], np.asarray(ref_grads[k]), lambda k=k: lazy.grad(k), stats)
    if own:
        assert_arbiter_rate(stats, where)
    return stats


# --------------------------------------------------------------------------------------------------------------------- #
# Kink-aware arbiter (opt-in; used by the SYN64 kink sweep of tests/test_gpu_parity.py)
#
# Two correct fp32 evaluations can take different sides of a non-smooth decision whose input sits within round-off of its
# switch point: a ReLU pre-activation near 0 that is also its pooling cell's maximum (z1 / z2 of each branch; every element
# of the head's fc1 output), or the top two members of a max-pool cell (cluster, channel) near a tie.  check_step_kinks
# accepts a step that fails check_step ONLY if the kernel's whole result matches, under the unchanged rule of `check`, the
# exact (float64) gradient of the network at a point at most beta away from the input, reached by flipping one to four such
# decisions.  Anything else still fails.
# --------------------------------------------------------------------------------------------------------------------- #

# beta = c * max |z64| over the channel of the batch.  Measured by tools/kink_beta.py over the sweep's seeds (SWEEP_SEEDS,
# SYN64): the fp32 oracle's worst pre-activation error, relative to that scale, is 5.1e-7 at the pooled sites z1 / z2
# (sGAT seed 3, a.z2), so KINK_C = 5e-6 is 9.7x it; at the head's fc1 output it is 2.3e-6 (FoutNet seed 3; a dot product of
# 32 / 64 terms over 64 graphs' channel maximum), and c may not exceed 1e-5, so KINK_C_HID = 1e-5 is 4.4x it.
KINK_C = 5e-6
KINK_C_HID = 1e-5
KINK_CAP = 64           # at most this many near decisions per case
KINK_MAX_FLIPS = 4      # at most this many flipped decisions
SWEEP_SEEDS = {"GINet": [0, 1, 2, 3, 4, 5, 6, 7, 11], "sGAT": [0, 1, 2, 3, 11], "FoutNet": [0, 1, 2, 3, 11]}


def _cells(z, cl):
    """Per (cell of ``cl``, channel): (top row, runner-up row or -1).  Ties keep the first row, as scatter_max does."""
    n, h = z.shape
    out = []
    for j in range(h):
        order = np.lexsort((-z[:, j], cl))
        cs = cl[order]
        starts = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
        size = np.r_[starts[1:], n] - starts
        top = order[starts]
        second = np.where(size >= 2, order[np.minimum(starts + 1, n - 1)], -1)
        out.append((j, cs[starts], top, second))
    return out


def near_decisions(trace, c=KINK_C, c_hid=KINK_C_HID):
    """The near set K of a float64 trace: a list of decisions, each a dict with site, kind ('zero' / 'tie'), graph, cluster
    (None for the head), channel, the flat index and additive delta of its flip, margin and beta."""
    out = []

    def add(site, kind, graph, cluster, channel, index, delta, margin, beta):
        out.append({"site": site, "kind": kind, "graph": int(graph), "cluster": None if cluster is None else int(cluster),
                    "channel": int(channel), "index": int(index), "delta": float(delta), "margin": float(margin),
                    "beta": float(beta)})

    for tag in sorted({k[:2] for k in trace if k.endswith("z1")}):
        pool_batch = trace[tag + "pool_batch"].numpy()
        cl0 = trace[tag + "cluster0"].numpy()
        for site, cl, graph_of in ((tag + "z1", cl0, lambda r, cl0=cl0: pool_batch[cl0[r]]),
                                   (tag + "z2", trace[tag + "cluster1"].numpy(), lambda r: pool_batch[r])):
            z = trace[site].detach().numpy()
            h = z.shape[1]
            beta = c * np.abs(z).max(axis=0)
            for j, cluster, top, second in _cells(z, cl):
                m1 = z[top, j]
                m2 = np.where(second >= 0, z[np.maximum(second, 0), j], -np.inf)
                for i in np.flatnonzero(np.abs(m1) <= beta[j]):
                    add(site, "zero", graph_of(top[i]), cluster[i], j, top[i] * h + j,
                        -2.0 * m1[i] if m1[i] != 0.0 else beta[j], abs(m1[i]), beta[j])
                gap = m1 - m2
                for i in np.flatnonzero((gap <= beta[j]) & (gap > 0.0) & (m1 > -beta[j])):
                    add(site, "tie", graph_of(top[i]), cluster[i], j, second[i] * h + j, 2.0 * gap[i], gap[i], beta[j])
    hid = trace["hid"].detach().numpy()
    beta = c_hid * np.abs(hid).max(axis=0)
    for g, j in np.argwhere(np.abs(hid) <= beta[None, :]):
        v = hid[g, j]
        add("hid", "zero", g, None, j, g * hid.shape[1] + j, -2.0 * v if v != 0.0 else beta[j], abs(v), beta[j])
    return out


def flip_nudge(decisions):
    """The oracle's ``nudge`` argument that flips every decision in ``decisions``."""
    nudge = {}
    for d in decisions:
        idx, delta = nudge.setdefault(d["site"], ([], []))
        idx.append(d["index"])
        delta.append(d["delta"])
    return nudge


def describe(decisions):
    return "[" + ", ".join("%s %s graph %d%s channel %d margin %.2g beta" % (
        d["site"], d["kind"], d["graph"], "" if d["cluster"] is None else " cluster %d" % d["cluster"], d["channel"],
        d["margin"] / d["beta"] if d["beta"] > 0 else 0.0) for d in decisions) + "]"


def _eval64(lazy, nudge=None, trace=None):
    n, p, b, t, task = lazy.args
    fw = dict(lazy.fw)
    if nudge is not None:
        fw["nudge"] = nudge
    pred, loss, grads = oracle64(n, p, b, target=t, task=task, trace=trace, **fw)
    out = {"loss": np.array([float(loss)]), "pred": pred.numpy().reshape(-1)}
    out.update({"grad " + k: v.numpy().reshape(-1) for k, v in grads.items()})
    return out


def check_step_kinks(where, lazy, loss, pred, grads, ref_loss, ref_pred, ref_grads, c=KINK_C, c_hid=KINK_C_HID):
    """check_step, and where it fails, the kink arbiter.  Same inputs as check_step (``lazy``: the float64 oracle of the same
    inputs).  Returns {"strict": did check_step pass, "arbiter": elements the float64 arbiter of `check` took, "K": near
    decisions, "F": the flipped decisions the acceptance rests on ([] when strict)}; raises AssertionError otherwise."""
    try:
        stats = check_step(where, lazy, loss, pred, grads, ref_loss, ref_pred, ref_grads)
        return {"strict": True, "arbiter": stats["arbiter"], "K": None, "F": []}
    except AssertionError as e:
        strict_msg = str(e)
    got = {"loss": np.array([float(loss)]), "pred": np.asarray(pred, dtype=np.float64).reshape(-1)}
    ref = {"loss": np.array([float(ref_loss)]), "pred": np.asarray(ref_pred, dtype=np.float64).reshape(-1)}
    assert set(grads) == set(ref_grads), (sorted(grads), sorted(ref_grads))
    for k in grads:
        got["grad " + k] = np.asarray(grads[k], dtype=np.float64).reshape(-1)
        ref["grad " + k] = np.asarray(ref_grads[k], dtype=np.float64).reshape(-1)
    for k in got:
        if (np.isnan(got[k]) != np.isnan(ref[k])).any():
            raise AssertionError(strict_msg)
    trace = {}
    r64 = _eval64(lazy, trace=trace)
    names = sorted(got)

    def failing(r):
        """Per name: the elements that fail `check`'s rule with float64 arbiter ``r`` (fp32 reference moved by r - r64)."""
        out = {}
        for k in names:
            ref32 = ref[k] + (r[k] - r64[k])
            bad = np.abs(got[k] - ref32) > TOL + TOL * np.abs(ref32)
            err = np.abs(got[k] - r[k])
            ok = (err <= TOL + TOL * np.abs(r[k])) | (err <= 4.0 * np.abs(ref[k] - r64[k]) + 1e-7)
            out[k] = bad & ~ok & ~np.isnan(ref[k])
        return out

    fail0 = failing(r64)
    n_fail = sum(int(m.sum()) for m in fail0.values())
    near = near_decisions(trace, c, c_hid)
    head = "%s: check_step failed (%s); " % (where, strict_msg)
    assert len(near) <= KINK_CAP, head + "%d near decisions, more than the cap of %d" % (len(near), KINK_CAP)

    def dist(r):
        return sum(float(np.abs(got[k] - r[k])[fail0[k]].sum()) for k in names)

    d0 = dist(r64)
    kept = []
    for dec in near:
        r = _eval64(lazy, nudge=flip_nudge([dec]))
        # kept: it brings failing elements within tolerance by moving them more than the tolerance itself (not by the small
        # change of every element that the flip's 2 |z| <= 2 beta change of the forward causes), more of them than it moves
        # passing elements out of tolerance, and the failing elements closer overall
        moved = {k: np.abs(r[k] - r64[k]) > TOL + TOL * np.abs(r64[k]) for k in names}
        within = {k: np.abs(got[k] - r[k]) <= TOL + TOL * np.abs(r[k]) for k in names}
        fixed = sum(int((fail0[k] & moved[k] & within[k]).sum()) for k in names)
        broken = sum(int((~fail0[k] & moved[k] & ~within[k] & ~np.isnan(r[k])).sum()) for k in names)
        if fixed > broken and dist(r) < d0:
            kept.append(dec)
    assert kept, head + "%d elements fail and no flip of the %d near decisions %s moves them toward the kernel" % (
        n_fail, len(near), describe(near))
    assert len(kept) <= KINK_MAX_FLIPS, head + "%d flips %s needed, more than %d" % (len(kept), describe(kept), KINK_MAX_FLIPS)
    rf = _eval64(lazy, nudge=flip_nudge(kept))
    stats = new_stats()
    for k in names:
        try:
            check("%s %s (flipped %s)" % (where, k, describe(kept)), got[k], ref[k] + (rf[k] - r64[k]), lambda k=k: rf[k], stats)
        except AssertionError as e:
            raise AssertionError(head + str(e))
    assert_arbiter_rate(stats, "%s (flipped %s)" % (where, describe(kept)))
    return {"strict": False, "arbiter": stats["arbiter"], "K": near, "F": kept}


def kink_line(where, report):
    """One summary line of a check_step_kinks case."""
    return "KINK %-40s strict=%-5s arbiter=%-4d F=%s" % (where, report["strict"], report["arbiter"], describe(report["F"]))
