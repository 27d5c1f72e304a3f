"""The kink arbiter of tests/elementwise.py (check_step_kinks) is not a loophole.  CPU only: each "kernel" is made from the
oracle (oracle/cpu_ref.py) on SYN64 (64 synthetic graphs of 200 nodes, 32 features), and the arbiter must accept exactly the
results that are the exact gradient of the network a few near decisions away -- and reject a far decision, or a gradient
element that no near decision explains."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from elementwise import (KINK_C, TOL, Lazy64, check_step, check_step_kinks, describe, flip_nudge, near_decisions,
                         oracle64)

NETS = ["GINet", "sGAT", "FoutNet"]
_CACHE = {}


def _fw(net):
    return {"looped": False} if net == "FoutNet" else {}


def _batch():
    if "batch" not in _CACHE:
        import deeprank_gnn_amd.synthetic as synth
        _CACHE["batch"] = synth.make_batch(0, 64)
    return _CACHE["batch"]


def _np(pred, loss, grads):
    return float(loss), pred.float().numpy(), {k: v.float().numpy() for k, v in grads.items()}


def _case(net, seed):
    """(params, fp32 oracle (loss, pred, grads) as numpy, float64 trace, Lazy64)."""
    key = (net, seed)
    if key not in _CACHE:
        batch = _batch()
        params = cpu_ref.init_params(net, 32, 1, 1, seed=seed)
        pred, loss, grads = cpu_ref.loss_and_grads(net, params, batch, batch.y, **_fw(net))
        trace = {}
        oracle64(net, params, batch, trace=trace, **_fw(net))
        _CACHE[key] = (params, _np(pred, loss, grads), trace)
    params, ref, trace = _CACHE[key]
    return params, ref, trace, Lazy64(net, params, _batch(), **_fw(net))


def _flipped(net, params, decisions):
    """The float64 oracle with ``decisions`` flipped, rounded to fp32: a kernel that took the other side of them."""
    batch = _batch()
    return _np(*oracle64(net, params, batch, nudge=flip_nudge(decisions), **_fw(net)))


def _arbiter(where, lazy, got, ref):
    return check_step_kinks(where, lazy, got[0], got[1], got[2], ref[0], ref[1], ref[2])


def _seed5_kink():
    """GINet, parameter seed 5: the one b.z2 pre-activation (7.8e-7, the maximum of its depth-1 cluster) whose side of zero
    the aggregation-first kernels and the fp32 reference disagree on (tools/r06/relu_kink_seed5.py)."""
    params, ref, trace, lazy = _case("GINet", 5)
    z = trace["b.z2"].detach().numpy()
    index = int(np.abs(z).argmin())
    near = [d for d in near_decisions(trace) if d["site"] == "b.z2" and d["index"] == index and d["kind"] == "zero"]
    assert len(near) == 1, describe(near_decisions(trace))
    assert abs(z.flat[index] - 7.75e-7) < 1e-9
    return params, ref, trace, lazy, near[0]


@pytest.mark.parametrize("net", NETS)
def test_fp32_oracle_is_accepted_against_float64(net):
    """The fp32 oracle as the kernel, judged with the float64 oracle as BOTH references (no fp32 slack), seeds 0-7."""
    for seed in range(8):
        params, ref, trace, lazy = _case(net, seed)
        p64, l64, g64 = lazy.get()
        report = _arbiter("%s seed %d" % (net, seed), lazy, ref, _np(p64, l64, g64))
        assert len(report["F"]) <= 1, describe(report["F"])


def test_seed5_b_z2_flip_is_accepted_and_named():
    params, ref, trace, lazy, kink = _seed5_kink()
    got = _flipped("GINet", params, [kink])
    with pytest.raises(AssertionError):                     # the strict rule cannot tell it from a wrong kernel ...
        check_step("seed 5", lazy, got[0], got[1], got[2], ref[0], ref[1], ref[2])
    report = _arbiter("seed 5", lazy, got, ref)             # ... the arbiter accepts it, on exactly that decision
    assert not report["strict"]
    assert report["F"] == [kink], describe(report["F"])
    assert report["F"][0]["margin"] < 0.05 * report["F"][0]["beta"]


def _far(trace, kind, site):
    """The decision of ``kind`` at ``site`` with the smallest margin above 100 beta."""
    wide = [d for d in near_decisions(trace, c=200 * KINK_C) if d["kind"] == kind and d["site"] == site]
    far = [d for d in wide if d["margin"] > 0.5 * d["beta"]]          # (d["beta"] is 200 beta)
    assert far, site
    return min(far, key=lambda d: d["margin"] / d["beta"])


@pytest.mark.parametrize("with_near", [False, True])
@pytest.mark.parametrize("kind,site", [("zero", "a.z2"), ("tie", "b.z2"), ("tie", "a.z1")])
def test_far_decision_is_rejected(kind, site, with_near):
    """A ReLU flip / max-pool reroute whose margin is above 100 beta changes the result (the strict check fails), and the
    arbiter rejects it -- alone, and next to the near seed-5 flip that it does accept."""
    params, ref, trace, lazy, kink = _seed5_kink()
    far = _far(trace, kind, site)
    got = _flipped("GINet", params, [far] + ([kink] if with_near else []))
    with pytest.raises(AssertionError):
        check_step("far", lazy, got[0], got[1], got[2], ref[0], ref[1], ref[2])
    with pytest.raises(AssertionError) as info:
        _arbiter("far %s" % describe([far]), lazy, got, ref)
    if with_near:
        assert "(flipped [b.z2 zero graph 19" in str(info.value), str(info.value)   # F was found; its verification rejects


def _deltas(lazy, trace):
    """Per near decision: {gradient name: float64 Delta of its flip}."""
    base = lazy.get()[2]
    out = []
    for dec in near_decisions(trace):
        batch = _batch()
        n, p = lazy.args[0], lazy.args[1]
        g = oracle64(n, p, batch, nudge=flip_nudge([dec]), **lazy.fw)[2]
        out.append({k: (g[k] - base[k]).numpy() for k in base})
    return out


@pytest.mark.parametrize("where", ["outside", "inside"])
def test_moved_gradient_element_is_rejected(where):
    """The seed-5 flip (accepted above), plus ONE gradient element moved by 3x its tolerance: outside the support of every near
    decision's Delta, and inside the seed-5 flip's support (where it moves the most) but not matching it."""
    params, ref, trace, lazy, kink = _seed5_kink()
    got = _flipped("GINet", params, [kink])
    deltas = _deltas(lazy, trace)
    names = sorted(got[2])
    reach = {k: np.max([np.abs(d[k]) for d in deltas], axis=0).reshape(-1) for k in names}
    if where == "outside":
        name = "conv1.fc.weight"
        i = int(np.argmin(reach[name]))
        assert reach[name][i] < 1e-3 * TOL
        step = 3.0
    else:
        name = "conv1_ext.fc.weight"
        kd = deltas[[j for j, d in enumerate(near_decisions(trace)) if d == kink][0]][name].reshape(-1)
        i = int(np.argmax(np.abs(kd)))
        assert abs(kd[i]) > 3 * (TOL + TOL * abs(ref[2][name].flat[i]))
        step = 3.0 * np.sign(kd[i])            # (got already carries the flip: moved past it, the same way)
    g = got[2][name].copy()
    g.flat[i] += step * (TOL + TOL * abs(g.flat[i]))
    moved = (got[0], got[1], dict(got[2], **{name: g}))
    _arbiter("unmoved", lazy, got, ref)
    with pytest.raises(AssertionError) as info:
        _arbiter("moved %s" % where, lazy, moved, ref)
    assert name in str(info.value), str(info.value)


@pytest.mark.parametrize("net", NETS)
def test_nudge_is_inert_when_empty(net):
    batch = _batch()
    params = cpu_ref.init_params(net, 32, 1, 1, seed=3)
    for dtype in (torch.float32, torch.float64):
        p = {k: v.to(dtype) for k, v in params.items()}
        outs = []
        for nudge in (None, {}):
            b = batch.clone()
            if dtype == torch.float64:
                b.x, b.edge_attr, b.y = b.x.double(), b.edge_attr.double(), b.y.double()
            trace = {}
            outs.append((cpu_ref.loss_and_grads(net, p, b, b.y, trace=trace, nudge=nudge, **_fw(net)), trace))
        (pa, la, ga), ta = outs[0]
        (pb, lb, gb), tb = outs[1]
        assert torch.equal(pa, pb) and torch.equal(la, lb)
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k
        assert sorted(ta) == sorted(tb) and "hid" in ta
        for k in ta:
            assert torch.equal(ta[k], tb[k]), k


def test_nudge_moves_only_its_pre_activation():
    batch = _batch()
    params = cpu_ref.init_params("GINet", 32, 1, 1, seed=3)
    t0 = {}
    oracle64("GINet", params, batch, trace=t0)
    for site, idx, delta, same in (("b.z2", [5, 70], [0.25, -0.5], ("a.z1", "a.z2", "b.z1")),
                                   ("hid", [3], [1.0], ("a.z1", "a.z2", "b.z1", "b.z2", "readout"))):
        t1 = {}
        oracle64("GINet", params, batch, trace=t1, nudge={site: (idx, delta)})
        d = (t1[site] - t0[site]).detach().reshape(-1)
        want = torch.zeros_like(d)
        want[idx] = torch.tensor(delta, dtype=d.dtype)
        assert torch.equal(d, want), site
        for k in same:
            assert torch.equal(t0[k], t1[k]), (site, k)
