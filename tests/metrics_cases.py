"""Inputs and checks shared by tests/test_metrics.py (host emulation) and tests/test_gpu_metrics.py (the device): Metrics
(drgnn_metrics.h) against tests/metrics_ref.py in float64 at the sizes where a boundary of the code meets the edge of
the data, with keys whose eight bytes all vary.

SIZES are the smallest n at which each boundary exists: the wave (64), the workgroup (256), the second reduction
workgroup (2049), the radix / hit-rate tile (4096: n = 4097 leaves a tile with one valid lane, 8192 puts the two middle
elements of the median in different tiles) and a third, one-lane tile (12289).  The ranking inputs are random 64-bit
patterns read as doubles, so every pass of the LSD sort sees every digit in every wave, mixed with values that differ
in their low bytes only, so that the low passes decide the order, with the values whose keys take a branch of their
own (-0.0 / +0.0, NaN, the infinities) and runs of equal values across a wave and a tile boundary written in.  The
regression inputs keep the project's own range (sums of random bit patterns would overflow or cancel
and the tolerance would mean nothing) but carry full float64 mantissas.  Tolerances are those of tests/test_metrics.py.

Every reference is computed once per input and the inputs are read-only."""
import functools

import numpy as np

import metrics_ref as R

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 2048, 2049, 4095, 4096, 4097, 8192, 8193, 12289]
CLASS_SIZES = [257, 4097, 12289]
RANK_TARGETS = ("dockQ", "bin_class")          # ascending (dir = -1) and reversed (dir = +1)
REG_TARGETS = ("irmsd", "fnat")
TILE = 4096                                    # MT_TILE
RUN = (60, 70)                                 # ten equal predictions across the wave boundary at 64
RUN2 = (TILE - 5, TILE + 5)                    # ten across the tile boundary (n > 4097)


def wide(n, seed):
    """float64 [n] of random 64-bit patterns (both signs, denormals, every exponent); the non-finite draws replaced
    by standard normals"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64).copy()
    bad = ~np.isfinite(v)
    v[bad] = rng.standard_normal(int(bad.sum()))
    return v


def nested(n, seed):
    """float64 [n] of +-(1 + m 2^-52) with m < 2^(8 L) for a level L in 1..6 drawn per element: keys that agree in
    every digit from L up, so that digits 0..L-1, the low passes of the sort, decide their order (256 values per sign at
    L = 1: ties as well).  Random patterns alone do not do that: any two of them differ in a high byte already, and
    the later passes put right whatever order a low pass left, as long as it lost no element."""
    rng = np.random.default_rng(seed)
    level = rng.integers(1, 7, n).astype(np.uint64)
    m = rng.integers(0, 2 ** 48, n, dtype=np.uint64) & ((np.uint64(1) << (np.uint64(8) * level)) - np.uint64(1))
    sign = rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)
    return (np.uint64(0x3FF0000000000000) | m | sign).view(np.float64).copy()


def specials(n):
    """index -> value of the special predictions of an n > 70 ranking input.  +0.0 comes BEFORE -0.0: the stable order
    of the tie (+0.0 first) is then the opposite of the order of their bit patterns."""
    return {5: 0.0, n - 3: -0.0, 17: np.nan, 30: np.inf, n - 7: -np.inf}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def ranking_input(n):
    """(pred, y): wide values, about half of pred replaced by nested ones; for n > 70 the specials and the tie runs in
    pred"""
    pred, y = wide(n, 1000 + n), wide(n, 2000 + n)
    near = np.random.default_rng(5000 + n).random(n) < 0.5
    pred[near] = nested(n, 6000 + n)[near]
    if n > 70:
        pred[RUN[0]:RUN[1]] = pred[RUN[0]]
        if n > TILE + 1:
            pred[RUN2[0]:RUN2[1]] = pred[RUN2[0]]
        for i, v in specials(n).items():
            pred[i] = v
        assert np.count_nonzero(pred == 0.0) == 2 and np.count_nonzero(np.isnan(pred)) == 1
    return _frozen(pred, y)


@functools.lru_cache(maxsize=None)
def ranking_reference(n, target):
    pred, y = ranking_input(n)
    return R.ranking(pred, y, target, 0.0), R.metrics(pred, y, target, 0.0)


@functools.lru_cache(maxsize=None)
def regression_input(n, target):
    """(pred, y, threshold): y uniform on [0, 10), pred = y + N(0, 2), full mantissas; fnat: both / 10"""
    rng = np.random.default_rng(3000 + n)
    y = rng.uniform(0.0, 10.0, n)
    pred = y + rng.normal(0.0, 2.0, n)
    if target == "fnat":
        return _frozen(pred / 10.0, y / 10.0) + (0.3,)
    return _frozen(pred, y) + (4.0,)


@functools.lru_cache(maxsize=None)
def regression_reference(n, target):
    pred, y, thr = regression_input(n, target)
    return R.metrics(pred, y, target, thr)


@functools.lru_cache(maxsize=None)
def class_input(n):
    """(pred, y): integer labels 0..7 as float64; 0, 6 and 7 are outside capri_class's 1..5"""
    rng = np.random.default_rng(4000 + n)
    pred, y = rng.integers(0, 8, n).astype(np.float64), rng.integers(0, 8, n).astype(np.float64)
    inside = (y >= 1) & (y <= 5)
    assert inside.any() and (~inside).any()
    return _frozen(pred, y)


def _on(device, *arrays):
    if device is None or str(device) == "cpu":
        return arrays
    import torch
    return tuple(torch.tensor(a).to(device) for a in arrays)                       # (a copy: the inputs are read-only)


def _bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


def assert_stable_order(idx, n, reverse):
    """the special predictions in the returned ranking itself: NaN last, the infinities at the ends of the rest, the
    equal values in index order (ascending ranking; the reversed one turns the whole order round)"""
    asc = np.asarray(idx)[::-1] if reverse else np.asarray(idx)
    assert sorted(asc.tolist()) == list(range(n))
    if n <= 70:
        return
    at = {v if v == v else "nan": i for i, v in specials(n).items() if v != 0.0}
    assert asc[-1] == at["nan"] and asc[-2] == at[np.inf] and asc[0] == at[-np.inf], (asc[:2], asc[-2:])
    where = np.empty(n, dtype=np.int64)
    where[asc] = np.arange(n)
    assert where[n - 3] == where[5] + 1, (where[5], where[n - 3])                  # +0.0 (index 5), then -0.0
    runs = [RUN] + ([RUN2] if n > TILE + 1 else [])
    for lo, hi in runs:
        assert np.array_equal(where[lo:hi], where[lo] + np.arange(hi - lo)), (lo, where[lo:hi])


def check_ranking(n, target, api, device):
    """order, binary targets, hit rate and AUC against metrics_ref, all exact; returns the integer results"""
    from deeprank_gnn_amd.metrics import Metrics
    from test_metrics import attrs_of, check_attrs
    pred, y = ranking_input(n)
    (idx, gt, hits, auc), ref = ranking_reference(n, target)
    m = Metrics(*_on(device, pred, y), target, 0.0, api=api)
    fidx, fgt = m.format_score()
    np.testing.assert_array_equal(fidx, idx)
    np.testing.assert_array_equal(fgt, gt)
    np.testing.assert_array_equal(m.hitrate(), hits)
    assert m.hitrate().dtype == np.int64 and fidx.dtype == np.int64
    assert R.same(m.auc(), auc), (m.auc(), auc)
    assert_stable_order(fidx, n, target in R.INVERSE)
    check_attrs(attrs_of(m), ref)
    order, h, p, s = m._rank()
    return {"order": order.cpu().numpy().tobytes(), "hits": h.cpu().numpy().tobytes(), "P": p, "S": s,
            "confusion": m.confusion_matrix.tobytes()}


def check_regression(n, target, api, device):
    """the scores against metrics_ref (counts, max_error and the median exact, the sums to RTOL) and the median bit for
    bit against np.median; returns the results that are the same bits on both builds"""
    from deeprank_gnn_amd.metrics import Metrics
    from test_metrics import attrs_of, check_attrs
    pred, y, thr = regression_input(n, target)
    m = Metrics(*_on(device, pred, y), target, thr, api=api)
    check_attrs(attrs_of(m), regression_reference(n, target))
    res = np.sort(np.abs(y - pred))
    if n % 2 == 0:
        assert res[n // 2 - 1] != res[n // 2]                  # the two middle elements differ: both must be read
    assert _bits(m.median_squared_log_error) == _bits(np.median(np.abs(y - pred))), (m.median_squared_log_error, n)
    assert _bits(m.max_error) == _bits(res[-1])
    return {"confusion": m.confusion_matrix.tobytes(), "max_error": _bits(m.max_error),
            "median": _bits(m.median_squared_log_error)}


def check_classes(n, api, device):
    """the K x K matrix of capri_class (binary=False): the labels outside 1..5 left out, exactly"""
    from deeprank_gnn_amd.metrics import Metrics
    from test_metrics import attrs_of, check_attrs
    pred, y = class_input(n)
    m = Metrics(*_on(device, pred, y), "capri_class", 3, binary=False, api=api)
    want = R.confusion(y, pred, R.LABELS["capri_class"])
    inside = (y >= 1) & (y <= 5) & (pred >= 1) & (pred <= 5)
    assert m.confusion_matrix.shape == (5, 5) and m.confusion_matrix.dtype == np.int64
    np.testing.assert_array_equal(m.confusion_matrix, want)
    assert 0 < int(m.confusion_matrix.sum()) == int(inside.sum()) < n
    check_attrs(attrs_of(m), R.metrics(pred, y, "capri_class", 3, False))
    return {"confusion": m.confusion_matrix.tobytes()}


def check_repeat(api, device, n=12289):
    """two Metrics on one input: the same bits"""
    import torch
    from deeprank_gnn_amd.metrics import Metrics
    pred, y = _on(device, *ranking_input(n))
    for target in RANK_TARGETS:
        a, b = Metrics(pred, y, target, 0.0, api=api), Metrics(pred, y, target, 0.0, api=api)
        assert torch.equal(a.hitrate_tensor(), b.hitrate_tensor())
        assert torch.equal(a._rank()[0], b._rank()[0])
        assert _bits(a.auc()) == _bits(b.auc()) and a._rank()[2:] == b._rank()[2:]


def assert_same_results(dev, host):
    """what the device and the emulation must agree on bit for bit: the integers, max_error and the median (the other
    float scores go through log1p and the libraries differ: those are held to the reference only)"""
    assert sorted(dev) == sorted(host)
    for k in dev:
        assert dev[k] == host[k], k
