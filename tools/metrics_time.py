"""Time the device Metrics (drgnn_metrics) next to the host reference on the same data.

usage: python tools/metrics_time.py [--sizes 10000,100000,1000000,4000000] [--repeats 5] [--out FILE]
Data: y uniform in [0, 10), fp32 predictions y + N(0, 2) on the device, target irmsd, threshold 4.
Device rows (HIP-synchronised wall clock, 2 warm-up calls, median over the repeats):
  kernels      the bare drgnn_metrics launch chain with counts, regression scores and ranking (buffers preallocated)
  get_metrics  Metrics(pred, y, 'irmsd', 4) + hitrate_tensor() + auc(): workspace allocation, the fp32 -> fp64
               conversion, both launch chains and the read-back of the scalars included, the hit rate left on the device
Host rows, same data copied to numpy: the reference's computation (sklearn's confusion_matrix and the eight regression
scores, np.argsort + np.cumsum for the hit rate, roc_auc_score of the argsort indices) where sklearn is installed, and
tests/metrics_ref.py (numpy only) always.  Needs the GPU: there is no fallback."""
import argparse
import contextlib
import io
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_ref as R                                        # noqa: E402
from deeprank_gnn_amd import _lib                              # noqa: E402
from deeprank_gnn_amd.metrics import Metrics                   # noqa: E402


def _median_time(fn, repeats, warm, sync):
    for _ in range(warm):
        fn()
    sync()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def sklearn_reference(p, y, thr):
    from sklearn import metrics
    yb, pb = (y < thr).astype(int), (p < thr).astype(int)
    metrics.confusion_matrix(yb, pb, labels=[0, 1])
    metrics.explained_variance_score(y, p)
    metrics.max_error(y, p)
    metrics.mean_absolute_error(y, p)
    metrics.mean_squared_error(y, p)
    metrics.root_mean_squared_error(y, p)
    if not ((y <= -1).any() or (p <= -1).any()):
        metrics.mean_squared_log_error(y, p)
    metrics.median_absolute_error(y, p)
    metrics.r2_score(y, p)
    idx = np.argsort(p)
    np.cumsum(yb[idx])
    metrics.roc_auc_score(yb, idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000,4000000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_time.txt"))
    args = ap.parse_args()
    api = _lib.get()
    sync = torch.cuda.synchronize
    try:
        import sklearn
        have_sk = sklearn.__version__
    except ImportError:
        have_sk = None
    lines = ["# drgnn_metrics on %s, torch %s; host reference: %s" % (
        torch.cuda.get_device_name(0), torch.__version__, "sklearn " + have_sk if have_sk else "no sklearn installed"),
        "# target irmsd, threshold 4, fp32 predictions; device: 2 warm-up calls, median of %d; host: median of %d"
        % (args.repeats, max(1, args.repeats // 2))]
    for n in [int(s) for s in args.sizes.split(",")]:
        rng = np.random.default_rng(n)
        y_h = rng.uniform(0.0, 10.0, n)
        p_h = (y_h + rng.normal(0.0, 2.0, n)).astype(np.float32)
        y = torch.from_numpy(y_h).cuda()
        p32 = torch.from_numpy(p_h).cuda()
        p = p32.to(torch.float64)
        ws = torch.empty(api.metrics_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        counts = torch.zeros(72, dtype=torch.int64, device="cuda")
        scores = torch.zeros(16, dtype=torch.float64, device="cuda")
        order = torch.empty(n, dtype=torch.int32, device="cuda")
        hits = torch.empty(n, dtype=torch.int64, device="cuda")
        what = _lib.METRICS_COUNTS | _lib.METRICS_REGRESSION | _lib.METRICS_RANKING

        def bare():
            api.metrics(p, y, n, what, -1, 4.0, 0, 0, ws, counts, scores, order, hits, _lib.current_stream(counts))

        def full():
            with contextlib.redirect_stdout(io.StringIO()):
                m = Metrics(p32, y, 'irmsd', 4)
            m.hitrate_tensor()
            m.auc()

        t_bare = _median_time(bare, args.repeats, 2, sync)
        t_full = _median_time(full, args.repeats, 2, sync)
        p64 = p_h.astype(np.float64)
        hr = max(1, args.repeats // 2)
        nothing = lambda: None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t_np = _median_time(lambda: (R.metrics(p64, y_h, 'irmsd', 4), R.ranking(p64, y_h, 'irmsd', 4)), hr, 0,
                                nothing)
            t_sk = _median_time(lambda: sklearn_reference(p64, y_h, 4.0), hr, 0, nothing) if have_sk else None
        row = "n %8d  device kernels %9.3f ms  get_metrics %9.3f ms  |  host numpy (metrics_ref) %9.3f ms" % (
            n, 1e3 * t_bare, 1e3 * t_full, 1e3 * t_np)
        row += ("  sklearn reference %9.3f ms" % (1e3 * t_sk)) if t_sk is not None else "  sklearn reference   n/a"
        lines.append(row)
        print(row, flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
