"""tests/golden/metrics.npz: the reference's own Metrics (deeprank_gnn/Metrics.py, unmodified) on small cases.

Build-container only (needs /root/reference and sklearn; never runs on the GPU box).  The reference calls
``metrics.mean_squared_error(..., squared=...)``, a keyword sklearn 1.6 removed: a shim maps ``squared=False`` to
``root_mean_squared_error`` while the reference runs.  Per case the file holds the inputs, every attribute, the printed
lines and, where the predictions are distinct (so numpy's unstable argsort is the stable one), ``hitrate()`` / ``auc()``.

    python tests/golden/gen/make_metrics_golden.py
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import warnings

import numpy as np
import sklearn.metrics

REF = "/root/reference/deeprank_gnn/Metrics.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metrics.npz")
ATTRS = ("sensitivity", "specificity", "precision", "NPV", "FPR", "FNR", "FDR", "accuracy", "explained_variance",
         "max_error", "mean_abolute_error", "mean_absolute_error", "mean_squared_error", "root_mean_squared_error",
         "mean_squared_log_error", "median_squared_log_error", "r2_score")

_mse = sklearn.metrics.mean_squared_error


def _mse_with_squared(y_true, y_pred, squared=True, **kw):
    return _mse(y_true, y_pred, **kw) if squared else sklearn.metrics.root_mean_squared_error(y_true, y_pred, **kw)


def _reference():
    spec = importlib.util.spec_from_file_location("reference_metrics", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    rng = np.random.default_rng(20261015)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)      # network outputs are fp32
    out = []
    y = rng.uniform(0.0, 20.0, 2001)
    out.append(("irmsd_distinct", f32(np.abs(y + rng.normal(0.0, 2.0, y.size))), y, "irmsd", 4, True))
    y = rng.uniform(0.0, 1.0, 1500)
    out.append(("fnat_negative", f32(y + rng.normal(0.0, 0.1, y.size)), y, "fnat", 0.3, True))
    y = rng.uniform(0.0, 10.0, 800)
    p = f32(y + rng.normal(0.0, 1.0, y.size))
    p[17] = -1.5
    out.append(("irmsd_le_minus1", p, y, "irmsd", 4, True))
    y = rng.uniform(0.0, 1.0, 600)
    out.append(("dockQ", f32(y + rng.normal(0.0, 0.2, y.size)), y, "dockQ", 0.23, True))
    y = rng.integers(0, 2, 700).astype(np.float64)
    p = np.where(rng.uniform(size=y.size) < 0.8, y, 1 - y)
    out.append(("bin_class_binary", p, y, "bin_class", 0, True))
    out.append(("bin_class_classes", p, y, "bin_class", 0, False))
    out.append(("bio_interface_threshold1", p, y, "bio_interface", 1, True))
    y = rng.integers(1, 6, 900).astype(np.float64)
    p = np.clip(y + rng.integers(-1, 2, y.size), 0, 6).astype(np.float64)     # 0 and 6: not capri classes
    out.append(("capri_class_binary", p, y, "capri_class", 3, True))
    out.append(("capri_class_classes", p, y, "capri_class", 3, False))
    out.append(("n1", np.array([2.5]), np.array([3.0]), "irmsd", 4, True))
    out.append(("n2", np.array([2.5, 7.0]), np.array([3.0, 1.0]), "irmsd", 4, True))
    y = rng.uniform(0.0, 8.0, 1000)
    out.append(("even_n", f32(np.abs(y + rng.normal(0.0, 1.0, y.size))), y, "lrmsd", 4, True))
    out.append(("single_class_constant_y", f32(rng.uniform(0.0, 8.0, 300)), np.full(300, 2.0), "irmsd", 4, True))
    y = rng.uniform(5.0, 9.0, 400)
    out.append(("all_negative", f32(rng.uniform(0.0, 9.0, y.size)), y, "irmsd", 4, True))
    y = rng.uniform(0.0, 1.0, 5000)
    out.append(("fnat_ranking_5000", y + rng.normal(0.0, 0.3, y.size), y, "fnat", 0.3, True))
    return out


def main():
    ref = _reference()
    data = {}
    sklearn.metrics.mean_squared_error = _mse_with_squared
    try:
        for name, pred, y, target, thr, binary in cases():
            meta = {"target": target, "threshold": thr, "binary": binary}
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                m = ref.Metrics(pred.tolist(), y.tolist(), target, thr, binary)
                ranked = len(np.unique(pred)) == pred.size
                if ranked:
                    data[name + "/hitrate"] = np.asarray(m.hitrate(), dtype=np.int64)
                    data[name + "/auc"] = np.float64(m.auc())
            meta["printed"] = buf.getvalue().splitlines()
            meta["ranked"] = ranked
            meta["none"] = []
            for a in ATTRS:
                v = getattr(m, a, None)
                if v is None:
                    meta["none"].append(a)
                else:
                    data["%s/attr/%s" % (name, a)] = np.asarray(v, dtype=np.float64)
            data[name + "/pred"] = pred
            data[name + "/y"] = y
            data[name + "/meta"] = np.array(json.dumps(meta))
    finally:
        sklearn.metrics.mean_squared_error = _mse
    np.savez_compressed(OUT, **data)
    print("wrote", os.path.abspath(OUT), len(data), "arrays")


if __name__ == "__main__":
    main()
