"""Plain numpy statement of the reference's Metrics (deeprank_gnn/Metrics.py on sklearn 1.7) as this project defines it:
sklearn's formulas written out, the ranking by a stable argsort, the hit rate by cumsum and the AUC by its closed form.
No sklearn, no kernels: the device tests compare drgnn_metrics against this."""
import math

import numpy as np

INVERSE = ('fnat', 'bin_class')
REGRESSION = ('fnat', 'irmsd', 'lrmsd')
LABELS = {'capri_class': [1, 2, 3, 4, 5], 'bin_class': [0, 1]}
CLASS_ATTRS = ("sensitivity", "specificity", "precision", "NPV", "FPR", "FNR", "FDR", "accuracy")
REG_ATTRS = ("explained_variance", "max_error", "mean_absolute_error", "mean_squared_error", "root_mean_squared_error",
             "mean_squared_log_error", "median_squared_log_error", "r2_score")
EXACT = ("max_error", "median_squared_log_error")


def binary(values, threshold, target):
    v = np.asarray(values, dtype=np.float64)
    return ((v > threshold) if target in INVERSE else (v < threshold)).astype(np.int64)


def confusion(y, p, labels):
    pos = {c: i for i, c in enumerate(labels)}
    cm = np.zeros((len(labels), len(labels)), dtype=np.int64)
    for a, b in zip(np.asarray(y, dtype=np.float64).tolist(), np.asarray(p, dtype=np.float64).tolist()):
        if a in pos and b in pos:
            cm[pos[a], pos[b]] += 1
    return cm


def _force_finite(num, den):
    if den != 0:
        return 1.0 - num / den
    return 1.0 if num == 0 else 0.0


def metrics(prediction, y, target, threshold=4, binary_=True):
    """dict attribute -> value (None where the reference leaves None); 'printed': the lines Metrics prints"""
    p = np.asarray(prediction, dtype=np.float64)
    t = np.asarray(y, dtype=np.float64)
    out = {"printed": ["Threshold set to {}".format(threshold)]}
    if binary_:
        cm = confusion(binary(t, threshold, target), binary(p, threshold, target), [0, 1])
    else:
        cm = confusion(t, p, LABELS[target])
    fp = cm.sum(axis=0) - np.diag(cm)
    fn = cm.sum(axis=1) - np.diag(cm)
    tp = np.diag(cm)
    tn = cm.sum() - (fp + fn + tp)
    if binary_:
        fp, fn, tp, tn = fp[1], fn[1], tp[1], tn[1]
    with np.errstate(divide='ignore', invalid='ignore'):
        out.update(sensitivity=tp / (tp + fn), specificity=tn / (tn + fp), precision=tp / (tp + fp),
                   NPV=tn / (tn + fn), FPR=fp / (fp + tn), FNR=fn / (tp + fn), FDR=fp / (tp + fp),
                   accuracy=(tp + tn) / (tp + fp + fn + tn))
    for a in REG_ATTRS:
        out[a] = None
    out["mean_abolute_error"] = None
    if target in REGRESSION:
        if not (np.isfinite(p).all() and np.isfinite(t).all()):
            raise ValueError("Input contains NaN or infinity.")
        r = t - p
        n = t.size
        out["explained_variance"] = _force_finite(np.mean((r - np.mean(r)) ** 2), np.mean((t - np.mean(t)) ** 2))
        out["max_error"] = float(np.max(np.abs(r)))
        out["mean_absolute_error"] = float(np.mean(np.abs(r)))
        out["mean_squared_error"] = float(np.mean(r ** 2))
        out["root_mean_squared_error"] = math.sqrt(np.mean(r ** 2))
        if (t <= -1).any() or (p <= -1).any():
            out["printed"].append("WARNING: Mean Squared Logarithmic Error cannot be used when "
                                  "targets contain negative values.")
        else:
            out["mean_squared_log_error"] = float(np.mean((np.log1p(t) - np.log1p(p)) ** 2))
        out["median_squared_log_error"] = float(np.median(np.abs(r)))
        out["r2_score"] = float('nan') if n < 2 else _force_finite(np.sum(r ** 2), np.sum((t - np.mean(t)) ** 2))
    return out


def ranking(prediction, y, target, threshold):
    """(idx, gt_bool, hitrate, auc): stable argsort (reversed for fnat / bin_class), cumsum of gt_bool[idx] and the
    reference's roc_auc_score(gt_bool, idx) in closed form (exact integers, one division)"""
    idx = np.argsort(np.asarray(prediction, dtype=np.float64), kind='stable')
    if target in INVERSE:
        idx = idx[::-1]
    gt = binary(y, threshold, target)
    hits = np.cumsum(gt[idx], dtype=np.int64)
    p = int(gt.sum())
    neg = gt.size - p
    if p == 0 or neg == 0:
        return idx, gt, hits, float('nan')
    s = int(idx[gt == 1].astype(np.int64).sum())
    return idx, gt, hits, (s + p - p * (p + 1) // 2) / (p * neg)


def same(a, b, rtol=0.0):
    """equal, None to None, nan to nan, arrays elementwise; rtol 0 means bit-equal values"""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    if rtol == 0.0:
        return bool(np.array_equal(a, b, equal_nan=True))
    return bool(np.allclose(a, b, rtol=rtol, atol=0.0, equal_nan=True))
