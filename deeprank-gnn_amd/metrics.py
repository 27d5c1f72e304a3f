"""Counterpart of the reference's ``deeprank_gnn.Metrics`` (Metrics.py): ``get_binary``, ``get_comparison`` and
``Metrics(prediction, y, target, threshold=4, binary=True)`` with the same attributes and methods, computed on the
device by ``drgnn_metrics`` (csrc/drgnn_metrics.h): the confusion counts and the regression sums in two reads of the
data, the median of |y - prediction| and the ranking by a stable radix sort, the hit rate by a scan.  The host turns the
returned counts and sums into the scores (a few scalar divisions).

Parity details (the reference on sklearn 1.7):

* 0 / 0 in a score is ``nan`` (the reference divides numpy integers: its ``try / except`` never fires); no
  RuntimeWarning is emitted.
* Regression scores exist for fnat / irmsd / lrmsd only; a NaN or an infinity in ``prediction`` or ``y`` then raises
  ``ValueError`` (sklearn's input check).  ``mean_squared_log_error`` stays ``None`` (and the reference's WARNING is
  printed) when a value is <= -1; ``median_squared_log_error`` holds the median ABSOLUTE error, ``mean_abolute_error``
  (sic) stays ``None``, both as in the reference.  ``explained_variance`` / ``r2_score`` follow sklearn's
  ``force_finite`` rule when var(y) == 0, and ``r2_score`` is ``nan`` for fewer than two samples.
* Ranking (``format_score``, ``hitrate``, ``auc``): ``np.argsort(prediction, kind='stable')``, reversed for fnat /
  bin_class.  For distinct predictions this is the reference's ranking; among TIES the reference's order depends on
  numpy's unstable introsort, here it is the stable order (equal predictions keep their index order; -0.0 ties +0.0;
  NaN ranks last in ascending order, as numpy puts it).
* ``auc()`` reproduces the reference as it is: ``roc_auc_score(gt_bool, idx)`` scores the ARGSORT INDICES, not the
  predictions.  Its closed form, evaluated here exactly, is ``(S + P - P (P + 1) / 2) / (P N)`` with
  ``S = sum(idx[i] for gt_bool[i] == 1)`` and P / N the positive / negative counts; ``nan`` with a single class.

``prediction`` / ``y`` may be lists, numpy arrays or torch tensors; a tensor already on the GPU is read in place
(converted to float64 on the device when it is not float64 already).  There is no CPU path.
"""
import math

import numpy as np
import torch

from . import _lib

__all__ = ["Metrics", "get_binary", "get_comparison"]

INVERSE = ('fnat', 'bin_class')            # 1 means value > threshold for these targets, value < threshold otherwise
REGRESSION = ('fnat', 'irmsd', 'lrmsd')    # targets that get the regression scores
_LABELS = {'capri_class': (1, 5), 'bin_class': (0, 2)}       # binary=False: (first label, number of labels)


def get_binary(values, threshold, target):
    """Metrics.get_binary: 1 for 'good' values (> threshold for fnat / bin_class, < threshold otherwise), else 0."""
    if target in INVERSE:
        return [1 if x > threshold else 0 for x in values]
    return [1 if x < threshold else 0 for x in values]


def get_comparison(prediction, ground_truth, binary=True, classes=[0, 1]):
    """Metrics.get_comparison: (FP, FN, TP, TN) from the confusion matrix of ``ground_truth`` (rows) against
    ``prediction`` (columns) over ``classes`` (pairs with a value outside them are left out, as sklearn's
    confusion_matrix does); class 1's numbers when ``binary``, else arrays over ``classes``.  Host helper."""
    cm = _confusion(np.asarray(ground_truth), np.asarray(prediction), list(classes))
    return _comparison(cm, binary)


def _confusion(y, p, classes):
    pos = {c: i for i, c in enumerate(classes)}
    cm = np.zeros((len(classes), len(classes)), dtype=np.int64)
    for a, b in zip(y.tolist(), p.tolist()):
        if a in pos and b in pos:
            cm[pos[a], pos[b]] += 1
    return cm


def _comparison(cm, binary):
    fp = cm.sum(axis=0) - np.diag(cm)
    fn = cm.sum(axis=1) - np.diag(cm)
    tp = np.diag(cm)
    tn = cm.sum() - (fp + fn + tp)
    if binary:
        return fp[1], fn[1], tp[1], tn[1]
    return fp, fn, tp, tn


def _force_finite(num, den):
    """sklearn's _assemble_r2_explained_variance with force_finite=True, one output"""
    if den != 0:
        return 1.0 - num / den
    return 1.0 if num == 0 else 0.0


def _values(v, device):
    """``v`` as a contiguous float64 vector on ``device`` (a tensor already there is used in place)"""
    if torch.is_tensor(v):
        t = v.detach()
        if t.device != device:
            t = t.to(device)
        return t.reshape(-1).to(torch.float64).contiguous()
    return torch.from_numpy(np.array(v, dtype=np.float64).reshape(-1)).to(device)


class Metrics(object):
    """Master class from which all metrics are computed (reference Metrics.py:67-240): the classification scores
    sensitivity, specificity, precision, NPV, FPR, FNR, FDR, accuracy; the regression scores explained_variance,
    max_error, mean_absolute_error, mean_squared_error, root_mean_squared_error, mean_squared_log_error,
    median_squared_log_error (the median absolute error), r2_score; ``auc()`` and ``hitrate()``.

    Args:
        prediction: predicted values (list, numpy array or torch tensor)
        y: target values
        target (str): irmsd, lrmsd, fnat, dockQ, capri_class, bin_class or a user target
        threshold: threshold that makes the values binary. Defaults to 4.
        binary (bool): binarise (default) or, for capri_class / bin_class, count the classes as they are.
    """

    def __init__(self, prediction, y, target, threshold=4, binary=True, api=None):
        self.prediction = prediction
        self.y = y
        self.binary = binary
        self.target = target
        self.threshold = threshold
        print('Threshold set to {}'.format(self.threshold))
        if binary:
            lo, k = 0, 0
        elif target in _LABELS:
            lo, k = _LABELS[target]
        else:
            raise ValueError('target must be capri_class on bin_class')
        if y is None:
            raise ValueError("Metrics needs the target values y")
        self._api = api or _lib.get()
        self._device = self._pick_device(prediction, y) if self._api is _lib._API else torch.device('cpu')
        self._pred, self._y = _values(prediction, self._device), _values(y, self._device)
        self.n = self._pred.numel()
        if self.n != self._y.numel():
            raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" %
                             (self._y.numel(), self.n))
        if self.n == 0:
            raise ValueError("Found array with 0 sample(s) while a minimum of 1 is required.")
        self._lo, self._k = lo, k
        self._dir = 1 if target in INVERSE else -1
        self._ranking = None
        regression = target in REGRESSION
        what = _lib.METRICS_COUNTS | (_lib.METRICS_REGRESSION if regression else 0)
        counts, scores, _, _ = self._launch(what)
        counts, scores = counts.cpu().numpy(), scores.cpu().numpy()

        kk = k or 2
        if not binary:
            if counts[0]:
                raise ValueError("Input contains NaN or infinity.")
            if counts[1]:
                raise ValueError("Classification metrics can't handle continuous targets")
            if counts[2] == 0:
                raise ValueError("At least one label specified must be in y_true")
        self.confusion_matrix = counts[8:8 + kk * kk].reshape(kk, kk).copy()
        fp, fn, tp, tn = _comparison(self.confusion_matrix, binary)
        with np.errstate(divide='ignore', invalid='ignore'):
            self.sensitivity = tp / (tp + fn)           # sensitivity, hit rate, recall, true positive rate
            self.specificity = tn / (tn + fp)           # specificity, true negative rate
            self.precision = tp / (tp + fp)             # precision, positive predictive value
            self.NPV = tn / (tn + fn)                   # negative predictive value
            self.FPR = fp / (fp + tn)                   # fall out, false positive rate
            self.FNR = fn / (tp + fn)                   # false negative rate
            self.FDR = fp / (tp + fp)                   # false discovery rate
            self.accuracy = (tp + tn) / (tp + fp + fn + tn)

        self.explained_variance = None
        self.max_error = None
        self.mean_abolute_error = None
        self.mean_absolute_error = None
        self.mean_squared_error = None
        self.root_mean_squared_error = None
        self.mean_squared_log_error = None
        self.median_squared_log_error = None
        self.r2_score = None
        if regression:
            if counts[0]:
                raise ValueError("Input contains NaN or infinity.")
            n = float(self.n)
            s = [float(v) for v in scores]
            self.explained_variance = _force_finite(s[9] / n, s[8] / n)
            self.max_error = s[6]
            self.mean_absolute_error = s[4] / n
            self.mean_squared_error = s[5] / n
            self.root_mean_squared_error = math.sqrt(s[5] / n)
            if s[0] <= -1 or s[1] <= -1:
                print("WARNING: Mean Squared Logarithmic Error cannot be used when "
                      "targets contain negative values.")
            else:
                self.mean_squared_log_error = s[7] / n
            self.median_squared_log_error = s[10]
            self.r2_score = float('nan') if self.n < 2 else _force_finite(s[5], s[8])

    @staticmethod
    def _pick_device(prediction, y):
        for v in (prediction, y):
            if torch.is_tensor(v) and v.is_cuda:
                return v.device
        return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')

    def _launch(self, what):
        api, dev, n = self._api, self._device, self.n
        if api is _lib._API:
            _lib.require_device(self._pred, self._y)
        ws = torch.empty(api.metrics_workspace_bytes(n), dtype=torch.uint8, device=dev)
        counts = torch.zeros(72, dtype=torch.int64, device=dev)
        scores = torch.zeros(16, dtype=torch.float64, device=dev)
        order = hits = None
        if what & _lib.METRICS_RANKING:
            order = torch.empty(n, dtype=torch.int32, device=dev)
            hits = torch.empty(n, dtype=torch.int64, device=dev)
        api.metrics(self._pred, self._y, n, what, self._dir, self.threshold, self._lo, self._k, ws, counts, scores,
                    order, hits, _lib.current_stream(counts))
        return counts, scores, order, hits

    def _rank(self):
        """(ascending stable argsort int32, hit rate int64, P, S) on the device, computed on first use"""
        if self._ranking is None:
            counts, _, order, hits = self._launch(_lib.METRICS_RANKING)
            c = counts[3:5].cpu().tolist()
            self._ranking = (order, hits, int(c[0]), int(c[1]))
        return self._ranking

    def format_score(self):
        """(idx, gt_bool): the ranking (``np.argsort(prediction, kind='stable')``, reversed for fnat / bin_class)
        and the binary targets, as numpy int64 arrays."""
        order = self._rank()[0].cpu().numpy().astype(np.int64)
        idx = order[::-1] if self.target in INVERSE else order
        y = self._y.cpu().numpy()
        gt = (y > self.threshold) if self.target in INVERSE else (y < self.threshold)
        return idx, gt.astype(np.int64)

    def hitrate(self):
        """The cumulative count of hits (binary target 1) along the ranking: numpy int64 [n]."""
        return self._rank()[1].cpu().numpy()

    def hitrate_tensor(self):
        """``hitrate()`` as the int64 device tensor it was computed in (no host copy)."""
        return self._rank()[1]

    def auc(self):
        """The reference's ``roc_auc_score(gt_bool, idx)`` (argsort indices as scores), exactly; nan for one class."""
        _, _, p, s = self._rank()
        neg = self.n - p
        if p == 0 or neg == 0:
            return float('nan')
        return (s + p - p * (p + 1) // 2) / (p * neg)
