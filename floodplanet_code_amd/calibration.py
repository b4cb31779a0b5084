"""Operating point and calibration of a trained network, from one histogram of class probability against target class.

The device makes the histogram in one pass (fu_eval_prob_hist over the resident logits, fu_prob_hist over any fp32
probabilities; HipUNet.prob_histogram); everything here is integer arithmetic on it, on the host, in numpy.

The bin rule (include/floodunet.h states it, prob_histogram_host below is its specification): n_bins is a power of two,
s = p * n_bins in float32 is exact, bin = s >= 1 ? min(int(s), n_bins - 1) : 0.  Hence bin >= j exactly when
p >= j / n_bins in float32, and the thresholds j / n_bins are float32 numbers: the reversed cumulative sums of the
histogram are, count for count, what thresholding the float32 probabilities at T_j = j / n_bins gives (T_0 = 0 declares
every counted pixel).  A NaN or negative probability sits in bin 0, p >= 1 in the last bin.

hist: int64 [k, k, n_bins], hist[c, t, b] = #pixels with target t whose probability of class c falls in bin b.
top:  int64 [2, n_bins], row 1 = pixels whose argmax (first maximum) is the target, row 0 the others, binned by the
winning probability.  Both count the pixels whose target is neither ignore_index nor outside [0, k).
"""
from __future__ import annotations

import json
from typing import Optional, Tuple

import numpy as np

MAX_BINS = 1024
METRICS = ("f1", "iou")


def check_bins(n_bins: int) -> int:
    n_bins = int(n_bins)
    if n_bins < 2 or n_bins > MAX_BINS or n_bins & (n_bins - 1):
        raise ValueError(f"n_bins must be a power of two in 2..{MAX_BINS}, got {n_bins}")
    return n_bins


def prob_bins(p: np.ndarray, n_bins: int) -> np.ndarray:
    """The bin of each float32 probability (the rule of the module docstring), int64."""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p * np.float32(n_bins)
        inside = (s >= np.float32(1)) & (s < np.float32(n_bins))
        b = np.where(inside, s, np.float32(0)).astype(np.int64)       # the truncation of (int)s, on in-range values only
        return np.where(s >= np.float32(n_bins), n_bins - 1, b)       # NaN fails both tests: bin 0


def prob_histogram_host(probs, target, ignore_index: int, n_bins: int = 256) -> Tuple[np.ndarray, np.ndarray]:
    """The specification of fu_prob_hist / fu_eval_prob_hist: probs float32 [..., k], target integer [...] of the same
    leading shape -> (hist int64 [k, k, n_bins], top int64 [2, n_bins])."""
    n_bins = check_bins(n_bins)
    probs = np.asarray(probs, dtype=np.float32)
    k = probs.shape[-1]
    p = probs.reshape(-1, k)
    t = np.asarray(target).reshape(-1).astype(np.int64)
    if t.shape[0] != p.shape[0]:
        raise ValueError(f"prob_histogram_host: {p.shape[0]} pixels of probabilities, {t.shape[0]} of targets")
    valid = (t != int(ignore_index)) & (t >= 0) & (t < k)
    p, t = p[valid], t[valid]
    hist = np.zeros((k, k, n_bins), dtype=np.int64)
    for c in range(k):
        np.add.at(hist[c], (t, prob_bins(p[:, c], n_bins)), 1)
    pm = np.full(p.shape[0], -np.inf, dtype=np.float32)                # the argmax loop of the kernels: first maximum wins,
    am = np.zeros(p.shape[0], dtype=np.int64)                          # a NaN never does
    for c in range(k):
        with np.errstate(invalid="ignore"):
            better = p[:, c] > pm
        pm = np.where(better, p[:, c], pm)
        am = np.where(better, c, am)
    top = np.zeros((2, n_bins), dtype=np.int64)
    np.add.at(top, ((am == t).astype(np.int64), prob_bins(pm, n_bins)), 1)
    return hist, top


def _check_hist(hist, cls: int) -> Tuple[np.ndarray, int]:
    hist = np.asarray(hist)
    if hist.ndim != 3 or hist.shape[0] != hist.shape[1] or not np.issubdtype(hist.dtype, np.integer):
        raise ValueError(f"hist must be integer [k, k, n_bins], got {hist.dtype} {hist.shape}")
    check_bins(hist.shape[2])
    cls = int(cls)
    if not 0 <= cls < hist.shape[0]:
        raise ValueError(f"class {cls} not in 0..{hist.shape[0] - 1}")
    return hist.astype(np.int64), cls


def _ratio(num, den):
    """num / den in float64 where den > 0, else 0 (the convention of metrics.SegmentationMetrics for an empty class)."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.zeros_like(num), where=den > 0)


def curves(hist, cls: int) -> dict:
    """One-versus-rest sweep of class `cls` over the thresholds j / n_bins, j = 0..n_bins-1: "declare cls where
    p[cls] >= T".  Positives are the pixels with target cls (row cls of hist[cls]), negatives all other counted pixels.
    -> {"thresholds" float64 [n_bins]; "tp", "fp", "fn", "tn" int64 [n_bins] (exact: reversed cumulative sums);
    "precision", "recall", "f1", "iou" float64 [n_bins], 0 where the denominator is 0}."""
    hist, cls = _check_hist(hist, cls)
    n_bins = hist.shape[2]
    pos = hist[cls, cls]
    neg = hist[cls].sum(axis=0) - pos
    tp = np.cumsum(pos[::-1])[::-1]
    fp = np.cumsum(neg[::-1])[::-1]
    fn = pos.sum() - tp
    tn = neg.sum() - fp
    return {"thresholds": np.arange(n_bins, dtype=np.float64) / n_bins, "tp": tp, "fp": fp, "fn": fn, "tn": tn,
            "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn), "f1": _ratio(2 * tp, 2 * tp + fp + fn),
            "iou": _ratio(tp, tp + fp + fn)}


def best_threshold(hist, cls: int, metric: str = "f1") -> Tuple[float, float]:
    """-> (threshold, value): the threshold j / n_bins with the largest F1 ("f1") or IoU ("iou") of class cls; ties go
    to the threshold nearest 0.5, then to the smaller."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {list(METRICS)}, got {metric!r}")
    cv = curves(hist, cls)
    v, th = cv[metric], cv["thresholds"]
    tied = np.flatnonzero(v == v.max())
    j = min(tied, key=lambda i: (abs(th[i] - 0.5), th[i]))
    return float(th[j]), float(v[j])


def average_precision(hist, cls: int) -> float:
    """sum over operating points of (recall step) * precision, walking the thresholds from the largest down (recall
    rises from its value at (n_bins - 1) / n_bins, counted from 0, to 1 at threshold 0).  0 without positives."""
    cv = curves(hist, cls)
    rec, prec = cv["recall"][::-1], cv["precision"][::-1]
    return float(np.sum(np.diff(np.concatenate([[0.0], rec])) * prec))


def expected_calibration_error(top, groups: int = 15) -> float:
    """ECE of the argmax decision over `groups` equal-width confidence groups: sum_g n_g / N * |accuracy_g -
    confidence_g|.  A pixel's confidence is taken as the midpoint (b + 0.5) / n_bins of its bin b and the pixel goes to
    group min(int(midpoint * groups), groups - 1).  The midpoint is within 1 / (2 n_bins) of the pixel's probability, so
    each group's mean confidence is too, and for the same assignment of pixels to groups the result is within
    1 / (2 n_bins) of the ECE of the probabilities themselves (0.002 at 256 bins); pixels within that distance of a
    group edge may fall into the neighbouring group.  0 for an empty histogram."""
    top = np.asarray(top)
    if top.ndim != 2 or top.shape[0] != 2 or not np.issubdtype(top.dtype, np.integer):
        raise ValueError(f"top must be integer [2, n_bins], got {top.dtype} {top.shape}")
    n_bins = check_bins(top.shape[1])
    groups = int(groups)
    if groups < 1:
        raise ValueError(f"groups must be >= 1, got {groups}")
    n = top.sum(axis=0).astype(np.float64)
    total = n.sum()
    if total == 0:
        return 0.0
    mid = (np.arange(n_bins, dtype=np.float64) + 0.5) / n_bins
    g = np.minimum((mid * groups).astype(np.int64), groups - 1)
    n_g = np.bincount(g, weights=n, minlength=groups)
    hit_g = np.bincount(g, weights=top[1].astype(np.float64), minlength=groups)
    conf_g = np.bincount(g, weights=n * mid, minlength=groups)
    return float(np.abs(hit_g - conf_g).sum() / total)


def argmax_point(top, cls: int, confusion=None) -> Optional[dict]:
    """The argmax decision, for comparison with the sweep: its accuracy over the counted pixels (from top), and with the
    confusion counts of the same pixels (int [k, k], target row, argmax column: fu_eval_confusion summed over the crops)
    the one-versus-rest operating point of class cls under the argmax.  None without both."""
    out = {}
    if top is not None:
        top = np.asarray(top).astype(np.int64)
        n = int(top.sum())
        out.update(accuracy=float(top[1].sum() / n) if n else 0.0, n_pixels=n)
    if confusion is not None:
        m = np.asarray(confusion).astype(np.int64)
        tp = int(m[cls, cls])
        fp, fn = int(m[:, cls].sum()) - tp, int(m[cls, :].sum()) - tp
        out.update(tp=tp, fp=fp, fn=fn, tn=int(m.sum()) - tp - fp - fn, precision=float(_ratio(tp, tp + fp)),
                   recall=float(_ratio(tp, tp + fn)), f1=float(_ratio(2 * tp, 2 * tp + fp + fn)),
                   iou=float(_ratio(tp, tp + fp + fn)))
    return out or None


def report(hist, top, cls: int, confusion=None) -> dict:
    """JSON-ready summary for class cls: best thresholds, average precision, ECE, the operating points at 0.5 and at the
    best-F1 threshold, the argmax decision for comparison (argmax_point), the curves' integer counts and the histograms
    themselves."""
    hist, cls = _check_hist(hist, cls)
    n_bins = hist.shape[2]
    cv = curves(hist, cls)
    half = n_bins // 2
    t_f1, v_f1 = best_threshold(hist, cls, "f1")
    t_iou, v_iou = best_threshold(hist, cls, "iou")

    def point(j):
        return {"threshold": float(cv["thresholds"][j]), **{m: int(cv[m][j]) for m in ("tp", "fp", "fn", "tn")},
                **{m: float(cv[m][j]) for m in ("precision", "recall", "f1", "iou")}}

    out = {"class": cls, "n_bins": n_bins, "n_classes": int(hist.shape[0]), "n_pixels": int(hist[cls].sum()),
           "best_threshold": t_f1, "best_f1": v_f1, "best_iou_threshold": t_iou, "best_iou": v_iou,
           "average_precision": average_precision(hist, cls), "at_half": point(half),
           "at_best": point(int(round(t_f1 * n_bins))), "argmax": argmax_point(top, cls, confusion),
           "ece": None if top is None else expected_calibration_error(top),
           "curves": {m: cv[m].tolist() for m in ("tp", "fp", "fn", "tn")},
           "hist": hist.tolist(), "top": None if top is None else np.asarray(top).astype(np.int64).tolist()}
    return out


def read_calibration(path: str) -> Tuple[int, float]:
    """-> (class, best_threshold) of a calibration.json that predict --calibrate wrote."""
    with open(path) as fh:
        d = json.load(fh)
    try:
        cls, thr = int(d["class"]), float(d["best_threshold"])
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"{path} is not a calibration.json: it needs 'class' and 'best_threshold'") from None
    return cls, thr


def check_threshold(threshold, cls: int, n_classes: Optional[int] = None) -> Tuple[int, float]:
    """The checks of fu_stitch_finalize_maps_ex on the host, before any device work -> (cls, threshold)."""
    cls, threshold = int(cls), float(threshold)
    if not np.isfinite(threshold) or not 0.0 <= threshold <= 1.0:
        raise ValueError(f"threshold must be a finite number in [0, 1], got {threshold}")
    if cls < 0 or (n_classes is not None and (n_classes < 2 or cls >= n_classes)):
        raise ValueError(f"threshold class {cls} not in 0..{(n_classes or 0) - 1} (at least 2 classes)" if n_classes
                         is not None else f"threshold class {cls} is negative")
    return cls, threshold
