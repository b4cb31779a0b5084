"""Numpy reference of window-weighted stitching and of the fused finalisation, independent of the package: the window
formulas are restated here, and every step is one fp32 numpy operation, so each rounds on its own as the kernels'
arithmetic is specified to (fu_stitch_add_batch_windowed, fu_stitch_finalize_maps in include/floodunet.h)."""
import numpy as np


def window(kind, n):
    """float32 window of n samples, formed in float64 and rounded once."""
    i = np.arange(n).astype(np.float64)
    if kind == "uniform":
        w = np.ones(n)
    elif kind == "linear":
        w = np.minimum(i + 1.0, n - i) / float((n + 1) // 2)
    elif kind == "hann":
        w = np.square(np.sin(np.pi * (i + 0.5) / n))
    else:
        raise KeyError(kind)
    return w.astype(np.float32)


def softmax_crops(logits):
    """[n, c, h, w] logits -> fp32 [n, h, w, c] softmax, as oracle.stitch_reference forms it."""
    x = np.asarray(logits, dtype=np.float32).transpose(0, 2, 3, 1)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def stitch_blend_reference(probs, boxes, H, W, win_y, win_x, canvas=None, weight=None, eps=0.0):
    """probs: fp32 [n, th, tw, k] per-crop probabilities; boxes: (h0, w0, hE, wE) per crop, in table order.  Per crop:
    w = win_y[:dh, None] * win_x[None, :dw]; canvas[box] = canvas[box] + w * p; weight[box] = weight[box] + w, all fp32.
    -> (canvas / (weight + eps) with uncovered pixels 0, raw canvas, weight)."""
    probs = np.asarray(probs, dtype=np.float32)
    win_y, win_x = np.asarray(win_y, np.float32), np.asarray(win_x, np.float32)
    k = probs.shape[-1]
    canvas = np.zeros((H, W, k), np.float32) if canvas is None else canvas.astype(np.float32).copy()
    weight = np.zeros((H, W), np.float32) if weight is None else weight.astype(np.float32).copy()
    for p, (h0, w0, hE, wE) in zip(probs, boxes):
        dh, dw = hE - h0, wE - w0
        w = win_y[:dh, None] * win_x[None, :dw]
        canvas[h0:hE, w0:wE] = canvas[h0:hE, w0:wE] + w[..., None] * p[:dh, :dw]
        weight[h0:hE, w0:wE] = weight[h0:hE, w0:wE] + w
    s = weight + np.float32(eps)
    covered = s > 0
    inv = np.float32(1) / np.where(covered, s, np.float32(1))
    out = np.where(covered[..., None], canvas * inv[..., None], np.float32(0)).astype(np.float32)
    return out, canvas, weight


def quantize_unit(x):
    """(uint8) rint(min(max(x, 0), 1) * 255) in fp32."""
    x = np.asarray(x, dtype=np.float32)
    return np.rint(np.minimum(np.maximum(x, np.float32(0)), np.float32(1)) * np.float32(255)).astype(np.uint8)


def finalize_maps_reference(canvas, weight, eps, class_values=None):
    """fu_stitch_finalize_maps restated: canvas fp32 [H, W, k] raw sums, weight fp32 [H, W].
    -> dict(canvas=normalised fp32, argmax, cls=uint8 [H, W], probs=uint8 [k, H, W], margin=uint8 [H, W], counts=int64 [k])."""
    canvas, weight = np.asarray(canvas, np.float32), np.asarray(weight, np.float32)
    k = canvas.shape[-1]
    s = weight + np.float32(eps)
    covered = s > 0
    inv = (np.float32(1) / np.where(covered, s, np.float32(1))).astype(np.float32)
    v = np.where(covered[..., None], canvas * inv[..., None], np.float32(0)).astype(np.float32)
    am = np.where(covered, v.argmax(-1), 0)                      # argmax: the first maximum
    if k == 1:
        margin = v[..., 0]
    else:
        srt = np.sort(v, axis=-1)
        margin = srt[..., -1] - srt[..., -2]
    values = np.arange(k, dtype=np.uint8) if class_values is None else np.asarray(class_values, np.uint8)
    return {"canvas": v, "argmax": am, "cls": values[am], "probs": np.ascontiguousarray(quantize_unit(v).transpose(2, 0, 1)),
            "margin": quantize_unit(np.where(covered, margin, np.float32(0))),
            "counts": np.bincount(am[covered].ravel(), minlength=k).astype(np.int64)}
