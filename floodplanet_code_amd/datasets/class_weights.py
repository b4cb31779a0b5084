"""Class frequencies of the label rasters and the "balanced" class weights made from them.

Flood is a small share of the valid pixels of most chips, so the weighted cross entropy (HipUNet.loss(class_weight=...),
C ABI fu_loss_ce_weighted) wants weights that follow the class frequencies of the TRAIN split.  The counts are taken over
the boxes of the split's example list -- every pixel of every tile, overlapping tiles counted as often as they are trained
on -- with the data set's own label decode (raw 2 -> 1, raw 0 -> nodata_value, anything else -> 0):

  * `label_class_counts` on the device: one table of boxes of resident uint8 label rasters, one launch
    (fu_label_class_counts; integer arithmetic, exact).  SceneTileLoader.class_counts() calls it on the rasters it keeps.
  * `label_class_counts_host`: the same contract in numpy -- what the tests compare the device against and what the
    streaming loader's command line uses (its label rasters are on the host), NOT a fallback for the device call.
  * `balanced_class_weights(counts, ignore_index)`: w_c = N / (|S| * count_c) over the classes S that are not ignored and
    occur, 0 elsewhere (scikit-learn's "balanced" heuristic restricted to S)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

__all__ = ["label_class_counts", "label_class_counts_host", "balanced_class_weights", "dataset_label_boxes"]

Box = Tuple[int, int, int, int]         # h0, w0, hE, wE


def _check_box(i: int, shape, box, fn: str = "label_class_counts") -> Box:
    h0, w0, hE, wE = (int(v) for v in box)
    H, W = int(shape[0]), int(shape[1])
    if h0 < 0 or w0 < 0 or hE > H or wE > W:
        raise ValueError(f"{fn}: entry {i}: box [{h0}:{hE}, {w0}:{wE}] lies outside its raster {H}x{W}")
    if hE - h0 < 1 or wE - w0 < 1:
        raise ValueError(f"{fn}: entry {i}: box [{h0}:{hE}, {w0}:{wE}] is empty")
    return h0, w0, hE, wE


def _check_host_entries(entries, fn: str = "label_class_counts") -> List[Tuple[np.ndarray, Box]]:
    """The entry check both host statements share (label_class_counts_host, sampling.label_box_counts_host)."""
    checked = []
    for i, (label, box) in enumerate(entries):
        if label is None:
            raise ValueError(f"{fn}: entry {i}: no label raster")
        label = np.asarray(label)
        if label.dtype != np.uint8 or label.ndim != 2:
            raise ValueError(f"{fn}: entry {i}: the label must be uint8 [H, W], got {label.dtype} {label.shape}")
        checked.append((label, _check_box(i, label.shape, box, fn)))
    return checked


def _device_table(entries, fn: str = "label_class_counts"):
    """entries = [(uint8 label raster on the ROCm device, box), ...] -> (the fu_scene_train_entry table both device calls
    take, the device)."""
    from .. import _lib
    n = len(entries)
    if n < 1:
        raise ValueError(f"{fn}: no entries")
    dev = entries[0][0].device
    if dev.type != "cuda":
        raise RuntimeError(f"{fn} runs only on a ROCm GPU; the host statement is {fn}_host")
    table = (_lib.FuSceneTrainEntry * n)()
    for i, (label, (h0, w0, hE, wE)) in enumerate(entries):
        if label.dtype != torch.uint8 or label.dim() != 2 or not label.is_contiguous() or label.device != dev:
            raise ValueError(f"{fn}: entry {i}: the label must be contiguous uint8 [H, W] on {dev}, got "
                             f"{tuple(label.shape)} {label.dtype} on {label.device}")
        table[i] = _lib.FuSceneTrainEntry(None, label.data_ptr(), label.shape[0], label.shape[1], int(h0), int(w0), int(hE),
                                          int(wE), 0, 0.0)
    return table, dev


def label_class_counts_host(entries: Sequence[Tuple[np.ndarray, Box]], nodata_value: int, n_classes: int,
                            counts: Optional[np.ndarray] = None) -> np.ndarray:
    """entries: [(raw uint8 label raster [H, W], (h0, w0, hE, wE)), ...].  -> int64 [n_classes]: counts[d] += the pixels of
    the boxes that decode to d (raw 2 -> 1, raw 0 -> nodata_value, anything else -> 0) with 0 <= d < n_classes; other
    values are dropped.  `counts` is added to when given.  Every entry is checked before anything is counted."""
    n_classes, nodata_value = int(n_classes), int(nodata_value)
    if n_classes < 1 or len(entries) < 1:
        raise ValueError(f"label_class_counts: {len(entries)} entries, n_classes = {n_classes} (both must be >= 1)")
    checked = _check_host_entries(entries)
    out = np.zeros(n_classes, dtype=np.int64) if counts is None else counts
    for label, (h0, w0, hE, wE) in checked:
        raw = np.bincount(label[h0:hE, w0:wE].reshape(-1), minlength=256)
        for d, k in ((1, int(raw[2])), (nodata_value, int(raw[0])), (0, int(raw.sum() - raw[2] - raw[0]))):
            if 0 <= d < n_classes:
                out[d] += k
    return out


def label_class_counts(ctx, entries: Sequence[Tuple[torch.Tensor, Box]], nodata_value: int, n_classes: int,
                       counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C ABI fu_label_class_counts: entries = [(raw uint8 label raster [H, W] on the ROCm device, box), ...] -> int64
    [n_classes] on that device, ADDED to `counts` when given.  One launch for the whole table.  ctx: the fu_ctx whose table
    buffer the call borrows (HipUNet._get_ctx)."""
    from .. import _lib
    if ctx is None:
        raise ValueError("label_class_counts: no fu_ctx (run or prepare a forward first)")
    table, dev = _device_table(entries)
    n = len(entries)
    if counts is None:
        counts = torch.zeros(int(n_classes), dtype=torch.int64, device=dev)
    elif counts.dtype != torch.int64 or counts.numel() != int(n_classes) or not counts.is_contiguous() or counts.device != dev:
        raise ValueError(f"label_class_counts: counts must be contiguous int64 [{n_classes}] on {dev}")
    _lib.check(_lib.load().fu_label_class_counts(ctx, n, table, int(nodata_value), int(n_classes), counts.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream))
    return counts


def dataset_label_boxes(dataset) -> List[Tuple[np.ndarray, Box]]:
    """The (raw uint8 label raster, box) of every example of a FloodplanetTiles split, each label file decoded once: the
    rasters SceneTileLoader keeps on the device and the boxes it cuts, on the host."""
    from .resize import resize_image
    from .floodplanet import read_image
    rasters, out = {}, []
    for ex in dataset.dataset:
        cp = ex["crop_params"]
        H, W = cp.og_height, cp.og_width
        label = rasters.get(ex["label_path"])
        if label is None:
            label = np.asarray(read_image(ex["label_path"]))
            if label.shape != (H, W):
                label = resize_image(label, H, W, resize_mode="nearest")
            if label.dtype != np.uint8:      # only 0 and 2 are told apart from the rest: keep exactly that
                label = np.where(label == 2, 2, np.where(label == 0, 0, 1)).astype(np.uint8)
            label = rasters[ex["label_path"]] = np.ascontiguousarray(label)
        out.append((label, (cp.h0, cp.w0, min(cp.hE, H), min(cp.wE, W))))
    return out


def balanced_class_weights(counts, ignore_index: Optional[int]) -> np.ndarray:
    """counts [n_classes] -> fp32 [n_classes]: with S = the classes c != ignore_index whose count is > 0 and N = the sum of
    their counts, w_c = N / (|S| * count_c) for c in S and 0 elsewhere (computed in fp64, rounded once).  ignore_index: the
    model's -- None ignores nothing, -1 means the last class.  The ignored class gets 0: label smoothing would otherwise
    spread weight onto it.  All counts zero -> all weights zero."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(c)) or np.any(c < 0):
        raise ValueError(f"balanced_class_weights: counts must be finite and >= 0, got {c.tolist()}")
    k = c.shape[0]
    ii = None if ignore_index is None else (k - 1 if int(ignore_index) == -1 else int(ignore_index))
    S = [i for i in range(k) if i != ii and c[i] > 0]
    w = np.zeros(k, dtype=np.float64)
    if S:
        N = c[S].sum()
        for i in S:
            w[i] = N / (len(S) * c[i])
    return w.astype(np.float32)
