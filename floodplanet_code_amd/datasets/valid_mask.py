"""Which pixels of a scene hold data: the valid-pixel rule of label-free scene inference (infer --nodata), its per-crop census,
and their device twins.

Real S1 / S2 / L8 / PS scenes come with swath edges, collars and fill.  Inference has no labels to tell it so; the mask has
to come from the image.  The numpy functions are the specification, the device functions are compared against them with
equality (the rule is integer-exact), and none of the host functions is a fallback for a device call:

  * `source_valid_host(raster, nodata)`: fp32 [C, h, w] after band selection, before sensor scaling -> uint8 [h, w].  A
    source pixel is valid (1) when every band is finite and not every band equals nodata (fp32 == against
    np.float32(nodata)); nodata None applies the finiteness test only.  A pixel where only some bands equal nodata is valid.
  * `grid_valid_host(src_valid, iy, wy, ix, wx)`: -> uint8 [H, W] on the resident grid, with the tables resident_grid builds
    (lanczos4_axis_window(n_src, n_dst, 0, n_dst, n_dst)).  Grid pixel (Y, X) is valid when src_valid[iy[Y, a], ix[X, b]]
    == 1 for every tap pair (a, b) with wy[Y, a] != 0 and wx[X, b] != 0: nothing it was resampled from was fill.  With
    identity tables this is the source mask itself.
  * `box_valid_counts_host(mask, boxes)`: int64 [n], the valid (non-zero) pixels of each box (h0, w0, hE, wE).
  * `scene_valid_mask(raster_dev, nodata, tables)` (C ABI fu_scene_valid_mask, two launches) and
    `box_valid_counts(ctx, mask, boxes)` (fu_mask_box_counts, one launch): the same on the device; results stay there.

Out of scope: the resampling itself is not mask-aware (a valid grid pixel never saw fill, so it needs none; an invalid one
is not read), norm_mode 'local' still takes a crop's statistics over all its pixels, fill included, and neither predict
(labelled evaluation, whose labels carry the nodata) nor training is touched.  Host-only at import."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

__all__ = ["source_valid_host", "grid_valid_host", "box_valid_counts_host", "scene_valid_mask", "box_valid_counts",
           "axis_tables"]

Box = Tuple[int, int, int, int]


def _check_nodata(fn: str, nodata) -> Optional[np.float32]:
    if nodata is None:
        return None
    value = np.float32(nodata)
    if not np.isfinite(value):
        raise ValueError(f"{fn}: nodata must be finite (or None), got {nodata!r}")
    return value


def source_valid_host(raster: np.ndarray, nodata=None) -> np.ndarray:
    a = np.asarray(raster, dtype=np.float32)
    if a.ndim != 3 or a.shape[0] < 1:
        raise ValueError(f"source_valid: raster must be [C, h, w], got {a.shape}")
    value = _check_nodata("source_valid", nodata)
    valid = np.isfinite(a).all(axis=0)
    if value is not None:
        valid &= ~(a == value).all(axis=0)
    return valid.astype(np.uint8)


def grid_valid_host(src_valid: np.ndarray, iy: np.ndarray, wy: np.ndarray, ix: np.ndarray, wx: np.ndarray) -> np.ndarray:
    m = np.asarray(src_valid) == 1
    iy, wy, ix, wx = (np.asarray(t) for t in (iy, wy, ix, wx))
    if m.ndim != 2 or iy.shape != wy.shape or ix.shape != wx.shape or iy.ndim != 2 or ix.ndim != 2 \
            or iy.shape[1] != 8 or ix.shape[1] != 8:
        raise ValueError("grid_valid: src_valid must be [h, w] and the tables [H, 8] / [W, 8]")
    out = np.ones((iy.shape[0], ix.shape[0]), dtype=bool)
    for a in range(8):
        rows = m[iy[:, a]]                                   # [H, w]
        use_y = (wy[:, a] != 0)[:, None]
        for b in range(8):
            tap = rows[:, ix[:, b]]                          # [H, W]
            use = use_y & (wx[:, b] != 0)[None, :]
            out &= tap | ~use
    return out.astype(np.uint8)


def _check_boxes(fn: str, mask_hw: Tuple[int, int], boxes: Sequence[Box]):
    if len(boxes) < 1:
        raise ValueError(f"{fn}: no boxes")
    H, W = mask_hw
    out = []
    for i, box in enumerate(boxes):
        h0, w0, hE, wE = (int(v) for v in box)
        if not (0 <= h0 < hE <= H and 0 <= w0 < wE <= W):
            raise ValueError(f"{fn}: box {i} [{h0}:{hE}, {w0}:{wE}] is empty or lies outside its mask {H}x{W}")
        out.append((h0, w0, hE, wE))
    return out


def box_valid_counts_host(mask: np.ndarray, boxes: Sequence[Box]) -> np.ndarray:
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f"box_valid_counts: mask must be [H, W], got {m.shape}")
    checked = _check_boxes("box_valid_counts", m.shape, boxes)
    return np.array([int(np.count_nonzero(m[h0:hE, w0:wE])) for h0, w0, hE, wE in checked], dtype=np.int64)


def axis_tables(src_hw: Tuple[int, int], grid_hw: Tuple[int, int], device=None):
    """The four tap tables of a whole scene, (iy, wy, ix, wx) as lanczos4_axis_window makes them for the whole grid; on
    `device` as torch tensors ([H, 8] / [W, 8], int32 / fp32) when one is given, else numpy."""
    from .resize import lanczos4_axis_window
    iy, wy, _ = lanczos4_axis_window(int(src_hw[0]), int(grid_hw[0]), 0, int(grid_hw[0]), int(grid_hw[0]))
    ix, wx, _ = lanczos4_axis_window(int(src_hw[1]), int(grid_hw[1]), 0, int(grid_hw[1]), int(grid_hw[1]))
    if device is None:
        return iy, wy, ix, wx
    return tuple(torch.from_numpy(t).to(device, non_blocking=True) for t in (iy, wy, ix, wx))


def scene_valid_mask(raster_dev: torch.Tensor, nodata, tables) -> Tuple[torch.Tensor, torch.Tensor]:
    """C ABI fu_scene_valid_mask: raster_dev contiguous fp32 [C, h, w] on the ROCm device (as uploaded, before sensor
    scaling), nodata None or a finite number, tables = (iy, wy, ix, wx) on that device ([H, 8] / [W, 8], or with the leading
    1 resize_lanczos4_tiles takes) -> (mask uint8 [H, W], n_valid int64 [1]), both on the device: grid_valid_host of
    source_valid_host, and its sum.  Two launches, no host read."""
    from .. import _lib
    fn = "scene_valid_mask"
    if raster_dev.device.type != "cuda":
        raise RuntimeError(f"{fn} runs only on a ROCm GPU; the host statement is grid_valid_host(source_valid_host(...))")
    if raster_dev.dim() != 3 or raster_dev.dtype != torch.float32 or not raster_dev.is_contiguous():
        raise ValueError(f"{fn}: raster must be contiguous fp32 [C, h, w], got {tuple(raster_dev.shape)} {raster_dev.dtype}")
    value = _check_nodata(fn, nodata)
    dev = raster_dev.device
    Cc, h, w = raster_dev.shape
    iy, wy, ix, wx = (t.reshape(-1, 8) for t in tables)
    iy, ix = (t.to(dev).to(torch.int32).contiguous() for t in (iy, ix))
    wy, wx = (t.to(dev).float().contiguous() for t in (wy, wx))
    if wy.shape != iy.shape or wx.shape != ix.shape:
        raise ValueError(f"{fn}: index and weight tables differ in shape")
    H, W = iy.shape[0], ix.shape[0]
    scratch = torch.empty(h, w, dtype=torch.uint8, device=dev)
    mask = torch.empty(H, W, dtype=torch.uint8, device=dev)
    n_valid = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().fu_scene_valid_mask(
        _lib.ptr(raster_dev), Cc, h, w, 0 if value is None else 1, 0.0 if value is None else float(value), _lib.ptr(iy),
        _lib.ptr(wy), _lib.ptr(ix), _lib.ptr(wx), H, W, _lib.ptr(scratch), _lib.ptr(mask), _lib.ptr(n_valid),
        torch.cuda.current_stream(dev).cuda_stream))
    return mask, n_valid


def box_valid_counts(ctx, mask: torch.Tensor, boxes: Sequence[Box], counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C ABI fu_mask_box_counts: mask uint8 [H, W] on the ROCm device (any row-contiguous view: its row stride is its
    width), boxes = [(h0, w0, hE, wE), ...] -> int64 [n] on that device, WRITTEN (cells of `counts` beyond n are left alone
    when it is given).  One launch for the whole table.  ctx: the fu_ctx whose table buffer the call borrows
    (HipUNet._get_ctx)."""
    from .. import _lib
    fn = "box_valid_counts"
    if ctx is None:
        raise ValueError(f"{fn}: no fu_ctx (run or prepare a forward first)")
    if mask.device.type != "cuda":
        raise RuntimeError(f"{fn} runs only on a ROCm GPU; the host statement is box_valid_counts_host")
    if mask.dim() != 2 or mask.dtype != torch.uint8 or not mask.is_contiguous():
        raise ValueError(f"{fn}: mask must be contiguous uint8 [H, W], got {tuple(mask.shape)} {mask.dtype}")
    checked = _check_boxes(fn, tuple(mask.shape), boxes)
    n = len(checked)
    dev = mask.device
    if counts is None:
        counts = torch.empty(n, dtype=torch.int64, device=dev)
    elif counts.dim() != 1 or counts.shape[0] < n or counts.dtype != torch.int64 or not counts.is_contiguous() \
            or counts.device != dev:
        raise ValueError(f"{fn}: counts must be contiguous int64 [>= {n}] on {dev}")
    table = (_lib.FuMaskBox * n)()
    for i, (h0, w0, hE, wE) in enumerate(checked):
        table[i] = _lib.FuMaskBox(mask.data_ptr(), mask.shape[0], mask.shape[1], h0, w0, hE, wE)
    _lib.check(_lib.load().fu_mask_box_counts(ctx, n, table, _lib.ptr(counts), torch.cuda.current_stream(dev).cuda_stream))
    return counts[:n]
