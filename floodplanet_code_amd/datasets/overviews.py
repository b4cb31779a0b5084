"""Overview pyramids of the rasters scene inference writes: the reduced-resolution images a GIS or a tile server draws a
large flood map from.  overviews_host is the numpy statement and the specification; overviews_on_device is the same thing on
a strided device tensor (C ABI fu_map_overviews, csrc/fu_overview.hip), six levels per launch from one read of the base, so
infer cuts the levels in HBM between the sieve and the scene's one device-to-host read.

Level sizes.  Level l >= 1 of an h x w raster is ceil(h / 2^l) x ceil(w / 2^l).  Pixel (y, x) of level l is reduced from
the pixels (2y..2y+1, 2x..2x+1) of level l - 1 that exist: one, two or four.  The levels are a cascade: level l is made from
level l - 1, never from the base.

Kinds.  Every one is integer-exact or has a fixed operation order, so host and device compare with == (fp32: bit patterns).
  mode_u8   (class map) the most frequent value among the block's pixels that differ from nodata_value (None: none is
            excluded); ties go to the smaller value, the sieve's own rule; nodata_value where every pixel is nodata.
  mean_u8   (probability bands, margin) over the block's valid pixels (2 * sum + n) // (2 * n): integers, rounding half up;
            0 where no pixel is valid.
  mean_f32  (fp32 canvas) the valid pixels summed in row-major order in fp32 starting from +0, one rounding per add, then
            one correctly rounded division by float32(n); 0 where no pixel is valid.  (Bit equality holds for finite
            samples and infinities; which payload a NaN carries through an add is the machine's.)
  any_u8    (the valid raster) 1 where a pixel of the block is non-zero, else 0.
The mean kinds take `valid`, a uint8 [h, w] mask at the resolution of the raster (None: every pixel is valid); the mask of
level l is `any` of the mask of level l - 1, and with a mask they return the mask levels as well.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

__all__ = ["KINDS", "overview_sizes", "max_levels", "auto_levels", "check_levels", "overviews_host", "overviews_on_device",
           "STRIP_SIDE"]

KINDS = {"mode_u8": 0, "mean_u8": 1, "mean_f32": 2, "any_u8": 3}     # enum fu_overview_kind
MAX_BANDS = 16              # FU_TIFF_MAX_BANDS
STRIP_SIDE = 256            # the `side` of auto_levels for a raster written in strips


def max_levels(h: int, w: int) -> int:
    """The number of levels down to 1 x 1: ceil(log2(max(h, w)))."""
    n, m = 0, max(int(h), int(w))
    while m > 1:
        m, n = -(-m // 2), n + 1
    return n


def check_levels(n_levels) -> int:
    if isinstance(n_levels, bool) or not isinstance(n_levels, (int, np.integer)) or int(n_levels) < 0:
        raise ValueError(f"n_levels must be an integer >= 0, got {n_levels!r}")
    return int(n_levels)


def overview_sizes(h: int, w: int, n_levels: int) -> List[Tuple[int, int]]:
    """(h_l, w_l) of levels 1..n_levels; a count above the number of levels down to 1 x 1 is clamped to that number."""
    if int(h) < 1 or int(w) < 1:
        raise ValueError(f"empty raster {h}x{w}")
    n = min(check_levels(n_levels), max_levels(h, w))
    return [(-(-int(h) // (1 << l)), -(-int(w) // (1 << l))) for l in range(1, n + 1)]


def auto_levels(h: int, w: int, side: int) -> int:
    """The smallest n with ceil(max(h, w) / 2^n) <= side; side: the tile side, or STRIP_SIDE for strips."""
    if int(side) < 1:
        raise ValueError(f"side must be >= 1, got {side!r}")
    n, m = 0, max(int(h), int(w))
    while -(-m // (1 << n)) > int(side):
        n += 1
    return n


def _check(kind: str, dtype, ndim: int, bands: int, valid, nodata_value) -> None:
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {list(KINDS)}, got {kind!r}")
    want = "float32" if kind == "mean_f32" else "uint8"
    if str(dtype).replace("torch.", "") != want:
        raise ValueError(f"{kind} takes {want} samples, got {dtype}")
    if ndim not in (2, 3) or not 1 <= bands <= MAX_BANDS:
        raise ValueError(f"the raster must be [H, W] or [bands, H, W] with 1..{MAX_BANDS} bands")
    if valid is not None and kind not in ("mean_u8", "mean_f32"):
        raise ValueError(f"{kind} takes no valid mask")
    if nodata_value is not None:
        if kind != "mode_u8":
            raise ValueError(f"{kind} takes no nodata_value")
        if isinstance(nodata_value, bool) or int(nodata_value) != nodata_value or not 0 <= int(nodata_value) <= 255:
            raise ValueError(f"nodata_value must be an integer in 0..255, got {nodata_value!r}")


def _quads(a: np.ndarray):
    """a [..., h, w] -> the four [..., ceil(h / 2), ceil(w / 2)] arrays of the block positions in row-major order, (0, 0),
    (0, 1), (1, 0), (1, 1) (zeros where the position lies outside a), and the four [h2, w2] bool arrays of which exist."""
    h, w = a.shape[-2:]
    h2, w2 = -(-h // 2), -(-w // 2)
    pad = np.zeros(a.shape[:-2] + (2 * h2, 2 * w2), dtype=a.dtype)
    pad[..., :h, :w] = a
    there = np.zeros((2 * h2, 2 * w2), dtype=bool)
    there[:h, :w] = True
    return [pad[..., dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)], [there[dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]


def _reduce(a: np.ndarray, kind: str, mask: Optional[np.ndarray], nodata_value: Optional[int]):
    """One level: a [bands, h, w], mask [h, w] bool or None -> (the level [bands, h2, w2], its mask or None)."""
    v, there = _quads(a)
    ok = [t[None] for t in there]                                     # [1, h2, w2], broadcast over the bands
    if mask is not None:
        ok = [o & m[None] for o, m in zip(ok, _quads(mask)[0])]
    if kind == "mode_u8":
        if nodata_value is not None:
            ok = [o & (x != nodata_value) for o, x in zip(ok, v)]
        best = np.full(v[0].shape, -1, dtype=np.int32)                # count << 8 | 255 - value; -1: every pixel is nodata
        for j in range(4):
            n = sum((ok[m] & (v[m] == v[j])).astype(np.int32) for m in range(4))
            best = np.maximum(best, np.where(ok[j], (n << 8) | (255 - v[j].astype(np.int32)), -1))
        fill = 0 if nodata_value is None else int(nodata_value)
        out = np.where(best < 0, fill, 255 - (best & 255)).astype(np.uint8)
    elif kind == "mean_u8":
        s = sum(np.where(o, x, 0).astype(np.int32) for o, x in zip(ok, v))
        n = sum(np.broadcast_to(o, x.shape).astype(np.int32) for o, x in zip(ok, v))
        out = np.where(n > 0, (2 * s + n) // np.maximum(2 * n, 1), 0).astype(np.uint8)
    elif kind == "mean_f32":
        acc = np.zeros(v[0].shape, dtype=np.float32)
        n = np.zeros(v[0].shape, dtype=np.int32)
        with np.errstate(all="ignore"):
            for o, x in zip(ok, v):                                   # row-major, one fp32 rounding per add
                acc = np.where(o, acc + x.astype(np.float32), acc).astype(np.float32)
                n = n + o
            out = np.where(n > 0, acc / np.maximum(n, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    else:
        out = np.zeros(v[0].shape, dtype=bool)
        for o, x in zip(ok, v):
            out |= o & (x != 0)
        out = out.astype(np.uint8)
    if mask is None:
        return out, None
    return out, np.logical_or.reduce([o[0] for o in ok])


def overviews_host(array, kind: str, n_levels: int, valid=None, nodata_value=None):
    """The numpy statement (see the module docstring).  array: [H, W] or [bands, H, W], uint8 (float32 for mean_f32), any
    strides.  -> the list of the levels 1..n_levels (clamped as overview_sizes does), each of the array's rank; for the mean
    kinds (levels, mask levels), the mask levels uint8 [h_l, w_l] 0 / 1, or None without a mask."""
    a = np.asarray(array)
    _check(kind, a.dtype, a.ndim, 1 if a.ndim < 3 else a.shape[0], valid, nodata_value)
    cur = a if a.ndim == 3 else a[None]
    sizes = overview_sizes(cur.shape[1], cur.shape[2], n_levels)
    mask = None
    if valid is not None:
        mask = np.asarray(valid) != 0
        if mask.shape != cur.shape[1:]:
            raise ValueError(f"valid of shape {mask.shape}, the raster is {cur.shape[1:]}")
    levels, masks = [], []
    for size in sizes:
        cur, mask = _reduce(cur, kind, mask, nodata_value)
        assert cur.shape[1:] == size
        levels.append(np.ascontiguousarray(cur if a.ndim == 3 else cur[0]))
        if mask is not None:
            masks.append(mask.astype(np.uint8))
    if kind in ("mean_u8", "mean_f32"):
        return levels, (masks if valid is not None else None)
    return levels


def overviews_on_device(tensor, kind: str, n_levels: int, valid=None, nodata_value=None):
    """C ABI fu_map_overviews: a tensor on the ROCm device, [H, W] or [bands, H, W] with any non-negative strides (canvas
    .permute(2, 0, 1) is a source without a copy), and for the mean kinds an optional uint8 [H, W] mask -> what
    overviews_host returns, as contiguous device tensors (views of one buffer), bit for bit.  One launch per six levels on
    the current stream; no host pass over the samples."""
    import torch

    from .. import _lib
    if not torch.is_tensor(tensor) or tensor.device.type != "cuda":
        raise RuntimeError("overviews_on_device runs only on a ROCm GPU tensor; the host statement is overviews_host")
    _check(kind, tensor.dtype, tensor.dim(), 1 if tensor.dim() < 3 else tensor.shape[0], valid, nodata_value)
    a = tensor if tensor.dim() == 3 else tensor[None]
    bands, H, W = (int(s) for s in a.shape)
    strides = [int(s) for s in a.stride()]
    if min(strides) < 0:
        raise ValueError("overviews_on_device: negative strides are not supported")
    sizes = overview_sizes(H, W, n_levels)
    if not sizes:                                                     # nothing to launch
        return ([], [] if valid is not None else None) if kind in ("mean_u8", "mean_f32") else []
    pixels = sum(h * w for h, w in sizes)
    dst = torch.empty(bands * pixels, dtype=a.dtype, device=a.device)
    mask = vdst = None
    if valid is not None:
        if not torch.is_tensor(valid) or valid.dtype != torch.uint8 or tuple(valid.shape) != (H, W) or \
                valid.device != a.device:
            raise ValueError(f"valid must be a uint8 [{H}, {W}] tensor on the raster's device")
        mask = valid.contiguous()
        vdst = torch.empty(pixels, dtype=torch.uint8, device=a.device)
    _lib.check(_lib.load().fu_map_overviews(a.data_ptr(), strides[0], strides[1], strides[2], bands, H, W, KINDS[kind],
                                            _lib.ptr(mask), -1 if nodata_value is None else int(nodata_value), len(sizes),
                                            _lib.ptr(dst), dst.numel(), _lib.ptr(vdst),
                                            torch.cuda.current_stream(a.device).cuda_stream))
    levels, masks, at, vat = [], [], 0, 0
    for h, w in sizes:
        level = dst[at:at + bands * h * w].view(bands, h, w)
        levels.append(level if tensor.dim() == 3 else level[0])
        at += bands * h * w
        if vdst is not None:
            masks.append(vdst[vat:vat + h * w].view(h, w))
            vat += h * w
    if kind in ("mean_u8", "mean_f32"):
        return levels, (masks if valid is not None else None)
    return levels
