"""GPU tile assembly: per-tile normalisation, edge-crop buffer and multi-sensor channel concatenation of a whole batch in HBM
(C ABI `fu_assemble_tiles`), replacing the per-item CPU work of the reference's `BaseDataset.normalize`
(st_water_seg/datasets/base_dataset.py:77-113), `_add_buffer_to_image` (:271-325) and the channel concatenation of the
fused inputs (ef_model.py:28-44; Planet + Sentinel-1 stacks of BASELINE configs[4]).  The output feeds `fu_augment` /
`fu_forward` directly."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from .. import _lib
from .._lib import check, ptr

NORM_MODES = {None: 0, "local": 1, "global": 2}


def _norm_mode(norm_mode) -> int:
    if norm_mode not in NORM_MODES:
        raise NotImplementedError(f'Normalization mode "{norm_mode}" not implemented.')      # base_dataset.py:106-108
    return NORM_MODES[norm_mode]


def _global_norm(mode: int, global_params, dev, mean: torch.Tensor, std: torch.Tensor):
    """-> the per-channel (mean, std) on dev that the C ABI takes in mode 2 ('global'), else (None, None); in mode 2 the
    returned mean / std rows are pre-filled with them (the kernels write those only in mode 1)."""
    if mode != 2:
        return None, None
    if global_params is None:
        raise ValueError("norm_mode 'global' needs (mean, std) per channel")
    gm, gs = (t.to(dev).float().contiguous() for t in global_params)
    mean[:] = gm
    std[:] = gs
    return gm, gs


def _check_scene(where: str, scene: torch.Tensor, Cc: int, dev) -> None:
    if scene.dim() != 3 or scene.shape[0] != Cc or scene.dtype != torch.float32 or not scene.is_contiguous() \
            or scene.device != dev or dev.type != "cuda":
        raise ValueError(f"{where}: scenes must be contiguous fp32 [{Cc}, H, W] on one ROCm device, got "
                         f"{tuple(scene.shape)} {scene.dtype} on {scene.device}")


def assemble_tiles(sources: Sequence[torch.Tensor], norm_mode: Optional[str] = None,
                   valid_hw: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                   global_params: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, pad_value: float = 0.0):
    """sources: fp32 NCHW [B, C_k, H, W] tiles on a ROCm device (raw crops in the top-left corner of the nominal tile).
    -> (image [B, sum C, H, W], mean [B, sum C, 1, 1], std [B, sum C, 1, 1]) as the item dict of the reference carries them."""
    mode = _norm_mode(norm_mode)
    if not sources or sources[0].device.type != "cuda":
        raise RuntimeError("assemble_tiles runs only on a ROCm GPU; there is no CPU fallback")
    srcs = [s.contiguous().float() for s in sources]
    B, _, H, W = srcs[0].shape
    for s in srcs:
        if s.shape[0] != B or s.shape[2:] != (H, W):
            raise ValueError("all sources must share batch and tile size")
    dev = srcs[0].device
    ctot = sum(s.shape[1] for s in srcs)
    out = torch.empty(B, ctot, H, W, dtype=torch.float32, device=dev)
    mean = torch.zeros(B, ctot, dtype=torch.float32, device=dev)
    std = torch.ones(B, ctot, dtype=torch.float32, device=dev)
    gm, gs = _global_norm(mode, global_params, dev, mean, std)
    vh = vw = None
    if valid_hw is not None:
        vh, vw = (t.to(dev).to(torch.int32).contiguous() for t in valid_hw)
    arr = (C.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])
    chs = (C.c_int32 * len(srcs))(*[s.shape[1] for s in srcs])
    check(_lib.load().fu_assemble_tiles(arr, chs, len(srcs), B, H, W, ptr(vh), ptr(vw), mode, ptr(gm), ptr(gs),
                                        float(pad_value), ptr(out), ptr(mean) if mode == 1 else None,
                                        ptr(std) if mode == 1 else None, torch.cuda.current_stream(dev).cuda_stream))
    return out, mean.view(B, ctot, 1, 1), std.view(B, ctot, 1, 1)


def scene_crops(ctx, boxes, tile_hw: Tuple[int, int], norm_mode: Optional[str] = None,
                global_params: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, pad_value: float = 0.0, out=None):
    """C ABI fu_scene_crops: boxes = [(scene, (h0, w0, hE, wE)), ...], each scene a contiguous fp32 [C, H_s, W_s] on the
    ROCm device, each box inside its scene and at most tile_hw.  -> (image [n, C, th, tw], mean, std [n, C, 1, 1]): equal
    bit for bit to assemble_tiles of the boxes cut into the top-left corner of a zero batch with valid_hw = the box sizes.
    ctx: the fu_ctx handle that owns the device copy of the table (HipUNet._ctx).  out: optional fp32 [>= n, C, th, tw]
    buffer whose first n samples receive the crops."""
    mode = _norm_mode(norm_mode)
    n = len(boxes)
    if n == 0:
        raise ValueError("scene_crops: no boxes")
    if ctx is None:
        raise ValueError("scene_crops: no fu_ctx (run or prepare a forward first)")
    th, tw = int(tile_hw[0]), int(tile_hw[1])
    dev = boxes[0][0].device
    Cc = boxes[0][0].shape[0]
    table = (_lib.FuSceneCrop * n)()
    for i, (scene, (h0, w0, hE, wE)) in enumerate(boxes):
        _check_scene(f"scene_crops: box {i}", scene, Cc, dev)
        table[i] = _lib.FuSceneCrop(scene.data_ptr(), scene.shape[1], scene.shape[2], int(h0), int(w0), int(hE), int(wE))
    if out is None:
        out = torch.empty(n, Cc, th, tw, dtype=torch.float32, device=dev)
    elif tuple(out.shape[1:]) != (Cc, th, tw) or out.shape[0] < n or out.dtype != torch.float32 \
            or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"scene_crops: out must be contiguous fp32 [>= {n}, {Cc}, {th}, {tw}] on {dev}")
    mean = torch.zeros(n, Cc, dtype=torch.float32, device=dev)
    std = torch.ones(n, Cc, dtype=torch.float32, device=dev)
    gm, gs = _global_norm(mode, global_params, dev, mean, std)
    check(_lib.load().fu_scene_crops(ctx, n, table, Cc, th, tw, mode, ptr(gm), ptr(gs), float(pad_value), ptr(out),
                                     ptr(mean) if mode == 1 else None, ptr(std) if mode == 1 else None,
                                     torch.cuda.current_stream(dev).cuda_stream))
    return out[:n], mean.view(n, Cc, 1, 1), std.view(n, Cc, 1, 1)


def _scene_aug(n: int, Cc: int, photometric: Optional[dict], zoom):
    """-> (fu_scene_aug, the numpy arrays it points into) from scene_train_tiles' photometric / zoom arguments; shapes are
    checked here, values by the library."""
    import numpy as np
    aug, keep = _lib.FuSceneAug(), []

    def host(v, dtype, size, name):
        if v is None:
            return None
        a = np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=dtype)
        if a.size != size:
            raise ValueError(f"scene_train_tiles: {name} has {a.size} values, expected {size}")
        keep.append(a)
        return a.ctypes.data

    ph = dict(photometric or {})
    unknown = sorted(set(ph) - {"gain", "bias", "sigma", "noise_key", "noise_stream"})
    if unknown:
        raise ValueError(f"scene_train_tiles: unknown photometric keys {unknown}")
    aug.gain = host(ph.get("gain"), np.float32, n * Cc, "photometric gain")
    aug.bias = host(ph.get("bias"), np.float32, n * Cc, "photometric bias")
    aug.sigma = host(ph.get("sigma"), np.float32, n * Cc, "photometric sigma")
    aug.noise_stream = host(ph.get("noise_stream"), np.uint64, n, "photometric noise_stream")
    aug.noise_key = int(ph.get("noise_key") or 0) & (2 ** 64 - 1)
    if zoom is not None:
        out_h, out_w = zoom
        aug.out_h = host(out_h, np.int32, n, "zoom out_h")
        aug.out_w = host(out_w, np.int32, n, "zoom out_w")
    return aug, keep


def scene_train_tiles(ctx, entries, tile_hw: Tuple[int, int], norm_mode: Optional[str] = None,
                      global_params: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, pad_value: float = 0.0,
                      nodata_value: int = 0, target_fill: int = 0, out=None, photometric: Optional[dict] = None,
                      zoom=None):
    """C ABI fu_scene_train_tiles: entries = [(scene, label, (h0, w0, hE, wE), flags, angle_deg), ...] -- scene a contiguous
    fp32 [C, H_s, W_s] on the ROCm device, label the scene's raw uint8 [H_s, W_s] label raster there (None for every entry:
    no target), the box inside the scene and at most tile_hw, flags / angle as augment.sample_transforms draws them.
    -> (image [n, C, th, tw], target int64 [n, th, tw] or None, mean, std [n, C, 1, 1]): bit for bit scene_crops followed
    by augment.apply on the decoded label boxes, in one launch (two with 'local') and without the batch in between.
    global_params: fp32 tensors; pass them on the device to keep the call free of host-to-device copies.
    out: optional (image, target, mean, std) buffers of those shapes (mean / std [n, C]) to write into.

    photometric / zoom (both None: the call above, unchanged) go to fu_scene_train_tiles_ex.  photometric: a dict with any of
    gain, bias, sigma (float [n, C], None = that term is skipped) and, for sigma, noise_key (int) and noise_stream (uint64
    [n]); augment.photometric_host states what they do.  zoom: (out_h, out_w), int [n] each -- entry b's box, of any size
    inside its scene, is resampled onto the top-left out_h[b] x out_w[b] region of the tile (sampling.zoom_tile_host);
    under 'local' mean / std are then the source box's."""
    mode = _norm_mode(norm_mode)
    n = len(entries)
    if n == 0:
        raise ValueError("scene_train_tiles: no entries")
    if ctx is None:
        raise ValueError("scene_train_tiles: no fu_ctx (run or prepare a forward first)")
    th, tw = int(tile_hw[0]), int(tile_hw[1])
    dev = entries[0][0].device
    Cc = entries[0][0].shape[0]
    with_target = entries[0][1] is not None
    table = (_lib.FuSceneTrainEntry * n)()
    for i, (scene, label, (h0, w0, hE, wE), flags, angle) in enumerate(entries):
        _check_scene(f"scene_train_tiles: entry {i}", scene, Cc, dev)
        if (label is not None) != with_target:
            raise ValueError("scene_train_tiles: either every entry has a label raster or none has")
        if label is not None and (label.dtype != torch.uint8 or tuple(label.shape) != tuple(scene.shape[1:])
                                  or not label.is_contiguous() or label.device != dev):
            raise ValueError(f"scene_train_tiles: entry {i}: the label must be contiguous uint8 {tuple(scene.shape[1:])} on "
                             f"{dev}, got {tuple(label.shape)} {label.dtype} on {label.device}")
        table[i] = _lib.FuSceneTrainEntry(scene.data_ptr(), ptr(label), scene.shape[1], scene.shape[2], int(h0), int(w0),
                                          int(hE), int(wE), int(flags), float(angle))
    if out is not None:
        image, target, mean, std = out
    else:
        image = torch.empty(n, Cc, th, tw, dtype=torch.float32, device=dev)
        target = torch.empty(n, th, tw, dtype=torch.int64, device=dev) if with_target else None
        mean = torch.zeros(n, Cc, dtype=torch.float32, device=dev)
        std = torch.ones(n, Cc, dtype=torch.float32, device=dev)
    gm, gs = _global_norm(mode, global_params, dev, mean, std)
    args = (ctx, n, table, Cc, th, tw, mode, ptr(gm), ptr(gs), float(pad_value), int(nodata_value), int(target_fill),
            ptr(image), ptr(target) if with_target else None, ptr(mean) if mode == 1 else None,
            ptr(std) if mode == 1 else None)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if photometric is None and zoom is None:
        check(_lib.load().fu_scene_train_tiles(*args, stream))
    else:
        aug, keep = _scene_aug(n, Cc, photometric, zoom)       # keep: the host arrays the struct points into
        check(_lib.load().fu_scene_train_tiles_ex(*args, C.byref(aug), stream))
        del keep
    return image, (target if with_target else None), mean.view(n, Cc, 1, 1), std.view(n, Cc, 1, 1)


def resize_lanczos4_tiles(windows: torch.Tensor, iy: torch.Tensor, wy: torch.Tensor, ix: torch.Tensor, wx: torch.Tensor,
                          scale_mode: int = 0) -> torch.Tensor:
    """C ABI fu_resize_lanczos4_tiles: windows fp32 [B, C, wh, ww] + the tap tables of `resize.lanczos4_axis_window`
    ([B, TH, 8] / [B, TW, 8]) on a ROCm device -> the resampled (and sensor-scaled) tiles [B, C, TH, TW]."""
    if windows.device.type != "cuda":
        raise RuntimeError("resize_lanczos4_tiles runs only on a ROCm GPU; the host restatement is datasets.resize")
    dev = windows.device
    win = windows.contiguous().float()
    iy, ix = (t.to(dev).to(torch.int32).contiguous() for t in (iy, ix))
    wy, wx = (t.to(dev).float().contiguous() for t in (wy, wx))
    B, Cc, wh, ww = win.shape
    TH, TW = iy.shape[1], ix.shape[1]
    if iy.shape != (B, TH, 8) or wy.shape != (B, TH, 8) or ix.shape != (B, TW, 8) or wx.shape != (B, TW, 8):
        raise ValueError("tap tables must be [B, tile_h, 8] / [B, tile_w, 8]")
    out = torch.empty(B, Cc, TH, TW, dtype=torch.float32, device=dev)
    check(_lib.load().fu_resize_lanczos4_tiles(ptr(win), B, Cc, wh, ww, ptr(iy), ptr(wy), ptr(ix), ptr(wx), TH, TW,
                                               int(scale_mode), ptr(out), torch.cuda.current_stream(dev).cuda_stream))
    return out
