"""GPU overlap-average stitching of tile predictions -- the canvas arithmetic of the reference's ImageStitcher_v2
(st_water_seg/utils/utils_image.py:364-494) as predict.py:329-347 uses it: every crop's softmax is added into an
[H, W, n_classes] canvas at [h0:hE, w0:wE], a weight canvas counts the contributions, the result is
canvas / (weight + 1e-5).  Here the softmax + accumulate runs on the logits that are still resident in the HIP
context after an eval forward, so predictions never leave HBM until the final map is read.

Extension (blend != "uniform"): every crop counts with a separable window that falls off towards the tile's border --
canvas += w * p, weight += w with w = win[ly] * win[lx] (fu_stitch_add_batch_windowed) -- so a pixel is decided by the
crops that see it with their interior, and the seam at the end of an overlap goes.  The windows are strictly positive,
so such a canvas is finalised with eps = 0."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .infer_options import BLEND_KINDS


def blend_window(kind: str, n: int) -> np.ndarray:
    """The 1-D blending window of an n-pixel tile axis, float32 (formed in float64, rounded once); the 2-D window of a
    tile is the outer product of its two axes'.  "uniform": ones.  "linear": min(i + 1, n - i) / ((n + 1) // 2), a
    triangle that peaks at exactly 1.  "hann": sin^2(pi (i + 0.5) / n), the raised cosine sampled at pixel centres.
    All are symmetric and strictly positive (hann's minimum at n = 512 is 9.4e-6), so a covered pixel always has a
    positive weight."""
    if kind not in BLEND_KINDS:
        raise ValueError(f"blend must be one of {list(BLEND_KINDS)}, got {kind!r}")
    n = int(n)
    if n < 1:
        raise ValueError(f"blend_window: n must be >= 1, got {n}")
    i = np.arange(n, dtype=np.float64)
    if kind == "uniform":
        w = np.ones(n, dtype=np.float64)
    elif kind == "linear":
        w = np.minimum(i + 1, n - i) / ((n + 1) // 2)
    else:
        w = np.sin(np.pi * (i + 0.5) / n) ** 2
    return w.astype(np.float32)


class GpuImageStitcher:
    def __init__(self, net, device, blend: str = "uniform"):
        if blend not in BLEND_KINDS:
            raise ValueError(f"blend must be one of {list(BLEND_KINDS)}, got {blend!r}")
        self.net = net                      # HipUNet whose last eval forward produced the crops
        self.device = torch.device(device)
        self.blend = blend
        self.image_canvas: Dict[str, torch.Tensor] = {}
        self.weight_canvas: Dict[str, torch.Tensor] = {}
        self._windows: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}   # tile (H, W) -> (win_y, win_x)

    def _tile_windows(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """The blend's windows for the context's tile size, uploaded once per size."""
        if self.net._ctx is None:
            raise RuntimeError("GpuImageStitcher: the net has no context yet (run a forward first)")
        hw = (int(self.net._ctx_key[1]), int(self.net._ctx_key[2]))
        if hw not in self._windows:
            self._windows[hw] = tuple(torch.from_numpy(blend_window(self.blend, n)).to(self.device) for n in hw)
        return self._windows[hw]

    def add_image(self, sample: int, image_name: str, crop_info, og_height: int, og_width: int) -> None:
        """crop_info: object or tuple with h0, w0, hE, wE (datasets/utils.py CropParams)."""
        h0, w0, hE, wE = (crop_info if isinstance(crop_info, (tuple, list))
                          else (crop_info.h0, crop_info.w0, crop_info.hE, crop_info.wE))
        k = self.net.n_classes
        if image_name not in self.image_canvas:
            self.image_canvas[image_name] = torch.zeros(og_height, og_width, k, device=self.device)
            self.weight_canvas[image_name] = torch.zeros(og_height, og_width, device=self.device)
        if self.blend != "uniform":
            return self.add_images([sample], [image_name], [(h0, w0, hE, wE)], [og_height], [og_width])
        cv, wt = self.image_canvas[image_name], self.weight_canvas[image_name]
        check(_lib.load().fu_stitch_add(self.net._ctx, int(sample), ptr(cv), ptr(wt), og_height, og_width, int(h0),
                                        int(w0), int(hE), int(wE), torch.cuda.current_stream(self.device).cuda_stream))

    def add_images(self, samples, image_names, crop_info, og_heights, og_widths, probs=None) -> None:
        """ImageStitcher_v2.add_images (utils_image.py:386-406) without the image arrays -- crop i is sample samples[i] of
        the net's last eval forward, still resident on the device.  The whole list goes through ONE fu_stitch_add_batch
        launch, bit-identical to add_image for each crop in list order (also where crops of the list overlap).
        With probs (fp32 [N, H, W, k] on the device, e.g. HipUNet.merge_views' test-time-augmented probabilities),
        crop i adds probs[samples[i]] as it is instead of a softmax of the logits (fu_stitch_add_batch_probs): the same
        as canvas[box] += probs[s, :dh, :dw]; weight[box] += 1 in list order, bit for bit.
        With a blend other than "uniform" both forms go through fu_stitch_add_batch_windowed instead: crop pixel
        (ly, lx) adds w * p to the canvas and w to the weight, w = win_y[ly] * win_x[lx]."""
        samples, image_names, crop_info = list(samples), list(image_names), list(crop_info)
        og_heights, og_widths = list(og_heights), list(og_widths)
        n = len(samples)
        if not (len(image_names) == len(crop_info) == len(og_heights) == len(og_widths) == n):
            raise ValueError("add_images: samples, image_names, crop_info, og_heights and og_widths differ in length")
        if n == 0:
            return
        k = self.net.n_classes
        if probs is not None:
            if probs.dim() != 4 or probs.shape[3] != k or probs.dtype != torch.float32 or not probs.is_contiguous() \
                    or not probs.is_cuda:
                raise ValueError(f"add_images: probs must be contiguous fp32 [N, H, W, {k}] on the GPU, got "
                                 f"{tuple(probs.shape)} {probs.dtype} on {probs.device}")
            if self.net._ctx is None or tuple(probs.shape[1:3]) != tuple(self.net._ctx_key[1:3]):
                raise ValueError(f"add_images: probs tiles {tuple(probs.shape[1:3])} differ from the net's tile")
        table = (_lib.FuStitchEntry * n)()
        for i, (smp, name, ci, oh, ow) in enumerate(zip(samples, image_names, crop_info, og_heights, og_widths)):
            h0, w0, hE, wE = ci if isinstance(ci, (tuple, list)) else (ci.h0, ci.w0, ci.hE, ci.wE)
            if name not in self.image_canvas:
                self.image_canvas[name] = torch.zeros(oh, ow, k, device=self.device)
                self.weight_canvas[name] = torch.zeros(oh, ow, device=self.device)
            cv, wt = self.image_canvas[name], self.weight_canvas[name]
            table[i] = _lib.FuStitchEntry(ptr(cv), ptr(wt), int(smp), cv.shape[0], cv.shape[1], int(h0), int(w0),
                                          int(hE), int(wE), 0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.blend != "uniform":
            win_y, win_x = self._tile_windows()
            check(_lib.load().fu_stitch_add_batch_windowed(self.net._ctx, n, table, ptr(probs),
                                                           0 if probs is None else probs.shape[0], ptr(win_y), ptr(win_x),
                                                           stream))
        elif probs is None:
            check(_lib.load().fu_stitch_add_batch(self.net._ctx, n, table, stream))
        else:
            check(_lib.load().fu_stitch_add_batch_probs(self.net._ctx, n, table, ptr(probs), probs.shape[0], stream))

    def combine(self, image_name: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (probabilities [H, W, n_classes], argmax [H, W]); like _combine_images + the argmax of predict.py."""
        if self.blend != "uniform":         # eps = 0 (see combine_maps); the class map widened to combine's int64
            maps = self.combine_maps(image_name)
            return maps["canvas"], maps["class"].to(torch.int64)
        cv, wt = self.image_canvas[image_name], self.weight_canvas[image_name]
        am = torch.empty(cv.shape[:2], dtype=torch.int64, device=self.device)
        check(_lib.load().fu_stitch_finalize(ptr(cv), ptr(wt), cv.shape[2], cv.shape[0], cv.shape[1], ptr(am),
                                             torch.cuda.current_stream(self.device).cuda_stream))
        return cv, am

    def combine_maps(self, image_name: str, class_values: Optional[Sequence[int]] = None, probs: bool = False,
                     margin: bool = False, counts: bool = False,
                     threshold: Optional[Tuple[int, float]] = None, valid: Optional[torch.Tensor] = None,
                     nodata_value: Optional[int] = None) -> dict:
        """The fused finalisation (fu_stitch_finalize_maps), one launch: the canvas is normalised in place -- by
        (weight + 1e-5) under "uniform" as combine() does, by the weight alone otherwise (the windows are strictly
        positive; 1e-5 would bias a corner pixel whose only weight is of that order) -- and the uint8 rasters come out
        of the same pass.  -> {"canvas": fp32 [H, W, k], "class": uint8 [H, W] = class_values[argmax] (None: the argmax
        itself), and when asked for "probs": uint8 [k, H, W] = rint(clip(p, 0, 1) * 255), "margin": uint8 [H, W] = the same
        of top-1 minus top-2, "counts": int64 [k] pixels per argmax class}, all on the device.  Call it once per image,
        instead of combine().  threshold=(cls, T): the class map and the counts follow the one-versus-rest rule of
        fu_stitch_finalize_maps_ex instead of the argmax -- cls where its normalised probability is >= T, else the
        first maximum over the other classes; the other outputs do not change.  valid (uint8 [H, W] on the device, with
        nodata_value in 0..255 that is none of the class map's values): fu_stitch_finalize_maps_masked -- a pixel whose
        byte is 0 comes out as an uncovered one (canvas, "probs", "margin" 0, not counted), with "class" =
        nodata_value; without it the call and its results are what they were."""
        cv, wt = self.image_canvas[image_name], self.weight_canvas[image_name]
        H, W, k = cv.shape
        if class_values is not None:
            if len(class_values) != k or any(not 0 <= int(v) <= 255 for v in class_values):
                raise ValueError(f"combine_maps: class_values must be {k} values in 0..255, got {list(class_values)}")
            class_values = (ctypes.c_uint8 * k)(*[int(v) for v in class_values])      # a host array, passed by value
        out = {"canvas": cv, "class": torch.empty(H, W, dtype=torch.uint8, device=self.device)}
        if probs:
            out["probs"] = torch.empty(k, H, W, dtype=torch.uint8, device=self.device)
        if margin:
            out["margin"] = torch.empty(H, W, dtype=torch.uint8, device=self.device)
        if counts:
            out["counts"] = torch.zeros(k, dtype=torch.int64, device=self.device)
        eps = 1e-5 if self.blend == "uniform" else 0.0
        thr = None
        if threshold is not None:
            from .calibration import check_threshold
            thr = _lib.FuClassThreshold(*check_threshold(threshold[1], threshold[0], k))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if valid is None:
            if nodata_value is not None:
                raise ValueError("combine_maps: nodata_value comes with valid")
            check(_lib.load().fu_stitch_finalize_maps_ex(ptr(cv), ptr(wt), k, H, W, eps, 1, class_values, ptr(out["class"]),
                                                         ptr(out.get("probs")), ptr(out.get("margin")),
                                                         ptr(out.get("counts")), thr, stream))
            return out
        if tuple(valid.shape) != (H, W) or valid.dtype != torch.uint8 or not valid.is_contiguous() \
                or valid.device != cv.device:
            raise ValueError(f"combine_maps: valid must be contiguous uint8 [{H}, {W}] on {cv.device}, got "
                             f"{tuple(valid.shape)} {valid.dtype} on {valid.device}")
        if nodata_value is None:
            raise ValueError("combine_maps: valid needs nodata_value, the class map's byte of a pixel without data")
        check(_lib.load().fu_stitch_finalize_maps_masked(ptr(cv), ptr(wt), k, H, W, eps, 1, class_values, ptr(out["class"]),
                                                         ptr(out.get("probs")), ptr(out.get("margin")),
                                                         ptr(out.get("counts")), thr, ptr(valid), int(nodata_value), stream))
        return out

    def drop(self, image_name: str) -> None:
        """Forget a finished image's canvases (after combine): their memory returns to the allocator, ordered on the
        current stream, so a run's footprint is bounded by the images in flight rather than by the run."""
        del self.image_canvas[image_name]
        del self.weight_canvas[image_name]


class PackedRead:
    """Several device tensors read by ONE device-to-host copy.  add(name, tensor) registers a contiguous tensor under a
    name; read() concatenates their bytes in the order they were added (torch.cat of uint8 views: one launch), copies
    that to the host once and returns {name: numpy array} with each tensor's dtype and shape.  The arrays are views of
    the one host buffer; one that starts at a byte offset its dtype does not divide is unaligned, which numpy handles."""

    def __init__(self):
        self._parts = []                    # (name, the tensor's bytes uint8 [nbytes], numpy dtype, shape)

    def add(self, name: str, tensor: torch.Tensor) -> None:
        if any(name == n for n, *_ in self._parts):
            raise ValueError(f"PackedRead: {name!r} is registered twice")
        dtype = torch.empty(0, dtype=tensor.dtype).numpy().dtype
        self._parts.append((name, tensor.view(-1).view(torch.uint8), dtype, tuple(tensor.shape)))

    def read(self) -> Dict[str, np.ndarray]:
        packed = torch.cat([b for _, b, _, _ in self._parts]).cpu().numpy()
        out, at = {}, 0
        for name, b, dtype, shape in self._parts:
            out[name] = packed[at:at + b.numel()].view(dtype).reshape(shape)
            at += b.numel()
        return out
