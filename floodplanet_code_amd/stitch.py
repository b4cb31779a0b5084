"""GPU overlap-average stitching of tile predictions -- the canvas arithmetic of the reference's ImageStitcher_v2
(st_water_seg/utils/utils_image.py:364-494) as predict.py:329-347 uses it: every crop's softmax is added into an
[H, W, n_classes] canvas at [h0:hE, w0:wE], a weight canvas counts the contributions, the result is
canvas / (weight + 1e-5).  Here the softmax + accumulate runs on the logits that are still resident in the HIP
context after an eval forward, so predictions never leave HBM until the final map is read."""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from . import _lib
from ._lib import check, ptr


class GpuImageStitcher:
    def __init__(self, net, device):
        self.net = net                      # HipUNet whose last eval forward produced the crops
        self.device = torch.device(device)
        self.image_canvas: Dict[str, torch.Tensor] = {}
        self.weight_canvas: Dict[str, torch.Tensor] = {}

    def add_image(self, sample: int, image_name: str, crop_info, og_height: int, og_width: int) -> None:
        """crop_info: object or tuple with h0, w0, hE, wE (datasets/utils.py CropParams)."""
        h0, w0, hE, wE = (crop_info if isinstance(crop_info, (tuple, list))
                          else (crop_info.h0, crop_info.w0, crop_info.hE, crop_info.wE))
        k = self.net.n_classes
        if image_name not in self.image_canvas:
            self.image_canvas[image_name] = torch.zeros(og_height, og_width, k, device=self.device)
            self.weight_canvas[image_name] = torch.zeros(og_height, og_width, device=self.device)
        cv, wt = self.image_canvas[image_name], self.weight_canvas[image_name]
        check(_lib.load().fu_stitch_add(self.net._ctx, int(sample), ptr(cv), ptr(wt), og_height, og_width, int(h0),
                                        int(w0), int(hE), int(wE), torch.cuda.current_stream(self.device).cuda_stream))

    def add_images(self, samples, image_names, crop_info, og_heights, og_widths, probs=None) -> None:
        """ImageStitcher_v2.add_images (utils_image.py:386-406) without the image arrays -- crop i is sample samples[i] of
        the net's last eval forward, still resident on the device.  The whole list goes through ONE fu_stitch_add_batch
        launch, bit-identical to add_image for each crop in list order (also where crops of the list overlap).
        With probs (fp32 [N, H, W, k] on the device, e.g. HipUNet.merge_views' test-time-augmented probabilities),
        crop i adds probs[samples[i]] as it is instead of a softmax of the logits (fu_stitch_add_batch_probs): the same
        as canvas[box] += probs[s, :dh, :dw]; weight[box] += 1 in list order, bit for bit."""
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
        if probs is None:
            check(_lib.load().fu_stitch_add_batch(self.net._ctx, n, table, stream))
        else:
            check(_lib.load().fu_stitch_add_batch_probs(self.net._ctx, n, table, ptr(probs), probs.shape[0], stream))

    def combine(self, image_name: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (probabilities [H, W, n_classes], argmax [H, W]); like _combine_images + the argmax of predict.py."""
        cv, wt = self.image_canvas[image_name], self.weight_canvas[image_name]
        am = torch.empty(cv.shape[:2], dtype=torch.int64, device=self.device)
        check(_lib.load().fu_stitch_finalize(ptr(cv), ptr(wt), cv.shape[2], cv.shape[0], cv.shape[1], ptr(am),
                                             torch.cuda.current_stream(self.device).cuda_stream))
        return cv, am

    def drop(self, image_name: str) -> None:
        """Forget a finished image's canvases (after combine): their memory returns to the allocator, ordered on the
        current stream, so a run's footprint is bounded by the images in flight rather than by the run."""
        del self.image_canvas[image_name]
        del self.weight_canvas[image_name]
