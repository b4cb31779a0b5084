"""What a scene's overview pyramid costs, measured on one GPU (datasets/overviews.py, C ABI fu_map_overviews).

  (a) kernel   fu_map_overviews alone, device-event time, on a --size x --size grid (4096), per kind: the uint8 class map
               (mode_u8, with a nodata value), a uint8 three-band raster and the fp32 three-band canvas read through its
               [H, W, k] strides (mean_u8 and mean_f32, with a valid mask), and the mask itself (any_u8); all levels down to
               one 512-pixel tile (--side), which is one launch up to six levels.  --inner back-to-back calls between two
               events, median of --repeats after --warmup, min / max beside it, in microseconds.  Bytes: the raster (and
               the mask) read once, every level (and mask level) written once, and their rate over the median.  Beside it
               fu_tiff_pack of the same raster in --side tiles without a predictor, timed the same way: the other pass
               over the raster that writing a scene makes.  With --check the levels are compared with overviews_host once
               per case.
  (b) host     the numpy statement overviews_host on the same inputs, seconds (median of --host_repeats): what the host
               would spend per raster if the levels were cut there.

    python tools/overview_bench.py [--size 4096] [--check]
Prints one JSON line.  Run it on an otherwise idle GPU."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from floodplanet_code_amd import _lib  # noqa: E402
from floodplanet_code_amd.datasets import geotiff as G  # noqa: E402
from floodplanet_code_amd.datasets import geotiff_write as GW  # noqa: E402
from floodplanet_code_amd.datasets import overviews as OV  # noqa: E402


def _stats(samples, scale=1.0, digits=5):
    s = sorted(samples)
    return {"median": round(s[len(s) // 2] * scale, digits), "min": round(s[0] * scale, digits),
            "max": round(s[-1] * scale, digits)}


def _timed(launch, args):
    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    samples = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            launch()
        e1.record()
        e1.synchronize()
        samples.append(e0.elapsed_time(e1) / args.inner)
    return _stats(samples, scale=1e3, digits=2)


def _rasters(S, K, dev, seed=1):
    """A class map of water blobs (0 / 255) with a corner of nodata (127), a smooth canvas [S, S, K] of probabilities, its
    uint8 bands [K, S, S] and the valid mask, on the device."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    coarse = torch.rand(1, K, max(S // 64, 2), max(S // 64, 2), generator=g)
    field = torch.nn.functional.interpolate(coarse, size=(S, S), mode="bilinear", align_corners=False)[0]
    canvas = torch.softmax(field * 6, dim=0).permute(1, 2, 0).contiguous().to(dev)
    valid = torch.ones(S, S, dtype=torch.uint8, device=dev)
    valid[: S // 5, : S // 4] = 0
    cls = (canvas.argmax(dim=2) > 0).to(torch.uint8) * 255
    cls[valid == 0] = 127
    probs = (canvas.permute(2, 0, 1) * 255).round().to(torch.uint8).contiguous()
    return cls.contiguous(), canvas, probs, valid


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host_repeats", type=int, default=3)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("overview_bench needs the GPU: nothing here is a measurement without it")
    dev = torch.device(args.device)
    lib = _lib.load()
    S = args.size
    n = OV.auto_levels(S, S, args.side)
    sizes = OV.overview_sizes(S, S, n)
    pixels = sum(h * w for h, w in sizes)
    out = {"size": S, "levels": n, "device": torch.cuda.get_device_name(dev), "inner": args.inner, "repeats": args.repeats,
           "kernel": {}}
    with torch.no_grad():
        cls, canvas, probs, valid = _rasters(S, 3, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        cases = {"mode_u8_map": (cls[None], "mode_u8", None, 127), "mean_u8_x3": (probs, "mean_u8", valid, None),
                 "mean_f32_x3_canvas": (canvas.permute(2, 0, 1), "mean_f32", valid, None),
                 "any_u8_mask": (valid[None], "any_u8", None, None)}
        for name, (t, kind, mask, nodata) in cases.items():
            k = int(t.shape[0])
            dst = torch.empty(k * pixels, dtype=t.dtype, device=dev)
            vdst = torch.empty(pixels, dtype=torch.uint8, device=dev) if mask is not None else None
            call = (t.data_ptr(), *[int(s) for s in t.stride()], k, S, S, OV.KINDS[kind], _lib.ptr(mask),
                    -1 if nodata is None else nodata, n, dst.data_ptr(), dst.numel(), _lib.ptr(vdst), stream)
            entry = {"us": _timed(lambda: _lib.check(lib.fu_map_overviews(*call)), args)}
            read = t.numel() * t.element_size() + (S * S if mask is not None else 0)
            written = dst.numel() * dst.element_size() + (pixels if mask is not None else 0)
            entry.update(bytes_read=read, bytes_written=written,
                         GB_per_s=round((read + written) / (entry["us"]["median"] * 1e-6) / 1e9, 1))
            L = GW.raster_layout(np.float32 if kind == "mean_f32" else np.uint8, S, S, k, tile=args.side)
            total = GW.check_pack_layout(L)
            packed = torch.empty(total, dtype=torch.uint8, device=dev)
            pack = (t.data_ptr(), *[int(s) for s in t.stride()], G.layout_struct(L), packed.data_ptr(), total, stream)
            entry["tiff_pack_us"] = _timed(lambda: _lib.check(lib.fu_tiff_pack(*pack)), args)
            entry["tiff_pack_bytes"] = t.numel() * t.element_size() + total
            host_in = t.cpu().numpy()
            host_kw = dict(valid=mask.cpu().numpy()) if mask is not None else dict(nodata_value=nodata) if nodata is not None \
                else dict()
            runs = []
            for _ in range(args.host_repeats):
                t0 = time.perf_counter()
                want = OV.overviews_host(host_in, kind, n, **host_kw)
                runs.append(time.perf_counter() - t0)
            entry["overviews_host_s"] = _stats(runs, digits=4)
            if args.check:
                levels = want[0] if isinstance(want, tuple) else want
                flat = np.concatenate([x.reshape(-1) for x in levels])
                entry["equals_host"] = bool(np.array_equal(dst.cpu().numpy().view(np.uint8), flat.view(np.uint8)))
            out["kernel"][name] = entry
            del dst, packed
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
