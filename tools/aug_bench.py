"""Per-batch time of fu_scene_train_tiles_ex's radiometric and zoom parts against the plain launch, on one GPU, at
16 x 8 x 256 x 256 (--batch, --channels, --tile) from synthetic scenes made on the device (nothing is read from disk).

Arms, all through the C ABI with tables, host arrays and buffers made beforehand, the same boxes (zoom: the same centres),
flags and angles (augment.sample_transforms' default draws):

  plain        fu_scene_train_tiles
  ex_null      fu_scene_train_tiles_ex with a NULL struct (must be the plain launch)
  gain_bias    gain and bias, no noise: the sibling kernel without the Philox rounds
  photometric  gain, bias and sigma: one Philox4x32-10 per output value
  zoom         out size = the tile, source boxes 1 / z the size, z log-uniform in [0.5, 2]
  combined     zoom + photometric

Device events around enough back-to-back calls to pass --min_ms, warm-up excluded, arms interleaved, median of --samples.
This times whole CALLS -- host validation, the table's host-to-device copy and the launch included --, not kernel time;
kernel time proper comes from a run of its own under rocprofv3 --kernel-trace --stats.  Bytes: what each arm must read and
write, from the shapes (zoom reads its source boxes once; the four taps of a pixel are served from L2).

    python tools/aug_bench.py [--samples 7] [--norm_mode none|local] [--arms plain,zoom]
One JSON object on the last line."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from floodplanet_code_amd import _lib, augment  # noqa: E402
from floodplanet_code_amd.datasets import sampling  # noqa: E402
from floodplanet_code_amd.unet import HipUNet  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--scene", type=int, default=1024, help="side of the four synthetic scenes")
    ap.add_argument("--norm_mode", type=str, default="none", choices=["none", "local"])
    ap.add_argument("--arms", type=str, default="plain,ex_null,gain_bias,photometric,zoom,combined",
                    help="comma-separated subset (gain_bias and photometric share a kernel: trace them in separate runs)")
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--min_ms", type=float, default=20.0)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    n, C_, T, S = args.batch, args.channels, args.tile, args.scene
    lib = _lib.load()
    net = HipUNet(2, 3, base_channels=8).to(dev)
    ctx = net._get_ctx(dev, 1, 32, 32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(0)
    scenes = [torch.rand(C_, S, S, device=dev, generator=g) for _ in range(4)]
    labels = [torch.randint(0, 3, (S, S), device=dev, generator=g, dtype=torch.uint8) for _ in range(4)]
    rng = np.random.RandomState(0)
    flags, angles = augment.sample_transforms(n, {}, rng)
    origin = rng.randint(0, S - T + 1, size=(n, 2))
    boxes = [(int(y), int(x), int(y) + T, int(x) + T) for y, x in origin]
    src_boxes, out_sizes = sampling.zoom_boxes(boxes, [(S, S)] * n, (0.5, 2.0), seed=0, epoch=0)

    def table(bx):
        return (_lib.FuSceneTrainEntry * n)(*[
            _lib.FuSceneTrainEntry(scenes[i % 4].data_ptr(), labels[i % 4].data_ptr(), S, S, *bx[i], int(flags[i]),
                                   float(angles[i])) for i in range(n)])
    plain_tab, zoom_tab = table(boxes), table(src_boxes)
    draws = augment.sample_photometric(n, C_, dict(gain=0.2, band_gain=0.1, brightness=0.2, noise=0.1), rng)
    streams = np.arange(n, dtype=np.uint64)
    out_h = np.array([o[0] for o in out_sizes], dtype=np.int32)
    out_w = np.array([o[1] for o in out_sizes], dtype=np.int32)
    p = lambda a: None if a is None else a.ctypes.data
    structs = {
        "gain_bias": _lib.FuSceneAug(p(draws["gain"]), p(draws["bias"]), None, None, 0, None, None),
        "photometric": _lib.FuSceneAug(p(draws["gain"]), p(draws["bias"]), p(draws["sigma"]), p(streams), 12345, None, None),
        "zoom": _lib.FuSceneAug(None, None, None, None, 0, p(out_h), p(out_w)),
        "combined": _lib.FuSceneAug(p(draws["gain"]), p(draws["bias"]), p(draws["sigma"]), p(streams), 12345, p(out_h), p(out_w)),
    }
    image = torch.empty(n, C_, T, T, device=dev)
    target = torch.empty(n, T, T, dtype=torch.int64, device=dev)
    mean, std = torch.zeros(n, C_, device=dev), torch.ones(n, C_, device=dev)
    mode = {"none": 0, "local": 1}[args.norm_mode]
    m, s = (mean.data_ptr(), std.data_ptr()) if mode == 1 else (None, None)
    common = (C_, T, T, mode, None, None, 0.0, 0, 0, image.data_ptr(), target.data_ptr(), m, s)

    def arm(name):
        if name == "plain":
            return lambda: _lib.check(lib.fu_scene_train_tiles(ctx, n, plain_tab, *common, stream))
        if name == "ex_null":
            return lambda: _lib.check(lib.fu_scene_train_tiles_ex(ctx, n, plain_tab, *common, None, stream))
        tab = zoom_tab if name in ("zoom", "combined") else plain_tab
        ref = ctypes.byref(structs[name])
        return lambda: _lib.check(lib.fu_scene_train_tiles_ex(ctx, n, tab, *common, ref, stream))
    arms = {k: arm(k) for k in args.arms.split(",")}

    def sample(fn):
        reps = 64
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= args.min_ms:
                return ms * 1e3 / reps                   # us per call
            reps *= 4
    for fn in arms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize(dev)
    got = {k: [] for k in arms}
    for _ in range(args.samples):
        for k, fn in arms.items():
            got[k].append(sample(fn))
    written = n * C_ * T * T * 4 + n * T * T * 8
    stats_pass = 2 if mode == 1 else 0                   # 'local': the statistics read the box twice more (from L2)
    read_plain = n * T * T * (C_ * 4 + 1)
    read_zoom = sum((hE - h0) * (wE - w0) for h0, w0, hE, wE in src_boxes) * (C_ * 4 + 1)
    out = {"shape": [n, C_, T, T], "norm_mode": args.norm_mode, "samples": args.samples, "us_per_call": {}, "MB_moved": {},
           "GBps": {}, "zoom_source_pixels_over_tile_pixels": round(read_zoom / read_plain, 3),
           "rotated": int((flags & 4).astype(bool).sum()), "stats_passes_from_L2": stats_pass}
    for k, v in got.items():
        us = statistics.median(v)
        moved = written + (read_zoom if k in ("zoom", "combined") else read_plain)
        out["us_per_call"][k] = {"median": round(us, 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        out["MB_moved"][k] = round(moved / 1e6, 2)
        out["GBps"][k] = round(moved / us / 1e3, 1)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
