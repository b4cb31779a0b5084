"""Input GB/s of the streaming band statistics (C ABI fu_band_stats) on one GPU, on the two bench shapes: B = 16 tiles of
8 x 256 x 256 and of 9 x 512 x 512, uniform values in [0, 1].  Per shape, device events around --launches launches after
warm-up, median:

  hist      fu_band_stats with the 4096-bin histogram (k_band_stats + k_band_stats_fold + k_band_hist_fold);
  no_hist   the same without a histogram;
  torch     for scale, the composition a user has without the kernel: x.double().sum, (x.double() ** 2).sum, amin, amax
            over (0, 2, 3) and torch.histc per channel -- it reads the input at least five times.

    python tools/band_stats_bench.py [--launches 50] [--warmup 5] [--mask nonzero|none]
Prints one JSON line; GB/s = input bytes / median time.  A one-pass kernel that loses to the composition is broken:
`hist_not_slower_than_torch` says so per shape."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from floodplanet_code_amd.datasets.stats import BandStats  # noqa: E402

SHAPES = {"b16_c8_256": (16, 8, 256, 256), "b16_c9_512": (16, 9, 512, 512)}


def _csrc_sha():
    """bench.py's hash of the kernel sources (profiles/ records builds by it)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "floodplanet_code_amd", "csrc")
    for fn in sorted(os.listdir(d)):
        if fn.endswith((".hip", ".h")):
            h.update(fn.encode())
            h.update(open(os.path.join(d, fn), "rb").read())
    return h.hexdigest()[:16]


def _median_ms(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def _torch_composition(x, bins):
    d = x.double()
    out = [d.sum((0, 2, 3)), (d ** 2).sum((0, 2, 3)), x.amin((0, 2, 3)), x.amax((0, 2, 3))]
    out += [torch.histc(x[:, c], bins=bins, min=0.0, max=1.0) for c in range(x.shape[1])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bins", type=int, default=4096)
    ap.add_argument("--mask", default="nonzero", choices=["nonzero", "none"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mask = None if args.mask == "none" else "nonzero"
    res = {"box": torch.cuda.get_device_name(dev), "csrc_sha": _csrc_sha(), "launches": args.launches, "bins": args.bins, "mask": args.mask}
    for name, shape in SHAPES.items():
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.rand(*shape, device=dev, generator=g)
        nbytes = x.numel() * 4
        with_hist = BandStats(shape[1], dev, bins=args.bins, mask=mask)
        without = BandStats(shape[1], dev, bins=None, mask=mask)
        ms = {"hist": _median_ms(lambda: with_hist.update([x]), args.launches, args.warmup),
              "no_hist": _median_ms(lambda: without.update([x]), args.launches, args.warmup),
              "torch": _median_ms(lambda: _torch_composition(x, args.bins), args.launches, args.warmup)}
        n = args.launches + args.warmup
        assert int(without.count[0]) == n * shape[0] * shape[2] * shape[3] - n * int((x.sum(1) == 0).sum())
        res[name] = {"input_MB": round(nbytes / 1e6, 1),
                     **{f"{k}_us": round(v * 1e3, 1) for k, v in ms.items()},
                     **{f"{k}_GBps": round(nbytes / (v * 1e-3) / 1e9, 1) for k, v in ms.items()},
                     "hist_not_slower_than_torch": ms["hist"] <= ms["torch"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
