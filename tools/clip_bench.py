"""Cost of global-norm gradient clipping on one GPU, at the bench shape (UNet base 64, 8 bands: 17.27 M parameters).

Optimiser step alone, on the net's own flat buffers with a real gradient:
  (a) fu_adam_step, clipping off     (k_adam)                                           the step as it was
  (b) fu_adam_step, clipping on      (k_grad_sqnorm_chunks, k_grad_norm_finalize, k_adam_dev)
  (c) fu_grad_norms                  (k_grad_sqnorm_chunks, k_grad_norm_finalize)       the two norm launches by themselves
(b) runs with max_norm = 1e30, so that its coefficient is 1 and the parameters follow (a)'s path.  Each sample is the device
time of --inner back-to-back calls between two events, divided by --inner; a figure is the median of --repeats samples after
--warmup untimed ones, with min / max beside it.  `clip_surcharge_us` is (b) - (a) on the medians; `a_spread_us` the
max - min of (a), measured twice, to read it against.  A kernel trace of this tool (rocprofv3 --kernel-trace --stats)
splits (c) into its two launches.

Whole training step (forward + CE + backward + optimiser, batch 16 of 256 x 256 tiles, --precision), eager trainer, clipping
off, on, off again.  With clipping off the step issues exactly the launches it issued before clipping existed.

    python tools/clip_bench.py [--precision bf16] [--repeats 30] [--inner 20]
Prints one JSON line.  Run it on an otherwise idle GPU."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from floodplanet_code_amd import _lib  # noqa: E402
from floodplanet_code_amd.unet import HipUNet  # noqa: E402


def _timed(fn, inner, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        samples.append(e0.elapsed_time(e1) / inner)
    s = sorted(samples)
    return {"median_ms": round(s[len(s) // 2], 5), "min_ms": round(s[0], 5), "max_ms": round(s[-1], 5)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-repeats", type=int, default=30)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    lib = _lib.load()
    torch.manual_seed(0)

    net = HipUNet(args.channels, 3, base_channels=args.base, precision=args.precision).to(dev).train()
    x = torch.rand(args.batch, args.channels, args.size, args.size, device=dev)
    t = torch.randint(0, 3, (args.batch, args.size, args.size), device=dev)
    net.train_step(x, t, 0)                                   # the context, the flat buffers and a real gradient
    stream = net._stream(dev)
    adam = (1e-4, 0.9, 0.999, 1e-8, 100, 1.0)
    norms = torch.zeros(len(net._table) + 1, device=dev)

    def step():
        _lib.check(lib.fu_adam_step(net._ctx, *adam, stream))

    def report():
        _lib.check(lib.fu_grad_norms(net._ctx, 1.0, norms.data_ptr(), stream))

    out = {"parameters": net._total, "tensors": len(net._table), "precision": args.precision,
           "device": torch.cuda.get_device_name(dev), "inner": args.inner, "repeats": args.repeats}
    with torch.no_grad():
        for name, clip, fn in (("a_adam_clip_off", None, step), ("b_adam_clip_on", 1e30, step), ("c_norm_launches", None, report),
                               ("a_adam_clip_off_again", None, step)):
            net.set_grad_clip(clip)
            out[name] = _timed(fn, args.inner, args.repeats, args.warmup)
    net.set_grad_clip(None)
    us = lambda k: 1e3 * out[k]["median_ms"]                                                  # noqa: E731
    out["a_spread_us"] = round(1e3 * max(out[k]["max_ms"] - out[k]["min_ms"] for k in ("a_adam_clip_off", "a_adam_clip_off_again")), 2)
    out["clip_surcharge_us"] = round(us("b_adam_clip_on") - min(us("a_adam_clip_off"), us("a_adam_clip_off_again")), 2)
    out["norm_launches_us"] = round(us("c_norm_launches"), 2)
    out["gradient_norm"] = float(norms[-1])

    # the whole step, clipping off and on (off: the step as it was before clipping existed)
    from floodplanet_code_amd.distributed import DataParallelTrainer
    for name, clip in (("step_clip_off", None), ("step_clip_on", 1e30), ("step_clip_off_again", None)):
        net.set_grad_clip(clip)
        tr = DataParallelTrainer(net, lr=1e-4)
        tr.step_count = 100
        out[name] = _timed(lambda: tr.step(x, t, 0), 1, args.step_repeats, args.warmup)
    out["step_delta_ms"] = round(out["step_clip_on"]["median_ms"]
                                 - min(out["step_clip_off"]["median_ms"], out["step_clip_off_again"]["median_ms"]), 5)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
