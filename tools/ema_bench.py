"""Cost of the weight EMA on one GPU, at the bench shape (UNet base 64, 8 bands: 17.27 M parameters).

Optimiser launch alone, on the net's own flat buffers with a random gradient, three ways:
  (a) fu_adam_step      (k_adam)                                7 streams of n floats
  (b) fu_adam_ema_step  (k_adam_ema)                            9 streams, one launch (running statistics included)
  (c) fu_adam_step, then ema.lerp_(params, w) in torch, plus the two running-statistics lerp_ calls
                                                                10 streams, four launches
Each sample is the device time of --inner back-to-back calls between two events, divided by --inner; a figure is the
median of --repeats samples after --warmup untimed ones, with min / max beside it.  The requirement the tool checks is
(b) <= (c) + the spread (max - min) it measured for (a); `b_not_slower_than_c` says whether it held.

Whole training step (forward + CE + backward + optimiser, batch 16 of 256 x 256 tiles, --precision), eager trainer, EMA
off and on, same way.  With the EMA off the step calls fu_adam_step, as it did before the EMA existed.

    python tools/ema_bench.py [--precision bf16] [--repeats 30] [--inner 20]
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
    net.enable_ema(0.999)
    ema_p, ema_rm, ema_rv = net.ema_buffers()
    stream = net._stream(dev)
    adam = (1e-4, 0.9, 0.999, 1e-8, 100, 1.0)
    w = 0.001

    def a():
        _lib.check(lib.fu_adam_step(net._ctx, *adam, stream))

    def b():
        _lib.check(lib.fu_adam_ema_step(net._ctx, *adam, w, stream))

    def c():
        _lib.check(lib.fu_adam_step(net._ctx, *adam, stream))
        ema_p.lerp_(net._flat, w)
        ema_rm.lerp_(net._flat_rm, w)
        ema_rv.lerp_(net._flat_rv, w)

    out = {"parameters": net._total, "bn_channels": net._total_bn, "precision": args.precision,
           "device": torch.cuda.get_device_name(dev), "inner": args.inner, "repeats": args.repeats}
    with torch.no_grad():
        for name, fn in (("a_adam", a), ("b_adam_ema", b), ("c_adam_then_torch_lerp", c), ("a_adam_again", a)):
            out[name] = _timed(fn, args.inner, args.repeats, args.warmup)
    spread = max(out[k]["max_ms"] - out[k]["min_ms"] for k in ("a_adam", "a_adam_again"))
    out["a_spread_ms"] = round(spread, 5)
    out["b_not_slower_than_c"] = out["b_adam_ema"]["median_ms"] <= out["c_adam_then_torch_lerp"]["median_ms"] + spread

    # the whole step, EMA off and on (off: fu_adam_step, the step as it was before the EMA existed)
    from floodplanet_code_amd.distributed import DataParallelTrainer
    for name, decay in (("step_ema_off", None), ("step_ema_on", 0.999), ("step_ema_off_again", None)):
        if decay is None:
            net.disable_ema()
        tr = DataParallelTrainer(net, lr=1e-4, ema_decay=decay)
        tr.step_count = 100
        out[name] = _timed(lambda: tr.step(x, t, 0), 1, args.step_repeats, args.warmup)
    out["step_delta_ms"] = round(out["step_ema_on"]["median_ms"]
                                 - min(out["step_ema_off"]["median_ms"], out["step_ema_off_again"]["median_ms"]), 5)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
