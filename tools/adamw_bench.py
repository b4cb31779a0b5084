"""Cost of the decoupled weight decay inside the fused Adam launch on one GPU, at the bench shape (UNet base 64, 8 bands:
17.27 M parameters).

The optimiser launch alone, on the net's own flat buffers with a random gradient, four variants:
  plain        fu_adam_step,     decay off   (k_adam)            7 streams of n floats
  ema          fu_adam_ema_step, decay off   (k_adam_ema)        9 streams
  decayed      fu_adam_step,     decay on    (k_adamw)           7 streams + the bounds table (a few hundred bytes, in LDS)
  decayed_ema  fu_adam_ema_step, decay on    (k_adamw_ema)       9 streams + the table
The variants are interleaved: each of --rounds rounds times every variant once, so that drift of the clocks falls on all of
them alike.  A sample is the device time of --inner back-to-back launches between two events, divided by --inner; a figure is
the median over the rounds with min / max beside it and the achieved GB/s of the median (streams * 4 bytes * n).
`decay_surcharge_us` / `decay_ema_surcharge_us` are decayed - plain on the medians; `plain_spread_us` / `ema_spread_us` the
max - min of the undecayed variants, to read them against.  --decay_all decays every tensor (one range) instead of the
ndim >= 2 tensors (a few dozen ranges).

    python tools/adamw_bench.py [--rounds 30] [--inner 20] [--decay_all]
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


def _sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weight_decay", type=float, default=0.01)
    ap.add_argument("--decay_all", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    lib = _lib.load()
    torch.manual_seed(0)

    net = HipUNet(args.channels, 3, base_channels=args.base).to(dev).train()
    net._get_ctx(dev, 1, 64, 64)                              # the context and the flat buffers; the tile shape does not matter
    net.enable_ema(0.999)
    net.flat_grads().normal_().mul_(1e-3)
    stream = net._stream(dev)
    adam = (1e-4, 0.9, 0.999, 1e-8, 100, 1.0)

    def step():
        _lib.check(lib.fu_adam_step(net._ctx, *adam, stream))

    def ema_step():
        _lib.check(lib.fu_adam_ema_step(net._ctx, *adam, 0.999, stream))

    variants = (("plain", step, 0.0, 7), ("ema", ema_step, 0.0, 9), ("decayed", step, args.weight_decay, 7),
                ("decayed_ema", ema_step, args.weight_decay, 9))
    samples = {name: [] for name, _, _, _ in variants}
    with torch.no_grad():
        for r in range(args.warmup + args.rounds):
            for name, fn, wd, _ in variants:
                net.set_weight_decay(wd, "all" if args.decay_all else "weights")
                fn()                                          # (the first launch after arming is not timed)
                torch.cuda.synchronize()
                t = _sample(fn, args.inner)
                if r >= args.warmup:
                    samples[name].append(t)
    net.set_weight_decay(args.weight_decay, "all" if args.decay_all else "weights")
    out = {"parameters": net._total, "tensors": len(net._table), "decayed_tensors": len(net.decayed_parameter_names()),
           "device": torch.cuda.get_device_name(dev), "inner": args.inner, "rounds": args.rounds,
           "weight_decay": args.weight_decay, "decay_all": bool(args.decay_all)}
    net.set_weight_decay(0.0)
    for name, _, _, streams in variants:
        s = sorted(samples[name])
        med = s[len(s) // 2]
        out[name] = {"median_ms": round(med, 5), "min_ms": round(s[0], 5), "max_ms": round(s[-1], 5),
                     "gb_per_s": round(streams * 4 * net._total / (med * 1e-3) / 1e9, 1)}
    us = lambda k: 1e3 * out[k]["median_ms"]                                                  # noqa: E731
    spread = lambda k: round(1e3 * (out[k]["max_ms"] - out[k]["min_ms"]), 2)                  # noqa: E731
    out["plain_spread_us"], out["ema_spread_us"] = spread("plain"), spread("ema")
    out["decay_surcharge_us"] = round(us("decayed") - us("plain"), 2)
    out["decay_ema_surcharge_us"] = round(us("decayed_ema") - us("ema"), 2)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
