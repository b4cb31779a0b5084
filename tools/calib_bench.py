"""Cost of the probability histogram (fu_eval_prob_hist) on one GPU, against the confusion counts of the same batch.

The bench's eval shape by default: batch 16, 256 x 256, 3 classes, 256 bins.  A tiny net's eval forward makes the context;
constructed fp32 NHWC logits are then copied over the resident ones (fu_test_loss_buffers), so the kernels read exactly
these two inputs:
  random     N(0, 2) logits: probabilities spread over the bins, lanes of a wave mostly in different bins
  saturated  every pixel the same logits (10, -10, ..) and the same target: every lane of every wave in the same bin of
             every histogram row -- the worst case for LDS-atomic contention, and what most of a flood scene looks like
and per input
  prob_hist       fu_eval_prob_hist, hist and top
  prob_hist_hist  fu_eval_prob_hist, hist only
  confusion       fu_eval_confusion, [B, k, k] counts: the yardstick, the same bytes read (k floats + one int64 per pixel)
Device times: --inner back-to-back calls between two events, divided by --inner; median of --repeats after --warmup
untimed ones, min / max beside it.  effective_GBps = bytes read / median time.  Ratios: saturated_over_random (prob_hist),
and prob_hist_over_confusion per input.  The first configuration is timed again at the end: its spread is the noise a
difference has to exceed.

    python tools/calib_bench.py [--batch 16] [--size 256] [--bins 256]
Prints one JSON line.  Run it on an otherwise idle GPU."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, inner, repeats, warmup):
    import torch
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
        samples.append(e0.elapsed_time(e1) / inner * 1e3)
    s = sorted(samples)
    return {"median_us": round(s[len(s) // 2], 3), "min_us": round(s[0], 3), "max_us": round(s[-1], 3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)

    import torch
    from floodplanet_code_amd import _lib
    from floodplanet_code_amd.unet import HipUNet

    dev = torch.device(args.device)
    lib = _lib.load()
    B, S, k, nb = args.batch, args.size, args.classes, args.bins
    net = HipUNet(1, k, base_channels=8).to(dev).eval()
    with torch.no_grad():
        net._forward_raw(torch.zeros(B, 1, S, S, device=dev), False, want_logits=False)
    lp, dp, n = C.c_void_p(), C.c_void_p(), C.c_int64()
    _lib.check(lib.fu_test_loss_buffers(net._ctx, C.byref(lp), C.byref(dp), C.byref(n)))
    assert n.value == B * S * S * k, (n.value, B, S, k)
    hip = C.CDLL("libamdhip64.so")                       # the process's HIP runtime (the one torch loaded)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int

    g = torch.Generator().manual_seed(0)
    sat = torch.full((k,), -10.0)
    sat[0] = 10.0
    inputs = {"random": (torch.randn(B, S, S, k, generator=g) * 2, torch.randint(0, k, (B, S, S), generator=g)),
              "saturated": (sat.expand(B, S, S, k).contiguous(), torch.zeros(B, S, S, dtype=torch.int64))}
    stream = torch.cuda.current_stream(dev).cuda_stream
    hist = torch.zeros(k, k, nb, dtype=torch.int64, device=dev)
    top = torch.zeros(2, nb, dtype=torch.int64, device=dev)
    counts = torch.zeros(B, k, k, dtype=torch.int64, device=dev)
    bytes_read = B * S * S * (4 * k + 8)
    out = {"batch": B, "size": S, "classes": k, "bins": nb, "device": torch.cuda.get_device_name(dev), "inner": args.inner,
           "repeats": args.repeats, "bytes_read": bytes_read}
    a = (args.inner, args.repeats, args.warmup)
    first = None
    for name, (logits, target) in inputs.items():
        ld, td = logits.to(dev), target.to(dev)
        torch.cuda.synchronize()
        assert hip.hipMemcpy(lp, C.c_void_p(ld.data_ptr()), n.value * 4, 3) == 0      # device to device
        torch.cuda.synchronize()

        def prob_hist(td=td, with_top=True):
            _lib.check(lib.fu_eval_prob_hist(net._ctx, td.data_ptr(), -100, nb, hist.data_ptr(),
                                             top.data_ptr() if with_top else None, stream))

        def confusion(td=td):
            _lib.check(lib.fu_eval_confusion(net._ctx, td.data_ptr(), -100, counts.data_ptr(), stream))

        entry = {"prob_hist": _timed(prob_hist, *a), "prob_hist_hist": _timed(lambda: prob_hist(with_top=False), *a),
                 "confusion": _timed(confusion, *a)}
        for v in entry.values():
            v["effective_GBps"] = round(bytes_read / v["median_us"] / 1e3, 1)
        entry["prob_hist_over_confusion"] = round(entry["prob_hist"]["median_us"] / entry["confusion"]["median_us"], 3)
        hist.zero_()
        top.zero_()
        prob_hist()
        entry["nonzero_bins"] = int((hist != 0).sum()) + int((top != 0).sum())
        assert int(top.sum()) == B * S * S and int(hist.sum()) == k * B * S * S
        out[name] = entry
        if first is None:
            first = (name, ld, prob_hist)
    out["saturated_over_random"] = round(out["saturated"]["prob_hist"]["median_us"] / out["random"]["prob_hist"]["median_us"], 3)
    assert hip.hipMemcpy(lp, C.c_void_p(first[1].data_ptr()), n.value * 4, 3) == 0
    torch.cuda.synchronize()
    out["prob_hist_again"] = dict(_timed(first[2], *a), input=first[0])
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
