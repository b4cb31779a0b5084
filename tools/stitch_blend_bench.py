"""Cost of window-weighted stitching and of the fused finalisation on one GPU.

A 1024 x 1024 canvas, k = 3, covered by 256 x 256 crops at stride 128 (49 crops), stitched in tables of --batch crops from
a probabilities tensor (the source that needs no network):
  (a) add_uniform    fu_stitch_add_batch_probs                       every table of the canvas, one launch each
  (b) add_windowed   fu_stitch_add_batch_windowed, hann windows      the same tables
and the canvas finalised two ways (on the raw sums of (a), restored by a device copy that is timed on its own and
subtracted):
  (c) finalize_chain fu_stitch_finalize, then clamp(0, 1) * 255 -> uint8, bincount and cat in torch: what infer ran
  (d) finalize_maps  fu_stitch_finalize_maps: class map + counts in one launch, then the same cat
  (e) finalize_maps_all  (d) with the uint8 probability bands and the margin as well
Each sample is the device time of --inner back-to-back calls between two events, divided by --inner; a figure is the
median of --repeats samples after --warmup untimed ones, with min / max beside it.  GB/s is the bytes the algorithm needs
(computed from the shapes, below) over the median; it is not a share of peak.  (a) and (c) are timed a second time at the
end: their spread is the noise a difference has to exceed.

    python tools/stitch_blend_bench.py [--canvas 1024] [--crop 256] [--stride 128] [--batch 16]
Prints one JSON line.  Run it on an otherwise idle GPU."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from floodplanet_code_amd import _lib  # noqa: E402
from floodplanet_code_amd.stitch import GpuImageStitcher, blend_window  # noqa: E402
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


def _gbps(nbytes, entry):
    entry["bytes"] = int(nbytes)
    entry["GBps"] = round(nbytes / (entry["median_ms"] * 1e-3) / 1e9, 1) if entry["median_ms"] > 0 else None
    return entry


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--canvas", type=int, default=1024)
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--stride", type=int, default=128)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    lib = _lib.load()
    torch.manual_seed(0)
    S, T, k, B = args.canvas, args.crop, args.classes, args.batch

    net = HipUNet(2, k, base_channels=8).to(dev).eval()       # the stitch entries need a context of the tile size only
    net._get_ctx(dev, B, T, T)
    starts = list(range(0, S - T + 1, args.stride))
    boxes = [(h, w, h + T, w + T) for h in starts for w in starts]
    probs = torch.rand(B, T, T, k, device=dev)
    probs /= probs.sum(-1, keepdim=True)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def tables(st):
        st.image_canvas["c"] = torch.zeros(S, S, k, device=dev)
        st.weight_canvas["c"] = torch.zeros(S, S, device=dev)
        cv, wt = st.image_canvas["c"], st.weight_canvas["c"]
        out = []
        for j in range(0, len(boxes), B):
            part = boxes[j:j + B]
            out.append((len(part), (_lib.FuStitchEntry * len(part))(
                *[_lib.FuStitchEntry(cv.data_ptr(), wt.data_ptr(), i, S, S, *b, 0) for i, b in enumerate(part)])))
        return out

    uni, win = GpuImageStitcher(net, dev), GpuImageStitcher(net, dev, blend="hann")
    uni_tables, win_tables = tables(uni), tables(win)
    wy = torch.from_numpy(blend_window("hann", T)).to(dev)

    def add_uniform():
        for n, tab in uni_tables:
            _lib.check(lib.fu_stitch_add_batch_probs(net._ctx, n, tab, probs.data_ptr(), B, stream))

    def add_windowed():
        for n, tab in win_tables:
            _lib.check(lib.fu_stitch_add_batch_windowed(net._ctx, n, tab, probs.data_ptr(), B, wy.data_ptr(), wy.data_ptr(),
                                                        stream))

    # bytes of the adds: per covered canvas pixel one read and one write of k + 1 floats per table that touches it, and per
    # crop pixel k floats of probabilities (+ two window floats, from cache); counted from the tables themselves
    add_bytes = 0
    for j in range(0, len(boxes), B):
        touched = torch.zeros(S, S, dtype=torch.bool)
        for h0, w0, hE, wE in boxes[j:j + B]:
            touched[h0:hE, w0:wE] = True
            add_bytes += T * T * k * 4
        add_bytes += int(touched.sum()) * (k + 1) * 4 * 2

    add_uniform()
    torch.cuda.synchronize()
    cv, wt = uni.image_canvas["c"], uni.weight_canvas["c"]
    raw = cv.clone()
    am = torch.empty(S, S, dtype=torch.int64, device=dev)
    cls = torch.empty(S, S, dtype=torch.uint8, device=dev)
    pq = torch.empty(k, S, S, dtype=torch.uint8, device=dev)
    mg = torch.empty(S, S, dtype=torch.uint8, device=dev)
    counts = torch.zeros(k, dtype=torch.int64, device=dev)
    values = (ctypes.c_uint8 * k)(*([0] + [255] * (k - 1)))

    def restore():
        cv.copy_(raw)

    def finalize_chain():
        restore()
        _lib.check(lib.fu_stitch_finalize(cv.data_ptr(), wt.data_ptr(), k, S, S, am.data_ptr(), stream))
        c8 = (am.clamp(0, 1) * 255).to(torch.uint8)
        n = torch.bincount(am.view(-1), minlength=k)
        return torch.cat([n.view(torch.uint8), c8.view(-1)])

    def finalize_maps(everything=False):
        restore()
        counts.zero_()
        _lib.check(lib.fu_stitch_finalize_maps(cv.data_ptr(), wt.data_ptr(), k, S, S, 1e-5, 1, values, cls.data_ptr(),
                                               pq.data_ptr() if everything else None, mg.data_ptr() if everything else None,
                                               counts.data_ptr(), stream))
        parts = [counts.view(torch.uint8), cls.view(-1)] + ([pq.view(-1), mg.view(-1)] if everything else [])
        return torch.cat(parts)

    npix = S * S
    fin_bytes = npix * ((k + 1) * 4 + k * 4)                    # canvas + weight read, canvas written
    out = {"canvas": S, "crop": T, "stride": args.stride, "crops": len(boxes), "tables": len(uni_tables), "classes": k,
           "device": torch.cuda.get_device_name(dev), "inner": args.inner, "repeats": args.repeats}
    with torch.no_grad():
        a = (args.inner, args.repeats, args.warmup)
        out["add_uniform"] = _gbps(add_bytes, _timed(add_uniform, *a))
        out["add_windowed"] = _gbps(add_bytes, _timed(add_windowed, *a))
        out["restore_copy"] = _timed(restore, *a)
        out["finalize_chain"] = _timed(finalize_chain, *a)
        out["finalize_maps"] = _timed(finalize_maps, *a)
        out["finalize_maps_all"] = _timed(lambda: finalize_maps(True), *a)
        out["add_uniform_again"] = _timed(add_uniform, *a)
        out["finalize_chain_again"] = _timed(finalize_chain, *a)
    copy_ms = out["restore_copy"]["median_ms"]
    for name, extra in (("finalize_chain", npix * 8 + npix), ("finalize_maps", npix),
                        ("finalize_maps_all", npix * (2 + k))):
        e = out[name]
        e["less_copy_ms"] = round(e["median_ms"] - copy_ms, 5)
        e["bytes"] = int(fin_bytes + extra)                    # the least the outputs need: the chain's int64 map counts once
        e["GBps"] = round(e["bytes"] / (e["less_copy_ms"] * 1e-3) / 1e9, 1) if e["less_copy_ms"] > 0 else None
    out["add_spread_ms"] = round(max(out[n]["max_ms"] - out[n]["min_ms"] for n in ("add_uniform", "add_uniform_again")), 5)
    out["finalize_spread_ms"] = round(max(out[n]["max_ms"] - out[n]["min_ms"]
                                          for n in ("finalize_chain", "finalize_chain_again")), 5)
    out["maps_faster_than_chain"] = out["finalize_maps"]["median_ms"] < out["finalize_chain"]["median_ms"]
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
