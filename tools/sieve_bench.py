"""Cost of connected-component labelling and of the sieve on one GPU, and what the sieve adds to a scene's finalisation.

A --size x --size uint8 map (1024: the label rasters' size), three inputs:
  speckled      smooth blobs (a thresholded low-pass field) with --speckle of the pixels flipped: what a class map looks like
  one_value     a single component: every pixel meets at one root, the worst contention
  checkerboard  every pixel its own component under 4-connectivity, the most components (two under 8)
and per input
  components_4 / components_8   fu_map_components                     (tile, seams, flatten: three launches)
  sieve_4 / sieve_8             fu_map_sieve, --min_pixels, one pass  (those three with the size count, donor, apply)
so sieve minus components is the cost of the count, the donor pass and the apply pass.
Then a scene's finalisation as infer runs it, on a canvas whose argmax is the speckled map:
  finalize        fu_stitch_finalize_maps (class map + counts), the packed device-to-host read, the strip-TIFF write
  finalize_sieve  the same with the sieve between the launch and the read, its two counts riding in the read
both as host wall time per scene (the read synchronises), median of --repeats; sieve_added_fraction is the difference
over `finalize`.  Device times: --inner back-to-back calls between two events, divided by --inner; median of --repeats
after --warmup untimed ones, min / max beside it.  The first configuration is timed again at the end: its spread is the
noise a difference has to exceed.

    python tools/sieve_bench.py [--size 1024] [--min_pixels 25]
Prints one JSON line.  Run it on an otherwise idle GPU."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from floodplanet_code_amd import _lib  # noqa: E402
from floodplanet_code_amd import postprocess as PP  # noqa: E402
from floodplanet_code_amd.datasets.synthetic import write_strip_tiff  # noqa: E402


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


def _wall(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        samples.append((time.perf_counter() - t0) * 1e3)
    s = sorted(samples)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4)}


def speckled_map(S, speckle, seed=0):
    g = np.random.default_rng(seed)
    f = g.standard_normal((S, S))
    F = np.fft.rfft2(f)
    ky, kx = np.fft.fftfreq(S)[:, None], np.fft.rfftfreq(S)[None, :]
    f = np.fft.irfft2(F * np.exp(-(ky ** 2 + kx ** 2) * (S / 16.0) ** 2), s=(S, S))      # blobs of some tens of pixels
    m = (f > np.quantile(f, 0.7)).astype(np.uint8)
    return m ^ (g.random((S, S)) < speckle).astype(np.uint8)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--min_pixels", type=int, default=25)
    ap.add_argument("--speckle", type=float, default=0.03)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    lib = _lib.load()
    S, k = args.size, args.classes
    stream = torch.cuda.current_stream(dev).cuda_stream

    inputs = {"speckled": speckled_map(S, args.speckle),
              "one_value": np.ones((S, S), np.uint8),
              "checkerboard": (np.indices((S, S)).sum(0) % 2).astype(np.uint8)}
    labels = torch.empty(S, S, dtype=torch.int32, device=dev)
    sieved = torch.empty(S, S, dtype=torch.uint8, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    nbytes = int(lib.fu_sieve_workspace_bytes(S, S))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    out = {"size": S, "min_pixels": args.min_pixels, "speckle": args.speckle, "device": torch.cuda.get_device_name(dev),
           "inner": args.inner, "repeats": args.repeats, "workspace_bytes": nbytes}
    a = (args.inner, args.repeats, args.warmup)
    first = None
    for name, m in inputs.items():
        md = torch.from_numpy(m).to(dev)
        entry = {}
        for conn in (4, 8):
            def components(md=md, conn=conn):
                _lib.check(lib.fu_map_components(md.data_ptr(), S, S, conn, labels.data_ptr(), stream))

            def sieve(md=md, conn=conn):
                _lib.check(lib.fu_map_sieve(md.data_ptr(), sieved.data_ptr(), S, S, conn, args.min_pixels, -1, 1,
                                            ws.data_ptr(), nbytes, stats.data_ptr(), stream))

            entry[f"components_{conn}"] = _timed(components, *a)
            entry[f"sieve_{conn}"] = _timed(sieve, *a)
            if first is None:
                first = (name, components)
        stats.zero_()
        sieve()
        entry["n_components_8"] = int(torch.unique(labels).numel())
        entry["merged_components_8"], entry["changed_pixels_8"] = stats.cpu().tolist()
        out[name] = entry
    out["components_again"] = dict(_timed(first[1], *a), input=first[0] + ", connectivity 4")

    # a scene's finalisation: the canvas holds one-hot probabilities of the speckled map, so its class map is that map
    cls_idx = torch.from_numpy(inputs["speckled"].astype(np.int64)).to(dev)
    raw = torch.nn.functional.one_hot(cls_idx, k).float().contiguous()
    cv = raw.clone()
    wt = torch.ones(S, S, device=dev)
    cls = torch.empty(S, S, dtype=torch.uint8, device=dev)
    counts = torch.zeros(k, dtype=torch.int64, device=dev)
    values = (ctypes.c_uint8 * k)(*([0] + [255] * (k - 1)))
    tmp = tempfile.mkdtemp(prefix="sieve_bench_")
    path = os.path.join(tmp, "scene.tif")

    def finalize(with_sieve):
        cv.copy_(raw)
        counts.zero_()
        _lib.check(lib.fu_stitch_finalize_maps(cv.data_ptr(), wt.data_ptr(), k, S, S, 1e-5, 1, values, cls.data_ptr(), None,
                                               None, counts.data_ptr(), stream))
        parts = [counts.view(torch.uint8), cls.view(-1)]
        if with_sieve:
            _, st = PP.sieve(cls, args.min_pixels, 4, out=cls)
            parts.append(st.view(torch.uint8))
        packed = torch.cat(parts).cpu().numpy()
        write_strip_tiff(path, packed[8 * k:8 * k + S * S].reshape(S, S))
        return packed

    with torch.no_grad():
        out["finalize"] = _wall(lambda: finalize(False), args.repeats, args.warmup)
        out["finalize_sieve"] = _wall(lambda: finalize(True), args.repeats, args.warmup)
        out["finalize_again"] = _wall(lambda: finalize(False), args.repeats, args.warmup)
    os.remove(path)
    os.rmdir(tmp)
    base = out["finalize"]["median_ms"]
    out["sieve_added_ms"] = round(out["finalize_sieve"]["median_ms"] - base, 4)
    out["sieve_added_fraction"] = round(out["sieve_added_ms"] / base, 3) if base > 0 else None
    out["finalize_spread_ms"] = round(max(out[n]["max_ms"] - out[n]["min_ms"] for n in ("finalize", "finalize_again")), 4)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
