"""Cost of vector output on one GPU: the crack edges of a class map and their rings (floodplanet_code_amd/vectorize.py).

A --size x --size uint8 map (1024: the label rasters' size), two inputs:
  sieved    smooth blobs with speckle, sieved at --min_pixels: what a written class map looks like -- few, long rings
  random    every pixel 255 with probability 0.5: about two edges per pixel in many short rings and a few very long ones
and per input, selecting 255, connectivity 4:
  offsets     fu_map_edge_offsets   (count + block scan, scan of the block totals, add: three launches)
  rings       fu_map_edge_rings     (emit, ceil(log2 n) rounds of min-doubling, as many of Wyllie ranking)
  components  fu_map_components     (for scale: the labelling the rings take their component from)
as device time between two events: --inner back-to-back calls, divided by --inner; median of --repeats after --warmup untimed
ones, min / max beside it.  "phases" splits the two calls by kernel -- count_scan (the three launches of offsets), emit,
ring (k_ring_round), rank (k_rank_init, k_rank_round, k_rank_final) -- from one run of each call under torch.profiler,
which sees the kernels by name; null when the profiler reports no kernels (--no-profiler: not asked, for a run under
`rocprofv3 --kernel-trace --stats`, whose statistics give the same split).  "bytes" is what each phase must move, from
the kernels' loads and stores (neighbour reads that hit the cache not counted), and "host" the wall time of the numpy
statements edge_rings_host (which includes label_components_host) and rings_to_polygons on the same map.
The first configuration is timed again at the end: its spread is the noise a difference has to exceed.

    python tools/vector_bench.py [--size 1024]
Prints one JSON line.  Run it on an otherwise idle GPU."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from floodplanet_code_amd import _lib  # noqa: E402
from floodplanet_code_amd import postprocess as PP  # noqa: E402
from floodplanet_code_amd import vectorize as V  # noqa: E402
from tools.sieve_bench import _timed, speckled_map  # noqa: E402

PHASES = {"k_edge_count_scan": "count_scan", "k_scan_totals": "count_scan", "k_scan_add": "count_scan", "k_edge_emit": "emit",
          "k_ring_round": "ring", "k_rank_init": "rank", "k_rank_round": "rank", "k_rank_final": "rank"}


def phase_bytes(n_pix: int, n: int) -> dict:
    """Bytes each phase loads and stores for n_pix pixels and n edges (int32 arrays, a byte per pixel of the map)."""
    rounds = V._rounds(n)
    return {"count_scan": n_pix * (1 + 4) + n_pix * 8,                       # map in, offsets out; offsets in and out
            "emit": n_pix * (1 + 4 + 4) + n * (4 + 4 * 4),                    # map, labels, offsets; a gathered offset, 4 stores
            "ring": n * (16 + 24 * (rounds - 1)),                            # a round: next and ring, own and gathered, 2 stores
            "rank": n * (20 + 24 * rounds + 16),
            "rounds": rounds}


def profiled_phases(calls) -> dict:
    """Device ms per phase of one run of every call in `calls`, from the kernels' names; None without kernel records."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for call in calls:
            call()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        for kernel, phase in PHASES.items():
            if kernel in ev.key:
                us = getattr(ev, "device_time_total", None)
                us = getattr(ev, "cuda_time_total", 0.0) if us is None else us
                out[phase] = out.get(phase, 0.0) + us / 1e3
    return {k: round(v, 5) for k, v in out.items()} if out else None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--min_pixels", type=int, default=25)
    ap.add_argument("--speckle", type=float, default=0.03)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-profiler", dest="profiler", action="store_false")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    lib = _lib.load()
    S = args.size
    stream = torch.cuda.current_stream(dev).cuda_stream
    select_host = V.select_flags([255])
    select = V._select_bytes(select_host)

    blobs = torch.from_numpy(speckled_map(S, args.speckle) * np.uint8(255)).to(dev)
    inputs = {"sieved": PP.sieve(blobs, args.min_pixels, 4)[0].cpu().numpy(),
              "random": ((np.random.default_rng(1).random((S, S)) < 0.5) * 255).astype(np.uint8)}
    labels = torch.empty(S, S, dtype=torch.int32, device=dev)
    offsets = torch.empty(S * S + 1, dtype=torch.int32, device=dev)
    ebytes = int(lib.fu_map_edges_workspace_bytes(S, S))
    ews = torch.empty(ebytes, dtype=torch.uint8, device=dev)

    out = {"size": S, "min_pixels": args.min_pixels, "speckle": args.speckle, "device": torch.cuda.get_device_name(dev),
           "inner": args.inner, "repeats": args.repeats, "select": [255], "connectivity": 4}
    a = (args.inner, args.repeats, args.warmup)
    first = None
    for name, m in inputs.items():
        md = torch.from_numpy(m).to(dev)

        def components(md=md):
            _lib.check(lib.fu_map_components(md.data_ptr(), S, S, 4, labels.data_ptr(), stream))

        def edge_offsets(md=md):
            _lib.check(lib.fu_map_edge_offsets(md.data_ptr(), S, S, select, offsets.data_ptr(), ews.data_ptr(), ebytes, stream))

        components()
        edge_offsets()
        n = int(offsets[-1].item())
        arrays = {k: torch.empty(max(n, 1), dtype=torch.int32, device=dev) for k in V.ARRAYS}
        rbytes = int(lib.fu_map_rings_workspace_bytes(max(n, 1)))
        rws = torch.empty(rbytes, dtype=torch.uint8, device=dev)

        def edge_rings(md=md, n=n, arrays=arrays, rws=rws, rbytes=rbytes):
            _lib.check(lib.fu_map_edge_rings(md.data_ptr(), labels.data_ptr(), S, S, select, 4, offsets.data_ptr(), n,
                                             *(arrays[k].data_ptr() for k in V.ARRAYS), rws.data_ptr(), rbytes, stream))

        entry = {"edges": n, "water_share": round(float((m == 255).mean()), 4), "workspace_bytes": ebytes + rbytes,
                 "read_bytes": 20 * n, "components": _timed(components, *a), "offsets": _timed(edge_offsets, *a),
                 "rings": _timed(edge_rings, *a), "bytes": phase_bytes(S * S, n),
                 "phases": profiled_phases([edge_offsets, edge_rings]) if args.profiler else None}
        if first is None:
            first = (name, edge_offsets)
        t0 = time.perf_counter()
        host = V.edge_rings_host(m, select_host, 4)
        t1 = time.perf_counter()
        polygons = V.rings_to_polygons(host, m.shape, m)
        t2 = time.perf_counter()
        same = all(np.array_equal(arrays[k][:n].cpu().numpy(), host[k]) for k in V.ARRAYS)
        entry["host"] = {"edge_rings_host_ms": round((t1 - t0) * 1e3, 2), "rings_to_polygons_ms": round((t2 - t1) * 1e3, 2),
                         "polygons": len(polygons), "rings": sum(len(p["rings"]) for p in polygons),
                         "device_equals_host": bool(same)}
        out[name] = entry
    out["offsets_again"] = dict(_timed(first[1], *a), input=first[0])
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
