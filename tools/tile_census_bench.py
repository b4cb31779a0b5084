"""The tile census of content-aware sampling (datasets/sampling.py), two parts in one JSON object:

  census   time per CALL of fu_label_box_counts on a table shaped like real training -- the synthetic Sentinel-1 tree's
           label rasters at 1024 x 1024 (datasets.synthetic.make_s1_tree), every 300 x 300 box of the stride-150 grid --
           against the yardstick fu_label_class_counts on the same table (it reads the same bytes and exists at the parent
           commit).  Both through the C ABI with the table made beforehand: device events around enough back-to-back calls to
           pass --min_ms, warm-up excluded, samples interleaved A/B/A/B, median and all --samples.  A call is host validation,
           the table's host-to-device copy and one launch -- NOT kernel time.  `floor_pct` is the spread of the yardstick's
           own samples, (max - min) / median; the per-box call is held to the yardstick's median plus that floor
           (`within_floor`), reported and not gated: the census runs once per epoch, or once per run.  Needs an MI355X;
  savings  steps per epoch that tile_sampling "labelled" saves on the labels bundled under tests/golden/rasters, for
           ignore_index 0 and 2: a host computation with label_box_counts_host (--crop / --stride / --batch), no GPU.

    python tools/tile_census_bench.py [--parts census,savings] [--samples 5] [--images_per_region 8]"""
from __future__ import annotations

import argparse
import glob
import gzip
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from floodplanet_code_amd import _lib  # noqa: E402
from floodplanet_code_amd.datasets import FloodplanetTiles, generate_image_slice_object  # noqa: E402
from floodplanet_code_amd.datasets.class_weights import dataset_label_boxes  # noqa: E402
from floodplanet_code_amd.datasets.sampling import label_box_counts_host, tile_stats  # noqa: E402


def _timed(fn, min_ms):
    def sample():
        reps = 16
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= min_ms:
                return ms * 1e3 / reps                   # us per call
            reps *= 4
    return sample


def census_part(args):
    from floodplanet_code_amd.datasets.synthetic import make_s1_tree
    from floodplanet_code_amd.unet import HipUNet
    dev = torch.device("cuda:0")
    lib = _lib.load()
    with tempfile.TemporaryDirectory(prefix="fu_census_") as root:
        n_img = make_s1_tree(root, images_per_region=args.images_per_region, label_size=1024, s1_size=360)
        ds = FloodplanetTiles(root, "train", generate_image_slice_object(300, 300, 150), eval_region=["RegC"], sensor="S1",
                              ignore_index=0)
        host = dataset_label_boxes(ds)
    rasters = {}
    entries = [(rasters.setdefault(id(lab), torch.from_numpy(lab).to(dev)), box) for lab, box in host]
    n = len(entries)
    net = HipUNet(2, 3, base_channels=8).to(dev).eval()
    ctx = net._get_ctx(dev, 1, 32, 32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    table = (_lib.FuSceneTrainEntry * n)(*[
        _lib.FuSceneTrainEntry(None, lab.data_ptr(), lab.shape[0], lab.shape[1], *box, 0, 0.0) for lab, box in entries])
    per_box = torch.empty(n, 3, dtype=torch.int64, device=dev)
    total = torch.zeros(3, dtype=torch.int64, device=dev)

    def box_counts():
        _lib.check(lib.fu_label_box_counts(ctx, n, table, per_box.data_ptr(), stream))

    def class_counts():
        _lib.check(lib.fu_label_class_counts(ctx, n, table, 0, 3, total.data_ptr(), stream))

    for fn in (box_counts, class_counts):
        for _ in range(5):
            fn()
    torch.cuda.synchronize(dev)
    want = label_box_counts_host(host)
    assert np.array_equal(per_box.cpu().numpy(), want), "fu_label_box_counts differs from the host statement"
    arms = {"box_counts": _timed(box_counts, args.min_ms), "class_counts": _timed(class_counts, args.min_ms)}
    got = {k: [] for k in arms}
    for _ in range(args.samples):
        for k, fn in arms.items():
            got[k].append(fn())
    b, c = statistics.median(got["box_counts"]), statistics.median(got["class_counts"])
    floor = (max(got["class_counts"]) - min(got["class_counts"])) / c
    px = int(want.sum())
    return {"box": torch.cuda.get_device_name(dev), "date": time.strftime("%Y-%m-%d"), "samples": args.samples,
            "table": f"{n} boxes of up to 300 x 300 at stride 150 over {len(rasters)} of {n_img} label rasters of 1024 x 1024",
            "box_MB": round(px / 1e6, 2), "box_counts_call_us": round(b, 2), "class_counts_call_us": round(c, 2),
            "box_over_class": round(b / c, 3), "floor_pct": round(100 * floor, 2), "within_floor": bool(b <= c * (1 + floor)),
            "box_counts_call_GBps": round(px / b / 1e3, 1), "class_counts_call_GBps": round(px / c / 1e3, 1),
            "box_counts_samples_us": [round(v, 2) for v in got["box_counts"]],
            "class_counts_samples_us": [round(v, 2) for v in got["class_counts"]]}


def savings_part(args):
    from floodplanet_code_amd.datasets import read_tiff
    from floodplanet_code_amd.datasets.tiles import get_crop_slices
    out = []
    pattern = os.path.join(ROOT, "tests", "golden", "rasters", "**", "labels", "*.tif.gz")
    for gz in sorted(glob.glob(pattern, recursive=True)):
        with tempfile.TemporaryDirectory(prefix="fu_label_") as d:
            path = os.path.join(d, os.path.basename(gz)[:-3])
            with gzip.open(gz, "rb") as src, open(path, "wb") as dst:
                dst.write(src.read())
            label = np.ascontiguousarray(np.asarray(read_tiff(path)))
        if label.dtype != np.uint8:
            label = np.where(label == 2, 2, np.where(label == 0, 0, 1)).astype(np.uint8)
        H, W = label.shape
        boxes = [(h0, w0, min(h0 + h, H), min(w0 + w, W)) for h0, w0, h, w in         # the data set's own grid
                 get_crop_slices(H, W, args.crop, args.crop, args.stride, mode="exact")]
        counts = label_box_counts_host([(label, b) for b in boxes])
        row = {"label": os.path.relpath(gz, ROOT), "raster": [H, W], "crop": args.crop, "stride": args.stride,
               "batch": args.batch, "tiles": len(boxes), "pixels_other_water_nodata": counts.sum(0).tolist()}
        for ii in (0, 2):
            trainable, water = tile_stats(counts, ii, 3)
            kept = int((trainable >= 1).sum())
            steps_all, steps_kept = -(-len(boxes) // args.batch), -(-kept // args.batch)
            row[f"ignore_index_{ii}"] = {"kept": kept, "dropped": len(boxes) - kept, "water_tiles": int((water >= 1).sum()),
                                         "steps_all": steps_all, "steps_labelled": steps_kept,
                                         "steps_saved": steps_all - steps_kept}
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="census,savings")
    ap.add_argument("--samples", type=int, default=5, help="samples per arm (interleaved; at least 3)")
    ap.add_argument("--min_ms", type=float, default=50.0, help="least event-timed window of a sample")
    ap.add_argument("--images_per_region", type=int, default=8)
    ap.add_argument("--crop", type=int, default=300)
    ap.add_argument("--stride", type=int, default=150)
    ap.add_argument("--batch", type=int, default=10)
    args = ap.parse_args()
    if args.samples < 3:
        raise SystemExit("--samples must be at least 3")
    parts = args.parts.split(",")
    res = {}
    if "census" in parts:
        if not torch.cuda.is_available():
            raise SystemExit("the census part needs an MI355X (--parts savings runs without one)")
        res["census"] = census_part(args)
    if "savings" in parts:
        res["savings"] = savings_part(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
