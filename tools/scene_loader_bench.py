"""Training from device-resident scenes, measured on one GPU on the synthetic Sentinel-1 tree of `bench.py --path loader`
(datasets.synthetic.make_s1_tree: 2 x 360 x 360 rasters -> 1024 x 1024 labels; 256 x 256 crops, batch 16, hflip / vflip /
rotate).  One JSON object with three parts:

  loaders   tiles/s of SceneTileLoader and of TileLoader(device_assembly, device_resize, 4 workers) over the same data set,
            samples interleaved A/B/A/B after a warm-up epoch each, median of --samples; a sample iterates whole epochs for
            at least --min_seconds and ends in one device synchronise;
  calls     time per batch of a whole fu_scene_train_tiles CALL against the fu_scene_crops + fu_augment calls on the same
            boxes and draws, through the C ABI with tables and buffers made beforehand: device events around enough
            back-to-back calls to pass --min_ms, warm-up excluded, interleaved, median of --samples.  This is the rate at
            which batches come out -- host validation, the table's host-to-device copy and the launches included -- NOT
            kernel time: at 16 x 2 x 256 x 256 the call overhead is a visible share.  Bytes moved (what each side must read
            and write, from the shapes) and the GB/s per call they imply.  The chain is given its un-augmented target batch
            for free (the streaming loader uploads it from the host).  Kernel time proper comes from a run of its own:
            rocprofv3 --kernel-trace --stats -- python tools/scene_loader_bench.py --parts calls;
  training  tiles/s of DataParallelTrainer steps (HipUNet, base 64, --precision) fed by SceneTileLoader against the same
            number of steps on one resident batch (what bench.py's `value` times), interleaved, median of --samples.

    python tools/scene_loader_bench.py [--samples 5] [--images_per_region 24] [--precision bf16]
Differences under 6 % between the arms of one run are within what one binary shows from box to box and run to run."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from floodplanet_code_amd import _lib, augment  # noqa: E402
from floodplanet_code_amd.datasets import (FloodplanetTiles, SceneTileLoader, TileLoader,  # noqa: E402
                                           generate_image_slice_object)
from floodplanet_code_amd.datasets.synthetic import make_s1_tree  # noqa: E402
from floodplanet_code_amd.unet import HipUNet  # noqa: E402


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


def _epochs_rate(loader, dev, min_seconds, consume=None):
    """Whole epochs for at least min_seconds of host time, one synchronise at the end -> tiles/s."""
    n, t0 = 0, time.perf_counter()
    while True:
        for b in loader:
            if consume is not None:
                consume(b)
            n += b["image"].shape[0]
        if time.perf_counter() - t0 >= min_seconds:
            break
    torch.cuda.synchronize(dev)
    return n / (time.perf_counter() - t0)


def _interleaved(arms: dict, samples: int):
    """arms: name -> callable returning one sample; A/B/A/B ..., -> name -> (median, all samples)."""
    got = {k: [] for k in arms}
    for _ in range(samples):
        for k, fn in arms.items():
            got[k].append(fn())
    return {k: (statistics.median(v), v) for k, v in got.items()}


def loaders_part(ds, net, dev, args):
    scene = SceneTileLoader(ds, args.batch, dev, net, shuffle=True, seed=0, drop_last=True, transforms={})
    tile = TileLoader(ds, args.batch, dev, shuffle=True, seed=0, drop_last=True, num_workers=args.workers, transforms={},
                      ignore_index=0, device_assembly=True, device_resize=True)
    t0 = time.perf_counter()
    for _ in scene:                                      # warm-up epoch: includes the one-time decode / upload / resample
        pass
    torch.cuda.synchronize(dev)
    first_epoch_s = time.perf_counter() - t0
    for _ in tile:                                       # warm-up epoch: worker start, page cache, first kernels
        pass
    torch.cuda.synchronize(dev)
    res = _interleaved({"scene": lambda: _epochs_rate(scene, dev, args.min_seconds),
                        "tile": lambda: _epochs_rate(tile, dev, args.min_seconds)}, args.samples)
    s, t = res["scene"][0], res["tile"][0]
    out = {"tiles_per_epoch": len(scene) * args.batch, "scene_first_epoch_s": round(first_epoch_s, 3),
           "scene_resident_MB": round(scene.resident_bytes / 1e6, 1), "tile_workers": args.workers,
           "scene_tiles_per_s": round(s, 1), "tile_tiles_per_s": round(t, 1), "scene_over_tile": round(s / t, 2),
           "scene_samples": [round(v, 1) for v in res["scene"][1]], "tile_samples": [round(v, 1) for v in res["tile"][1]]}
    del tile
    return out, scene


def calls_part(items, net, dev, args, C_, tile_hw, norm_mode):
    """items: [(grid, label, box)] of one batch.  Both sides through the C ABI, tables and buffers made once."""
    lib = _lib.load()
    th, tw = tile_hw
    n = len(items)
    rng = np.random.RandomState(0)
    flags, angles = augment.sample_transforms(n, {}, rng)
    ctx = net._get_ctx(dev, n, th, tw)
    stream = torch.cuda.current_stream(dev).cuda_stream
    train_tab = (_lib.FuSceneTrainEntry * n)(*[
        _lib.FuSceneTrainEntry(g.data_ptr(), l.data_ptr(), g.shape[1], g.shape[2], *box, int(f), float(a))
        for (g, l, box), f, a in zip(items, flags, angles)])
    crop_tab = (_lib.FuSceneCrop * n)(*[_lib.FuSceneCrop(g.data_ptr(), g.shape[1], g.shape[2], *box) for g, _, box in items])
    image = torch.empty(n, C_, th, tw, device=dev)
    image2 = torch.empty_like(image)
    target_in = torch.randint(0, 2, (n, th, tw), device=dev)
    target = torch.empty_like(target_in)
    mean, std = torch.zeros(n, C_, device=dev), torch.ones(n, C_, device=dev)
    f_dev, a_dev = torch.from_numpy(flags).to(dev), torch.from_numpy(angles).to(dev)
    mode = {None: 0, "local": 1}[norm_mode]
    m, s = (mean.data_ptr(), std.data_ptr()) if mode == 1 else (None, None)

    def fused():
        _lib.check(lib.fu_scene_train_tiles(ctx, n, train_tab, C_, th, tw, mode, None, None, 0.0, 0, 0, image.data_ptr(),
                                            target.data_ptr(), m, s, stream))

    def chain():
        _lib.check(lib.fu_scene_crops(ctx, n, crop_tab, C_, th, tw, mode, None, None, 0.0, image2.data_ptr(), m, s, stream))
        _lib.check(lib.fu_augment(image2.data_ptr(), target_in.data_ptr(), image.data_ptr(), target.data_ptr(),
                                  f_dev.data_ptr(), a_dev.data_ptr(), n, C_, th, tw, 0, stream))

    def timed(fn):
        def sample():
            reps, ms = 64, 0.0
            while True:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                if ms >= args.min_ms:
                    return ms * 1e3 / reps               # us per call
                reps *= 4
        return sample
    for fn in (fused, chain):
        for _ in range(10):
            fn()
    torch.cuda.synchronize(dev)
    res = _interleaved({"fused": timed(fused), "chain": timed(chain)}, args.samples)
    box_px = sum((b[2] - b[0]) * (b[3] - b[1]) for _, _, b in items)
    tile_px = n * th * tw
    stats_read = box_px * C_ * 4 * 2 if mode == 1 else 0                 # k_tile_stats reads the boxes twice
    fused_bytes = stats_read + box_px * (C_ * 4 + 1) + tile_px * (C_ * 4 + 8)
    chain_bytes = stats_read + box_px * C_ * 4 + tile_px * C_ * 4 + tile_px * (C_ * 4 + 8) * 2
    fu, ch = res["fused"][0], res["chain"][0]
    return {"shape": [n, C_, th, tw], "norm_mode": norm_mode, "rotated_samples": int((flags & 4).astype(bool).sum()),
            "fused_call_us": round(fu, 2), "chain_call_us": round(ch, 2), "fused_over_chain": round(fu / ch, 3),
            "fused_MB": round(fused_bytes / 1e6, 2), "chain_MB": round(chain_bytes / 1e6, 2),
            "fused_call_GBps": round(fused_bytes / fu / 1e3, 1), "chain_call_GBps": round(chain_bytes / ch / 1e3, 1),
            "fused_call_samples_us": [round(v, 2) for v in res["fused"][1]],
            "chain_call_samples_us": [round(v, 2) for v in res["chain"][1]]}


def training_part(ds, dev, args):
    from floodplanet_code_amd.distributed import DataParallelTrainer
    torch.manual_seed(0)
    net = HipUNet(2, 3, bilinear=True, base_channels=64, precision=args.precision).to(dev).train()
    trainer = DataParallelTrainer(net, lr=1e-4, world_size=1, rank=0, graph=False)
    loader = SceneTileLoader(ds, args.batch, dev, net, shuffle=True, seed=0, drop_last=True, transforms={})
    first = next(iter(loader))
    x, t = first["image"].clone(), first["target"].clone()
    steps = len(loader)
    for _ in range(5):
        trainer.step(x, t, 0)
    torch.cuda.synchronize(dev)

    def fed():
        return _epochs_rate(loader, dev, args.min_seconds, consume=lambda b: trainer.step(b["image"], b["target"], 0))

    def resident():
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(steps):
                trainer.step(x, t, 0)
                n += x.shape[0]
            if time.perf_counter() - t0 >= args.min_seconds:
                break
        torch.cuda.synchronize(dev)
        return n / (time.perf_counter() - t0)
    fed()                                                # warm-up of the fed arm
    res = _interleaved({"loader_fed": fed, "resident_batch": resident}, args.samples)
    a, b = res["loader_fed"][0], res["resident_batch"][0]
    return {"model": f"HipUNet(2, 3, base_channels=64, {args.precision}), batch {args.batch}, eager launches",
            "steps_per_epoch": steps, "loader_fed_tiles_per_s": round(a, 1), "resident_batch_tiles_per_s": round(b, 1),
            "loader_fed_over_resident": round(a / b, 3), "loader_fed_samples": [round(v, 1) for v in res["loader_fed"][1]],
            "resident_batch_samples": [round(v, 1) for v in res["resident_batch"][1]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5, help="samples per arm (interleaved; at least 3)")
    ap.add_argument("--min_seconds", type=float, default=3.0, help="least duration of a loader / training sample")
    ap.add_argument("--min_ms", type=float, default=50.0, help="least event-timed window of a calls sample")
    ap.add_argument("--images_per_region", type=int, default=24)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--parts", default="loaders,calls,training")
    args = ap.parse_args()
    if args.samples < 3:
        raise SystemExit("--samples must be at least 3")
    if not torch.cuda.is_available():
        raise SystemExit("scene_loader_bench needs an MI355X; the device data path has no CPU fallback")
    dev = torch.device("cuda:0")
    parts = args.parts.split(",")
    res = {"box": torch.cuda.get_device_name(dev), "csrc_sha": _csrc_sha(), "date": time.strftime("%Y-%m-%d"),
           "samples": args.samples, "batch": args.batch, "size": args.size}
    with tempfile.TemporaryDirectory(prefix="fu_scene_") as root:
        n_img = make_s1_tree(root, images_per_region=args.images_per_region, label_size=1024, s1_size=360)
        ds = FloodplanetTiles(root, "train", generate_image_slice_object(args.size, args.size, args.size),
                              eval_region=["RegC"], sensor="S1", ignore_index=0)
        res["workload"] = (f"synthetic CSDAP tree: {n_img} Sentinel-1 rasters 2 x 360 x 360 f32 -> labels 1024 x 1024 u8, "
                           f"{len(ds)} training tiles of {args.size} x {args.size}, batch {args.batch}, shuffle, hflip / "
                           "vflip / rotate")
        net = HipUNet(2, 3, base_channels=8).to(dev).eval()        # owns the table's context for the first two parts
        scene = None
        if "loaders" in parts:
            res["loaders"], scene = loaders_part(ds, net, dev, args)
        if "calls" in parts:
            if scene is None:
                scene = SceneTileLoader(ds, args.batch, dev, net, shuffle=True, seed=0, drop_last=True, transforms={})
                next(iter(scene))
            order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(0))[:args.batch].tolist()
            items = [scene._items[i] for i in order]
            res["calls"] = [calls_part(items, net, dev, args, 2, (args.size, args.size), nm) for nm in (None, "local")]
            # the flagship's 8 channels: synthetic scenes of the same size
            g = torch.Generator(device=dev).manual_seed(0)
            big = [torch.rand(8, 1024, 1024, device=dev, generator=g) for _ in range(4)]
            items8 = [(big[k % 4], items[k][1], items[k][2]) for k in range(len(items))]
            res["calls"].append(calls_part(items8, net, dev, args, 8, (args.size, args.size), None))
        del scene
        if "training" in parts:
            res["training"] = training_part(ds, dev, args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
