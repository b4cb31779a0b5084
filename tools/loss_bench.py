"""Time per call of the fused cross-entropy entry points on one GPU, training mode (loss + stored logits gradient), at the
bench's loss shape: 16 tiles of 256 x 256, 3 classes, ignore_index 0.  Device events around every call, median:

  ce            fu_loss_ce            (k_ce_loss<3, false, false> + k_ce_finalize<false> + k_ce_grad<3, false, false>): the reference's
                loss, the default path;
  ce_weighted   fu_loss_ce_weighted   (k_ce_loss<3, true, false> + k_ce_finalize<true> + k_ce_grad<3, true, false>) with class weights and
                label smoothing 0.1;
  ce_focal      fu_loss_ce_focal      (k_ce_loss<3, true, true> + k_ce_finalize<true> + k_ce_grad<3, true, true>) with the
                same class weights and gamma = 2, same shape, same run;
  ce_region     fu_loss_ce_region     (the plain CE's three kernels + k_region_sums<3> + k_region_finalize<3> +
                k_region_grad_add<3>): plain cross entropy + soft Dice (weight 1, alpha = beta = 0.5, s = 1), same shape,
                same run;
  label_counts  fu_label_class_counts on 64 whole label rasters of 1024 x 1024 (64 MiB of uint8), one launch.

    python tools/loss_bench.py [--launches 200] [--warmup 20] [--parent_ce_us X]
    python tools/loss_bench.py --ce_only          # uses nothing newer than fu_loss_ce: runs on the parent commit too

--parent_ce_us: `ce_us` of this tool's --ce_only run on the parent commit's build, same box; both per-call numbers are then
stated against it (`ce_vs_parent`, `ce_weighted_vs_parent`).  Nothing is gated on the ratios or on `ce_focal_us`: the weighted
and focal losses and the region term are capabilities; the three CE forms are instantiations of one kernel family, the
region term is two more passes over logits and target behind them (fu_loss.hip).  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from floodplanet_code_amd.unet import HipUNet  # noqa: E402

B, H, W, N_CLASSES, IGNORE = 16, 256, 256, 3, 0


def _median_us(fn, launches, warmup):
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
    return round(1e3 * statistics.median(times), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ce_only", action="store_true")
    ap.add_argument("--parent_ce_us", type=float, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    net = HipUNet(4, N_CLASSES, base_channels=8).to(dev).train()
    x = torch.rand(B, 4, H, W, device=dev, generator=g)
    target = torch.randint(0, N_CLASSES, (B, H, W), device=dev, generator=g)
    net._forward_raw(x, True, want_logits=False)           # the logits the loss calls read stay resident
    res = {"box": torch.cuda.get_device_name(dev), "shape": [B, N_CLASSES, H, W], "launches": args.launches,
           "ce_us": _median_us(lambda: net._loss_raw(target, IGNORE, dev), args.launches, args.warmup)}
    if not args.ce_only:
        from floodplanet_code_amd.datasets.class_weights import label_class_counts
        w = torch.tensor([0.0, 0.6, 2.4])
        net._class_weight_dev(w, dev)                      # (validated and uploaded once, outside the timed calls)
        res["ce_weighted_us"] = _median_us(lambda: net._loss_raw(target, IGNORE, dev, class_weight=w, label_smoothing=0.1),
                                           args.launches, args.warmup)
        res["ce_focal_us"] = _median_us(lambda: net._loss_raw(target, IGNORE, dev, class_weight=w, focal_gamma=2.0),
                                        args.launches, args.warmup)
        res["ce_region_us"] = _median_us(lambda: net._loss_raw(target, IGNORE, dev, region_weight=1.0), args.launches,
                                         args.warmup)
        labels = [torch.randint(0, 3, (1024, 1024), device=dev, generator=g, dtype=torch.uint8) for _ in range(64)]
        entries = [(lab, (0, 0, 1024, 1024)) for lab in labels]
        counts = torch.zeros(N_CLASSES, dtype=torch.int64, device=dev)
        n = max(args.launches // 4, 10)
        res["label_counts_us"] = _median_us(lambda: label_class_counts(net._ctx, entries, IGNORE, N_CLASSES, counts), n, 3)
        res["label_counts_GBps"] = round(64 * 1024 * 1024 / (res["label_counts_us"] * 1e-6) / 1e9, 1)
        assert int(counts.sum()) == (n + 3) * 64 * 1024 * 1024
        if args.parent_ce_us:
            res["parent_ce_us"] = args.parent_ce_us
            res["ce_vs_parent"] = round(res["ce_us"] / args.parent_ce_us, 3)
            res["ce_weighted_vs_parent"] = round(res["ce_weighted_us"] / args.parent_ce_us, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
