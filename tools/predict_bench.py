"""Crops/s of scene prediction on one GPU, three ways:

  reference_loop  the reference's predict.py shape (predict.py:207-260): batch 1, NCHW logits, fu_stitch_add per crop and
                  a host read of the crop's F1 / IoU per crop;
  batched_gpu     the batched pipeline on resident synthetic tiles (the GPU stage of predict() alone): eval forward,
                  fu_eval_confusion, per-crop metrics read once per batch, one fu_stitch_add_batch per batch; with
                  --tta, one forward of T*B view samples (fu_forward_views), fu_merge_views (probabilities and counts)
                  and one fu_stitch_add_batch_probs per batch instead;
  predict_e2e     floodplanet_code_amd.predict.predict() end to end on datasets.synthetic.make_s1_tree, next to the host
                  loader alone (TileLoader with device assembly / resampling and nothing else), which names the cap.

    python tools/predict_bench.py [--batch 16] [--precision bf16] [--crop 300] [--stride 150] [--tta {none,hflip,flips,d4}]
Prints one JSON line.  Run under `rocprofv3 --kernel-trace --stats -- python tools/predict_bench.py` to count the
launches: one k_stitch_add_batch and one k_eval_confusion per batch, no k_ce_loss (with --tta: one
k_gather_views_nchw_to_nhwc per encoder, one k_merge_views and one k_stitch_add_batch_probs per batch, no
k_eval_confusion)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from floodplanet_code_amd.metrics import SegmentationMetrics  # noqa: E402
from floodplanet_code_amd.stitch import GpuImageStitcher  # noqa: E402
from floodplanet_code_amd.unet import HipUNet  # noqa: E402


def _grid(n_side, S, stride):
    H = W = stride * (n_side - 1) + S
    return H, W, [(i * stride, j * stride, i * stride + S, j * stride + S) for i in range(n_side) for j in range(n_side)]


def reference_loop(net, x, target, boxes, H, W, dev):
    met = SegmentationMetrics(3, None, "test_")
    st = GpuImageStitcher(net, dev)
    vals = []
    for i, box in enumerate(boxes):
        logits = net._forward_raw(x[i:i + 1], False, want_logits=True)
        pred = logits.argmax(dim=1)
        r = met(pred, target[i:i + 1])
        vals.append((r["test_MulticlassF1Score"].item(), r["test_MulticlassJaccardIndex"].item()))
        st.add_image(0, "img", box, H, W)
    return st.combine("img")


def batched_gpu(net, x, target, boxes, H, W, dev, B, codes=None):
    met = SegmentationMetrics(3, None, "test_")
    st = GpuImageStitcher(net, dev)
    vals = []
    for b0 in range(0, len(boxes), B):
        n = min(B, len(boxes) - b0)
        probs = None
        if codes is None:
            net._forward_raw(x[b0:b0 + n], False, want_logits=False)
            counts = net.eval_confusion(target[b0:b0 + n], -100)
        else:
            net.forward_views(x[b0:b0 + n], codes)
            probs, counts = net.merge_views(target[b0:b0 + n], -100)
        met.accumulate_counts(counts)
        r = met.reduce_batch(counts)
        vals += torch.stack([r["test_MulticlassF1Score"], r["test_MulticlassJaccardIndex"]]).cpu().tolist()
        st.add_images(range(n), ["img"] * n, boxes[b0:b0 + n], [H] * n, [W] * n, probs=probs)
    return st.combine("img")


def _rate(fn, n_crops, dev, reps):
    fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(dev)
    return n_crops * reps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--crop", type=int, default=300)
    ap.add_argument("--stride", type=int, default=150)
    ap.add_argument("--side", type=int, default=6, help="crops per side of the synthetic raster (resident cases)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--images_per_region", type=int, default=2)
    ap.add_argument("--label_size", type=int, default=1024)
    ap.add_argument("--n_workers", type=int, default=0)
    ap.add_argument("--skip_e2e", action="store_true")
    ap.add_argument("--skip_reference", action="store_true", help="skip the reference-shaped loop")
    ap.add_argument("--tta", default="none", choices=["none", "hflip", "flips", "d4"],
                    help="test-time augmentation of the batched GPU stage and predict() (default: none)")
    args = ap.parse_args()
    tta = None if args.tta == "none" else args.tta
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    S = args.crop
    H, W, boxes = _grid(args.side, S, args.stride)
    n = len(boxes)
    net = HipUNet(2, 3, base_channels=args.base, precision=args.precision).to(dev).eval()
    x = torch.rand(n, 2, S, S, device=dev)
    target = torch.randint(0, 3, (n, S, S), device=dev)
    res = {"box": torch.cuda.get_device_name(dev), "precision": args.precision, "batch": args.batch, "crop": S,
           "stride": args.stride, "resident_crops": n, "tta": args.tta}
    with torch.no_grad():
        if not args.skip_reference:
            res["reference_loop_crops_per_s"] = round(_rate(lambda: reference_loop(net, x, target, boxes, H, W, dev), n,
                                                            dev, args.reps), 1)
        res["batched_gpu_crops_per_s"] = round(_rate(lambda: batched_gpu(net, x, target, boxes, H, W, dev, args.batch,
                                                                         tta), n, dev, args.reps), 1)
    from floodplanet_code_amd import _lib
    res["context_workspace_gib"] = round(_lib.load().fu_workspace_bytes(net._ctx) / 2**30, 2)   # sized for T * batch samples
    if not args.skip_e2e:
        from floodplanet_code_amd import predict as P
        from floodplanet_code_amd.datasets import FloodplanetTiles, TileLoader, generate_image_slice_object
        from floodplanet_code_amd.datasets.synthetic import make_s1_tree
        from floodplanet_code_amd.models import build_model
        with tempfile.TemporaryDirectory() as tmp:
            root = os.path.join(tmp, "data")
            make_s1_tree(root, images_per_region=args.images_per_region, label_size=args.label_size)
            exp = os.path.join(tmp, "exp")
            os.makedirs(os.path.join(exp, "checkpoints"))
            cfg = dict(crop_height=S, crop_width=S, crop_stride=args.stride, batch_size=args.batch,
                       eval_region=["RegA", "RegB", "RegC"], n_workers=args.n_workers,
                       model=dict(name="ms_model", model_kwargs=dict(optimizer_name="adam", base_channels=args.base,
                                                                     precision=args.precision)))
            model = build_model("ms_model", {"ms_image": 2}, 3, 1e-4, 200, None, 0, base_channels=args.base,
                                precision=args.precision)
            ckpt = os.path.join(exp, "checkpoints", "model-epoch=00-val_MulticlassJaccardIndex=0.0000.ckpt")
            torch.save({"state_dict": model.state_dict(), "hyper_parameters": cfg}, ckpt)
            ds = FloodplanetTiles(root, "test", generate_image_slice_object(S, S, args.stride),
                                  eval_region=["RegA", "RegB", "RegC"], sensor="S1", ignore_index=0, output_metadata=True)
            crops = len(ds)
            t0 = time.perf_counter()
            for batch in TileLoader(ds, args.batch, dev, num_workers=args.n_workers, device_assembly=True,
                                    device_resize=True):
                pass
            torch.cuda.synchronize(dev)
            loader = crops / (time.perf_counter() - t0)
            full_cfg = P.resolve_cfg(exp, ckpt)
            P.predict(full_cfg, exp, ckpt, "floodplanet", n_workers=args.n_workers, data_root=root,
                      batch_size=args.batch, device=str(dev), tta=tta)           # warm-up (context, packing, caches)
            t0 = time.perf_counter()
            P.predict(full_cfg, exp, ckpt, "floodplanet", n_workers=args.n_workers, data_root=root,
                      batch_size=args.batch, device=str(dev), tta=tta)
            torch.cuda.synchronize(dev)
            e2e = crops / (time.perf_counter() - t0)
        res.update({"e2e_crops": crops, "predict_e2e_crops_per_s": round(e2e, 1),
                    "host_loader_alone_crops_per_s": round(loader, 1),
                    "e2e_capped_by": "host loader" if loader < res["batched_gpu_crops_per_s"] else "GPU stage"})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
