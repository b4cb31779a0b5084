"""Batched scene prediction: restatement of st_water_seg/predict.py:20-400 for machines without omegaconf, torchmetrics,
tifffile, PIL, scipy or einops.

    python -m floodplanet_code_amd.predict <exp>/checkpoints/<name>.ckpt --data_root <dir with CSDAP_complete/> [...]

Same outputs as the reference, under the same directory (`pred_dir`, predict.py:186-196): metrics.json, the four ranked
lists (predict.py:73-126, byte for byte for the same values) and, with predict_images, per image
image_predictions/<region>/<image>/{pred_class.tif, pred_softmax.png, cm.png}.  What runs differently:
  * crops go through the model `batch_size` at a time (TileLoader with device assembly and device resampling), not one by
    one; the logits stay in the HIP context in NHWC and are never copied to NCHW or to the host;
  * per-crop metrics come from one fu_eval_confusion per batch ([B, k, k] counts of the resident logits) and
    SegmentationMetrics' formulas, read back once per batch (the reference syncs twice per crop);
  * stitching is one fu_stitch_add_batch launch per batch (bit-identical to per-crop fu_stitch_add) and one
    fu_stitch_finalize per image;
  * each crop's counts are added to the running metric once: predict.py:239-240 adds them twice (metric forward plus
    update), which doubles every count and leaves all micro ratios -- the only thing metrics.json holds -- unchanged;
  * the model is built with model_kwargs also on load_from_checkpoint (base_channels / precision: the reference has one
    width); as in the reference, load_from_checkpoint gets no ignore_index, so the test metrics ignore no class;
  * pred_class.tif is float32, bands first (planar), written by datasets.synthetic.write_strip_tiff (the reference writes
    float16 [H, W, 3] through tifffile; the values are the same 0 / 1); PNGs come from a stdlib zlib writer.
Extension: --tta {hflip,flips,d4} (test-time augmentation, floodplanet_code_amd.tta) averages each crop's softmax over
flips / 90-degree rotations: per batch one forward of T*B view samples (HipUNet.forward_views), one fu_merge_views for
the averaged probabilities and their confusion counts, one fu_stitch_add_batch_probs; metrics.json gains a "tta" key.
Extension: --weights {auto,raw,ema} chooses between the checkpoint's state_dict and the weight EMA a run with --ema_decay
stored beside it as ema_state_dict (auto: the EMA when there is one); metrics.json records the choice under "weights"
whenever the EMA was served or a choice was given (absent: the state_dict, as always).
Extension: --calibrate [CLS] (default 1, water) accumulates the histogram of class probability against target class over
the crops (HipUNet.prob_histogram: one more launch per batch beside the confusion counts, each crop once; with --tta on
the merged probabilities) and writes calibration.json beside metrics.json: the one-versus-rest threshold sweep of CLS,
its best-F1 / best-IoU thresholds, average precision and the expected calibration error (calibration.report).
infer --calibration applies the threshold.  Without the flag nothing new is launched or written.
Out of scope: rgb.png, gt.png and rgb_cm.gif (to_RGB and a GIF encoder), infer.py, multi-GPU prediction, datasets other
than floodplanet.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import struct
import zlib
from collections import defaultdict
from typing import Dict, List, Optional

import numpy as np
import torch

from .infer_options import WEIGHT_CHOICES, check_blend, check_weights
from .tta import VIEW_SETS, recorded, view_codes
# conf/config.yaml + conf/dataset/floodplanet.yaml + conf/model/ef_model.yaml of the reference: what a key missing from
# the experiment's config takes
CONFIG_DEFAULTS = dict(
    eval_region="Nepal", train_split_pct=0.8, crop_height=300, crop_width=300, crop_stride=150, n_epochs=11, lr=1e-4,
    optimizer="adam", batch_size=10, n_workers=4, save_topk_models=3, ignore_index=0, seed_num=0, profiler=None,
    limit_train_batches=None, limit_val_batches=None, log_image_iter=200, norm_mode=None,
    dataset=dict(name="floodplanet", channels="ALL", sensor="S1", dataset_kwargs=None),
    model=dict(name="ef_model", model_kwargs=dict(optimizer_name="adam")))


# ---------------------------------------------------------------------------------------------------------- config
def _merge(base: dict, over: dict) -> dict:
    out = copy.deepcopy(base)
    for k, v in (over or {}).items():
        out[k] = _merge(out[k], v) if isinstance(out.get(k), dict) and isinstance(v, dict) else copy.deepcopy(v)
    return out


def resolve_cfg(experiment_dir: str, checkpoint_path: str) -> dict:
    """<exp>/.hydra/config.yaml, else <exp>/hydra/config.yaml (predict.py:45-49) when PyYAML imports; otherwise the
    checkpoint's hyper_parameters (what fit_model writes).  Missing keys take CONFIG_DEFAULTS."""
    cfg = None
    try:
        import yaml  # type: ignore
    except ImportError:
        yaml = None
    if yaml is not None:
        for sub in (".hydra", "hydra"):
            path = os.path.join(experiment_dir, sub, "config.yaml")
            if os.path.exists(path):
                with open(path) as fh:
                    cfg = yaml.safe_load(fh)
                break
    if cfg is None:
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        cfg = ckpt.get("hyper_parameters") if isinstance(ckpt, dict) else None
        if cfg is None:
            raise ValueError(f"no config.yaml under {experiment_dir} (or PyYAML missing) and no hyper_parameters in "
                             f"{checkpoint_path}")
    return _merge(CONFIG_DEFAULTS, dict(cfg))


def checkpoint_weights(ckpt: dict, which: str = "auto", path: Optional[str] = None):
    """Which weights of a checkpoint to serve -> (state_dict, chosen) with chosen 'raw' or 'ema'.  'raw': the checkpoint's
    state_dict (a bare state dict counts as one); 'ema': its ema_state_dict, an error naming the file when it has none;
    'auto': 'ema' when there is one, else 'raw'.  Host only."""
    check_weights(which)
    ema = ckpt.get("ema_state_dict") if isinstance(ckpt, dict) else None
    if which == "ema" and ema is None:
        raise KeyError(f"checkpoint {path if path is not None else '<dict>'} has no ema_state_dict (it was trained without "
                       f"--ema_decay): use --weights raw or auto")
    if ema is not None and which in ("auto", "ema"):
        return ema, "ema"
    return (ckpt["state_dict"] if "state_dict" in ckpt else ckpt), "raw"


def load_checkpoint_model(model, checkpoint_path: str, weights: str, **ctor):
    """A new model of `model`'s class holding the chosen weights of the checkpoint -> (model, chosen): what
    load_from_checkpoint(checkpoint_path, **ctor) builds -- cls(**ctor), then load_state_dict -- with the file read once and
    checkpoint_weights choosing the dict.  The served model keeps no EMA of its own: ema_decay / ema_warmup are training
    arguments, and the callers keep them out of ctor."""
    ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    sd, chosen = checkpoint_weights(ckpt, weights, checkpoint_path)
    model = type(model)(**ctor)
    model.load_state_dict(sd)
    return model, chosen


def load_eval_model(cfg: dict, checkpoint_path: str, weights: str, n_channels, n_classes: int, device):
    """The model the config describes, holding the chosen weights of the checkpoint, in eval mode on the device ->
    (model, chosen).  build_model only names the class: the served model is the one load_checkpoint_model builds, which
    as load_from_checkpoint gets no ignore_index."""
    from .models import build_model
    model_kwargs = {k: v for k, v in (cfg["model"].get("model_kwargs") or {}).items()
                    if k not in ("ema_decay", "ema_warmup")}
    model = build_model(cfg["model"]["name"], n_channels, n_classes, cfg["lr"], log_image_iter=cfg["log_image_iter"],
                        to_rgb_fcn=None, ignore_index=cfg["ignore_index"], **model_kwargs)
    model, chosen = load_checkpoint_model(model, checkpoint_path, weights, in_channels=n_channels, n_classes=n_classes,
                                          lr=cfg["lr"], **model_kwargs)
    model._set_model_to_eval()
    return model.to(device), chosen


def eval_forward(net, sources, codes=None, target=None, ignore_index: int = -100, want_probs: bool = False):
    """One eval forward of a batch on the device -> (probs | None, counts | None).  codes None: the plain forward, whose
    logits stay resident in the context (probs is None), plus eval_confusion when there is a target.  With view codes:
    one forward of all views and one merge_views launch for the averaged probabilities (when wanted) and the counts."""
    if codes is None:
        net._forward_raw(sources, False, want_logits=False)
        return None, (net.eval_confusion(target, ignore_index) if target is not None else None)
    net.forward_views(sources, codes)
    return net.merge_views(target, ignore_index, want_probs=want_probs)


def prediction_dir(cfg: dict, experiment_dir: str, checkpoint_path: str, eval_dataset_name: str) -> str:
    """pred_dir of predict.py:188-195, including its quirk that the checkpoint name keeps only the text before the first
    '.' of the file name."""
    chkpt_name = checkpoint_path.split("/")[-1].split(".")[:-1][0]
    region = cfg.get("eval_region")
    if region is None:
        return os.path.join(experiment_dir, "predictions_PS_alldata_4", eval_dataset_name,
                            f"split_pct_{cfg['train_split_pct']}", chkpt_name)
    if isinstance(region, (list, tuple)):
        region = "_".join(region)
    return os.path.join(experiment_dir, "predictions_PS_alldata_4", eval_dataset_name, region, chkpt_name)


# ---------------------------------------------------------------------------------------------------------- outputs
def _ranked_lines(stats: Dict[str, List[float]], kind: str, metric_name: str, names) -> str:
    means = [np.mean(v) for v in stats.values()]
    keys = [k for _, k in sorted(zip(means, list(stats.keys())))][::-1]      # ties: the larger key first
    values = sorted(means)[::-1]
    lines = [f"Ranked {kind} {metric_name} \n", "---------------------- \n"]
    lines += [f"{name}: {v * 100}% \n" for name, v in zip(names(keys), values)]
    return "".join(lines)


def ranked_images_text(image_stats: Dict[str, List[float]], metric_name: str) -> str:
    """The text save_image_stats (predict.py:73-106) writes: images by the mean of their crops' values, best first,
    named by the file name minus its last four characters."""
    return _ranked_lines(image_stats, "image", metric_name, lambda ks: [os.path.split(p)[1][:-4] for p in ks])


def ranked_regions_text(region_stats: Dict[str, List[float]], metric_name: str) -> str:
    """The text save_region_stats (predict.py:109-126) writes."""
    return _ranked_lines(region_stats, "region", metric_name, lambda ks: list(ks))


def write_ranked_files(pred_dir: str, image_f1, image_iou, region_f1, region_iou) -> None:
    """predict.py:395-400: the image lists always, the region lists when any region was seen."""
    files = [("ranked_images_F1-score.txt", ranked_images_text(image_f1, "F1-score")),
             ("ranked_images_mIoU.txt", ranked_images_text(image_iou, "mIoU"))]
    if len(region_iou) > 0:
        files += [("ranked_regions_F1-Score.txt", ranked_regions_text(region_f1, "F1-Score")),
                  ("ranked_regions_iou.txt", ranked_regions_text(region_iou, "iou"))]
    for name, text in files:
        with open(os.path.join(pred_dir, name), "w") as fh:
            fh.write(text)


def write_png(path: str, image: np.ndarray) -> None:
    """8-bit PNG (gray [H, W], RGB [H, W, 3] or RGBA [H, W, 4]) with zlib only: filter 0 on every row, one IDAT."""
    a = np.ascontiguousarray(image, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4):
        raise ValueError(f"write_png: expected [H, W], [H, W, 3] or [H, W, 4], got {image.shape}")
    h, w, ch = a.shape
    color = {1: 0, 3: 2, 4: 6}[ch]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * ch)], axis=1).tobytes()

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color, 0, 0, 0))
                 + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def softmax_png(prob: np.ndarray) -> np.ndarray:
    """The PIL branch of ImageStitcher_v2._save_image (utils_image.py:521-543): x255 when every value is below 1, then
    uint8."""
    img = prob * 255 if prob.max() < 1 else prob
    return img.astype(np.uint8)


def conf_matrix_image(pred: np.ndarray, target: np.ndarray) -> np.ndarray:
    """create_conf_matrix_pred_image (tools.py:118-135): TP white, FP teal, FN red, the rest black."""
    out = np.zeros(pred.shape + (3,), dtype=np.uint8)
    out[(pred == 1) & (target == 1)] = (255, 255, 255)
    out[(pred == 1) & (target == 0)] = (0, 255, 255)
    out[(pred == 0) & (target == 1)] = (255, 0, 0)
    return out


# ---------------------------------------------------------------------------------------------------------- predict
def predict(cfg, experiment_dir, checkpoint_path, eval_dataset_name, predict_images=False, eval_region=None,
            eval_dataset_split="test", n_workers=0, *, data_root, batch_size=None, device="cuda:0", tta=None,
            weights="auto", blend="uniform", calibrate=None, calibrate_bins=256) -> dict:
    """predict.py:129-400 with batched crops.  Returns {"pred_dir", "metrics", "image_stats_f1", "image_stats_iou",
    "region_stats_f1", "region_stats_iou", "probabilities"} (probabilities: {region/image: [H, W, k] float32} of the
    stitched canvases when predict_images, else {}).  tta: None, a tta.VIEW_SETS name or a list of view codes; with it,
    every crop's prediction (metrics and canvases) is the mean softmax over its views.  T views run batch_size * T
    samples per forward: lower batch_size when that does not fit.  weights: 'auto', 'raw' or 'ema' (checkpoint_weights);
    metrics.json records the choice under "weights" when the EMA was served or weights is not 'auto'.  blend: "uniform",
    "linear" or "hann" (stitch.blend_window) -- how overlapping crops are averaged in the stitched images; the per-crop
    metrics come from the crops and do not depend on it.  metrics.json records a blend other than "uniform".
    calibrate: None, or the class whose threshold sweep goes to <pred_dir>/calibration.json (calibration.report over
    calibrate_bins bins); the result then also holds "best_threshold" and "best_f1"."""
    from .datasets import FloodplanetTiles, TileLoader, generate_image_slice_object
    from .datasets.synthetic import write_strip_tiff
    from .stitch import GpuImageStitcher

    cfg = _merge(CONFIG_DEFAULTS, cfg)
    check_weights(weights)
    check_blend(blend)
    if calibrate is not None:            # checked before any GPU work
        from .calibration import check_bins
        calibrate, calibrate_bins = int(calibrate), check_bins(calibrate_bins)
        if calibrate < 0:
            raise ValueError(f"calibrate: class {calibrate} is negative")
    if eval_dataset_name != "floodplanet":
        raise NotImplementedError(f'prediction supports the "floodplanet" dataset only, not "{eval_dataset_name}"')
    slice_params = generate_image_slice_object(cfg["crop_height"], cfg["crop_width"], cfg["crop_stride"])
    codes = None
    if tta is not None:                  # checked before any GPU work (d4 needs square crops)
        codes = view_codes(tta, cfg["crop_height"], cfg["crop_width"])
    if eval_region:
        cfg["eval_region"] = eval_region
    ds_cfg = cfg["dataset"]
    dataset = FloodplanetTiles(data_root, eval_dataset_split, slice_params, eval_region=copy.copy(cfg["eval_region"]),
                               sensor=ds_cfg["sensor"], channels=ds_cfg["channels"], norm_mode=cfg["norm_mode"],
                               ignore_index=cfg["ignore_index"], seed_num=cfg.get("seed_num"), train_split_pct=0.8,
                               output_metadata=True, norm_params=cfg.get("norm_params"),
                               **(ds_cfg.get("dataset_kwargs") or {}))

    dev = torch.device(device)
    if calibrate is not None and calibrate >= dataset.n_classes:
        raise ValueError(f"calibrate: class {calibrate} not in 0..{dataset.n_classes - 1}")
    model, chosen = load_eval_model(cfg, checkpoint_path, weights, dataset.n_channels, dataset.n_classes, dev)
    net = model.model
    metrics = model.test_metrics
    ignore = model._loss_ignore          # -100 when the model has no ignore_index (as load_from_checkpoint builds it)

    pred_dir = prediction_dir(cfg, experiment_dir, checkpoint_path, eval_dataset_name)
    os.makedirs(pred_dir, exist_ok=True)

    image_f1, region_f1 = defaultdict(list), defaultdict(list)
    image_iou, region_iou = defaultdict(list), defaultdict(list)
    stitcher = GpuImageStitcher(net, dev, blend=blend) if predict_images else None
    gt: Dict[str, torch.Tensor] = {}
    where: Dict[str, tuple] = {}         # canvas key -> (region, image name)
    loader = TileLoader(dataset, batch_size or cfg["batch_size"], dev, shuffle=False, num_workers=n_workers,
                        ignore_index=cfg["ignore_index"], device_assembly=True, device_resize=True)
    hist = top = None                    # calibrate: int64 device accumulators, read once at the end
    with torch.no_grad():
        for batch in loader:
            probs, counts = eval_forward(net, model._gather_sources(batch), codes, batch["target"], ignore,
                                         want_probs=predict_images or calibrate is not None)   # counts: [B, k, k]
            if calibrate is not None:                                         # one launch, no host read
                h, t = net.prob_histogram(batch["target"], ignore, calibrate_bins, probs=probs)
                hist, top = (h, t) if hist is None else (hist + h, top + t)
            metrics.accumulate_counts(counts)                                 # each crop once (see module docstring)
            per_crop = metrics.reduce_batch(counts)
            vals = torch.stack([per_crop[f"{metrics.prefix}MulticlassF1Score"],
                                per_crop[f"{metrics.prefix}MulticlassJaccardIndex"]]).cpu().tolist()  # one host read
            meta = batch["metadata"]
            for i, md in enumerate(meta):
                image_f1[md["image_path"]].append(vals[0][i])
                image_iou[md["image_path"]].append(vals[1][i])
                region_f1[md["region_name"]].append(vals[0][i])
                region_iou[md["region_name"]].append(vals[1][i])
            if predict_images:
                keys, crops = [], []
                for i, md in enumerate(meta):
                    name = os.path.splitext(os.path.split(md["image_path"])[1])[0]
                    key = f"{md['region_name']}/{name}"
                    cp = md["crop_params"]
                    keys.append(key)
                    crops.append(cp)
                    if key not in gt:
                        gt[key] = torch.zeros(cp.og_height, cp.og_width, dtype=torch.uint8, device=dev)
                        where[key] = (md["region_name"], name)
                    # ceil of the averaged [target == 1] canvas (predict.py:311-314, 372-373) = any covering crop says 1
                    g = gt[key][cp.h0:cp.hE, cp.w0:cp.wE]
                    torch.maximum(g, (batch["target"][i, :cp.hE - cp.h0, :cp.wE - cp.w0] == 1).to(torch.uint8), out=g)
                stitcher.add_images(range(len(meta)), keys, crops, [c.og_height for c in crops],
                                    [c.og_width for c in crops], probs=probs)

        probabilities = {}
        if predict_images:
            for key, (region, name) in where.items():
                prob, am = stitcher.combine(key)
                prob_h, am_h, gt_h = prob.cpu().numpy(), am.cpu().numpy(), gt[key].cpu().numpy()
                out_dir = os.path.join(pred_dir, "image_predictions", region, name)
                os.makedirs(out_dir, exist_ok=True)
                write_strip_tiff(os.path.join(out_dir, "pred_class.tif"),
                                 np.ascontiguousarray((prob_h >= 0.5).astype(np.float32).transpose(2, 0, 1)))
                write_png(os.path.join(out_dir, "pred_softmax.png"), softmax_png(prob_h))
                write_png(os.path.join(out_dir, "cm.png"), conf_matrix_image(am_h, gt_h))
                probabilities[key] = prob_h

        all_metrics = {k: v.item() for k, v in metrics.compute().items()}
        all_metrics["eval_dataset"] = eval_dataset_name
        if chosen == "ema" or weights != "auto":      # (a plain checkpoint under 'auto' writes the file it always wrote)
            all_metrics["weights"] = chosen
        if codes is not None:
            all_metrics["tta"] = recorded(tta, codes)
        if blend != "uniform":
            all_metrics["blend"] = blend
        with open(os.path.join(pred_dir, "metrics.json"), "w") as fh:
            json.dump(all_metrics, fh, indent=4)
        write_ranked_files(pred_dir, image_f1, image_iou, region_f1, region_iou)

    extra = {}
    if calibrate is not None:
        from .calibration import report
        if hist is None:
            raise ValueError("calibrate: the data set has no crops")
        rep = report(hist.cpu().numpy(), top.cpu().numpy(), calibrate, confusion=metrics.confusion().cpu().numpy())
        if codes is not None:
            rep["tta"] = recorded(tta, codes)
        with open(os.path.join(pred_dir, "calibration.json"), "w") as fh:
            json.dump(rep, fh)
        extra = {"best_threshold": rep["best_threshold"], "best_f1": rep["best_f1"]}
    return {**extra, "pred_dir": pred_dir, "metrics": all_metrics, "image_stats_f1": dict(image_f1),
            "image_stats_iou": dict(image_iou), "region_stats_f1": dict(region_f1), "region_stats_iou": dict(region_iou),
            "probabilities": probabilities}


def build_parser() -> argparse.ArgumentParser:
    """predict.py:20-70's command line plus --data_root, --batch_size, --device and --tta."""
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint_path", type=str)
    ap.add_argument("--eval_dataset_name", type=str)
    # as in the reference, the flag defaults to True and so cannot be switched off
    ap.add_argument("--predict_images", default=True, action="store_true", help="Create image predictions")
    ap.add_argument("--eval_region", type=str)
    ap.add_argument("--eval_dataset_split", type=str, default="test")
    ap.add_argument("--n_workers", type=int, default=None)
    ap.add_argument("--data_root", type=str, required=True, help="directory that holds CSDAP_complete/")
    ap.add_argument("--batch_size", type=int, default=None, help="crops per eval forward (default: the config's)")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--tta", type=str, default=None, choices=sorted(VIEW_SETS),
                    help="test-time augmentation: average each crop's softmax over its flips (hflip, flips) or all eight "
                         "flips / 90-degree rotations (d4, square crops only); default: none")
    ap.add_argument("--blend", type=str, default="uniform", choices=["uniform", "linear", "hann"],
                    help="how overlapping crops are averaged in the stitched images: equal weights (uniform, the default) "
                         "or a window that falls off towards the crop's border (linear, hann); metrics are per crop and "
                         "do not change")
    ap.add_argument("--weights", type=str, default="auto", choices=list(WEIGHT_CHOICES),
                    help="which weights of the checkpoint to serve: its state_dict (raw), its weight EMA (ema; an error when "
                         "the checkpoint has none) or the EMA when there is one (auto, the default)")
    ap.add_argument("--norm_params", type=str, default=None,
                    help="parameter file of norm_mode 'global' (config key norm_params; "
                         "python -m floodplanet_code_amd.datasets.stats writes it)")
    ap.add_argument("--calibrate", type=int, nargs="?", const=1, default=None, metavar="CLS",
                    help="also write calibration.json: the threshold sweep (precision / recall / F1 / IoU per threshold), "
                         "best thresholds, average precision and calibration error of class CLS against the rest "
                         "(default 1, water), from a probability histogram accumulated over the crops on the device")
    ap.add_argument("--calibrate_bins", type=int, default=256,
                    help="histogram bins of --calibrate, a power of two in 2..1024 (default 256)")
    return ap


def main(argv: Optional[List[str]] = None) -> None:
    args = build_parser().parse_args(argv)
    if args.calibrate is not None:       # option errors before anything is read
        from .calibration import check_bins
        check_bins(args.calibrate_bins)
        if args.calibrate < 0:
            raise ValueError(f"calibrate: class {args.calibrate} is negative")
    experiment_dir = "/".join(args.checkpoint_path.split("/")[:-2])
    cfg = resolve_cfg(experiment_dir, args.checkpoint_path)
    name = args.eval_dataset_name if args.eval_dataset_name is not None else cfg["dataset"]["name"]
    n_workers = args.n_workers if args.n_workers is not None else cfg["n_workers"]
    if args.norm_params is not None:
        cfg["norm_params"] = args.norm_params
    out = predict(cfg, experiment_dir, args.checkpoint_path, eval_dataset_name=name, predict_images=args.predict_images,
                  eval_region=args.eval_region, eval_dataset_split=args.eval_dataset_split, n_workers=n_workers,
                  data_root=args.data_root, batch_size=args.batch_size, device=args.device, tta=args.tta,
                  weights=args.weights, blend=args.blend, calibrate=args.calibrate, calibrate_bins=args.calibrate_bins)
    print(json.dumps({"pred_dir": out["pred_dir"], **out["metrics"]}))


if __name__ == "__main__":
    main()
