"""Minimal trainer that drives the plugin exactly the way st_water_seg/fit.py:16-103 drives it through
pytorch_lightning -- for environments where Lightning / Hydra / the GeoTIFF stack are absent (this image, the GPU
box).  When those packages exist, use the reference's own fit.py with `floodplanet_code_amd.models.build_model`
(INTEGRATION.md); this file only restates the loop Lightning's automatic optimisation runs:

    per epoch:  for batch in train_loader:  opt.zero_grad(); loss = model.training_step(batch, i);
                                            loss.backward(); opt.step()                         (fit.py:95-97)
                for batch in valid_loader:  model.validation_step(batch, i)
                model.validation_epoch_end(outputs)  -> 'val_MulticlassJaccardIndex'
                keep the top-k checkpoints by that metric, named as fit.py:80-85 names them.

`cfg` is a plain nested dict with the reference's key names (conf/config.yaml): lr, batch_size, n_epochs,
crop_height, crop_width, ignore_index, save_topk_models, limit_train_batches, limit_val_batches,
model: {name, model_kwargs}, plus `n_channels` (dict) / `n_classes` that the reference reads off the dataset.
fit_model takes any iterable of batches: SyntheticTiles below (tests, benchmarks), or the loaders of
floodplanet_code_amd.datasets over real rasters, which is what the command line builds:

    python -m floodplanet_code_amd.fit DATA_ROOT --exp_dir DIR [--sensor S1] [--eval_region R ...] [--crop H W] [...]

DATA_ROOT holds CSDAP_complete/.  The train / valid FloodplanetTiles are made as fit.py:25-53 makes them; --loader scene
(default) keeps every scene on the device and cuts finished batches there (datasets.SceneTileLoader), --loader tile streams
tiles through DataLoader workers (datasets.TileLoader with device assembly and resampling).  One JSON line comes out: the
best checkpoint and the per-epoch history.  The checkpoint's hyper_parameters carry the data set keys, so predict / infer
run on it without a config file.

fit_model is made of train_epoch, validate, history_entry and TopKCheckpoints; main of cfg_from_args, build_datasets,
build_loaders and run_summary.  The command line's options belong to four values, each built in one place and handed down
unchanged: LossOptions (loss_options.py), OptimOptions (optim_options.py), TileOptions (datasets/sampling.py) and LrSchedule
(schedule.py).  A new training option is one field and one check there, read in that class's from_args, and one flag in
build_parser below; cfg_from_args and main do not change for it.
"""
from __future__ import annotations

import argparse
import json
import os
import time
from typing import Dict, Iterable, List, Optional

import torch

from .datasets.sampling import SAMPLING_KEYWORDS as SAMPLING_OPTIONS, TileOptions
from .loss_options import BALANCED, LossOptions, parse_class_weights  # noqa: F401 (parse_class_weights: callers find it here)
from .models import build_model
from .optim_options import OptimOptions
from .schedule import CFG_KEYS as SCHEDULE_OPTIONS, KINDS as LR_SCHEDULES, LrSchedule

DEFAULTS = dict(lr=1e-4, batch_size=10, n_epochs=11, crop_height=300, crop_width=300, ignore_index=0,
                save_topk_models=3, limit_train_batches=None, limit_val_batches=None, log_image_iter=200,
                seed_num=0, model=dict(name="ef_model", model_kwargs=dict(optimizer_name="adam")))
N_CLASSES = 3          # of the data set the command line trains on (FloodplanetTiles.n_classes)


class SyntheticTiles:
    """An iterable of batches shaped like the default collate of Floodplanet_Dataset.__getitem__
    (datasets/floodplanet.py:644-648): image f32 [B,C,h,w] in [0,1), target i64 [B,h,w], mean/std [B,C,1,1]."""

    def __init__(self, n_batches: int, batch_size: int, n_channels: Dict[str, int], height: int, width: int,
                 device, seed: int = 0, extras: Iterable[str] = ()):
        self.n_batches, self.B, self.h, self.w = n_batches, batch_size, height, width
        self.n_channels, self.device, self.seed = n_channels, torch.device(device), seed
        self.C = n_channels.get("ms_image", next(iter(n_channels.values())))
        self.extras = [k for k in n_channels if k != "ms_image" and k in
                       ("dem", "slope", "preflood", "pre_post_difference", "hand")] or list(extras)

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        g = torch.Generator(device=self.device).manual_seed(self.seed)
        yy, xx = torch.meshgrid(torch.arange(self.h, device=self.device), torch.arange(self.w, device=self.device),
                                indexing="ij")
        for _ in range(self.n_batches):
            ph = torch.rand(self.B, 3, device=self.device, generator=g) * 6.28
            f = (torch.sin(yy[None] * 0.07 + ph[:, 0, None, None]) + torch.cos(xx[None] * 0.05 + ph[:, 1, None, None])
                 + torch.sin((xx + yy)[None] * 0.03 + ph[:, 2, None, None]))
            target = (f > 0.3).long()                      # {0 = not flood / ignored under ignore_index 0, 1 = flood}
            image = torch.rand(self.B, self.C, self.h, self.w, device=self.device, generator=g)
            image[:, 0] = 0.5 * image[:, 0] + 0.5 * (f > 0.3).float()   # a learnable signal in band 0
            batch = {"image": image, "target": target,
                     "mean": torch.zeros(self.B, self.C, 1, 1, device=self.device),
                     "std": torch.ones(self.B, self.C, 1, 1, device=self.device)}
            for k in self.extras:
                batch[k] = torch.rand(self.B, 1, self.h, self.w, device=self.device, generator=g)
            yield batch


def _limited(loader, limit: Optional[int]):
    for i, b in enumerate(loader):
        if limit is not None and i >= limit:
            break
        yield i, b


# ---------------------------------------------------------------------------------------------------- fit_model's parts
def train_epoch(model, opt, loader, limit: Optional[int], schedule: Optional[LrSchedule], n_steps: int, device="cuda:0"):
    """One epoch of Lightning's automatic optimisation over at most `limit` batches -> (the last step's loss, tiles trained,
    host seconds, n_steps).  n_steps counts the run's optimiser steps: with a schedule, step n runs at schedule.lr(n), set
    into the optimiser before it.  The seconds are closed by the epoch's one device synchronise, so they cover finished
    steps; what the caller reads off the device afterwards sits behind it."""
    loss, n_tiles, t0 = None, 0, time.perf_counter()
    for i, batch in _limited(loader, limit):
        opt.zero_grad()
        loss = model.training_step(batch, i)
        loss.backward()
        n_steps += 1
        if schedule is not None:
            opt.param_groups[0]["lr"] = schedule.lr(n_steps)
        opt.step()
        model.global_step += 1
        n_tiles += int(batch["image"].shape[0])
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    return loss, n_tiles, time.perf_counter() - t0, n_steps


def validate(model, loader, limit: Optional[int]) -> float:
    """The validation loop over at most `limit` batches, on the weight EMA where the model keeps one (swapped in once) ->
    val_MulticlassJaccardIndex."""
    model.valid_metrics.reset()
    outs = []
    with model.eval_weights():
        for i, batch in _limited(loader, limit):
            outs.append(model.validation_step(batch, i))
    model.validation_epoch_end(outs)
    return float(model.logged.get("val_MulticlassJaccardIndex", torch.zeros(())))


def history_entry(epoch: int, train_loss: float, miou: float, n_tiles: int, seconds: float, *, train_region=None, lr=None,
                  clip_state=None, weight_decay=None, decayed_tensors=None, plan=None) -> dict:
    """An epoch's entry of model.history from the numbers collected; a key after the first four is there only when its
    number is (fit_model's docstring says when that is)."""
    entry = {"epoch": epoch, "train_loss": train_loss, "val_MulticlassJaccardIndex": miou,
             "train_tiles_per_s": n_tiles / seconds if n_tiles and seconds > 0 else None}
    if train_region is not None:
        entry["train_region"] = train_region
    if lr is not None:
        entry["lr"] = lr                                                     # the last step's
    if clip_state is not None:
        entry["grad_norm"] = clip_state["grad_norm"]                         # the last step's, before clipping
        entry["clipped_steps"] = clip_state["clipped_steps"]                 # of the run so far
    if weight_decay is not None:
        entry["weight_decay"] = weight_decay
        entry["decayed_tensors"] = decayed_tensors
    if plan is not None:
        entry["plan"] = dict(plan)
    return entry


class TopKCheckpoints:
    """The k best checkpoints by val_MulticlassJaccardIndex under exp_dir/checkpoints, named as the reference's fit.py:80-85
    names them.  Among equal metrics the earlier epoch ranks first.  Without an exp_dir nothing is written and `best`
    stays ''."""

    def __init__(self, exp_dir: Optional[str], k: int, hyper_parameters: dict):
        self.dir, self.k, self.hyper_parameters = os.path.join(exp_dir, "checkpoints") if exp_dir else None, k, hyper_parameters
        self.kept: List = []                                                 # (metric, path), best first
        if self.dir:
            os.makedirs(self.dir, exist_ok=True)

    def save(self, model, epoch: int, miou: float) -> None:
        if not self.dir:
            return
        path = os.path.join(self.dir, f"model-epoch={epoch:02d}-val_MulticlassJaccardIndex={miou:.4f}.ckpt")
        ckpt = {"state_dict": model.state_dict(), "epoch": epoch, "hyper_parameters": dict(self.hyper_parameters)}
        hook = getattr(model, "on_save_checkpoint", None)                    # (the weight EMA: "ema_state_dict")
        if hook is not None:
            hook(ckpt)
        torch.save(ckpt, path)
        self.kept.append((miou, path))
        self.kept.sort(key=lambda t: -t[0])                                  # stable: a tie keeps the earlier epoch ahead
        for _, stale in self.kept[self.k:]:
            if os.path.exists(stale):
                os.remove(stale)
        self.kept = self.kept[:self.k]

    @property
    def best(self) -> str:
        return self.kept[0][1] if self.kept else ""


def fit_model(cfg: dict, train_loader, valid_loader, n_channels: Dict[str, int], n_classes: int = 3,
              exp_dir: Optional[str] = None, device="cuda:0", to_rgb_fcn=None, model=None) -> str:
    """Restatement of fit.py:16-103 without Lightning.  Returns the best checkpoint path ('' if exp_dir is None).
    model: an already built model to train in place of the build_model call (a loader that needs the network's context,
    SceneTileLoader, is made before fit_model runs).  The trained model keeps `history`, one dict per epoch: epoch, train_loss
    (the last step's), train_region (that step's region term R, when the model's region_weight > 0),
    val_MulticlassJaccardIndex and train_tiles_per_s -- the tiles of the epoch's training loop over its
    host time, closed by one device synchronise per epoch (None when the train loader yields nothing) -- plus `plan`, the
    train loader's `last_plan`, when it has one.  With an lr schedule (cfg lr_schedule / warmup_steps / min_lr: schedule.lr_at
    per optimiser step, over n_epochs x the loader's length) or gradient clipping (the model's grad_clip_norm) an entry also
    carries `lr`, the last step's; with clipping `grad_norm`, the last step's global gradient norm before clipping, and
    `clipped_steps`, the steps clipped so far.  With weight decay (the model's weight_decay) an entry carries `weight_decay`
    and `decayed_tensors`, the number of tensors it acts on."""
    c = dict(DEFAULTS)
    c.update(cfg or {})
    torch.manual_seed(c["seed_num"])                                         # pl.seed_everything(seed_num)
    if model is None:
        model = build_model(c["model"]["name"], n_channels, n_classes, c["lr"], log_image_iter=c["log_image_iter"],
                            to_rgb_fcn=to_rgb_fcn, ignore_index=c["ignore_index"], **c["model"].get("model_kwargs", {}))
    model = model.to(device)
    opt = model.configure_optimizers()
    # one lr per optimiser step where the config has a schedule; gradient clipping is the model's (grad_clip_norm -> HipAdam)
    # (the loader's length only where it is needed: a loader that plans its epochs takes its census for it)
    schedule = LrSchedule.from_cfg(c, len(train_loader)) if any(k in c for k in SCHEDULE_OPTIONS) else None
    optim = model.optim_options
    clipping = optim.grad_clip_norm is not None
    n_steps = 0
    checkpoints = TopKCheckpoints(exp_dir, c["save_topk_models"], c)
    history = []
    for epoch in range(c["n_epochs"]):
        model.current_epoch = epoch
        loss, n_tiles, seconds, n_steps = train_epoch(model, opt, train_loader, c["limit_train_batches"], schedule, n_steps,
                                                      device)
        # read once per epoch, behind train_epoch's synchronise: R of the last step, before validation rewrites it
        region = getattr(model, "region_weight", 0.0) > 0.0 and n_tiles
        train_region = float(model.model.last_region_terms()[0]) if region else None
        clip_state = model.model.grad_clip_state() if clipping and n_tiles else None
        miou = validate(model, valid_loader, c["limit_val_batches"])
        decaying = optim.weight_decay > 0.0
        history.append(history_entry(
            epoch, float(loss.detach()), miou, n_tiles, seconds, train_region=train_region, clip_state=clip_state,
            lr=float(opt.param_groups[0]["lr"]) if schedule is not None or clipping else None,
            weight_decay=float(opt.param_groups[0]["weight_decay"]) if decaying else None,
            decayed_tensors=len(model.model.decayed_parameter_names()) if decaying else None,
            plan=getattr(train_loader, "last_plan", None)))                  # a loader that chooses its tiles says which
        checkpoints.save(model, epoch, miou)
    model.history = history
    fit_model.last_model = model
    return checkpoints.best


# ---------------------------------------------------------------------------------------------------------- command line
def build_parser() -> argparse.ArgumentParser:
    """Defaults: DEFAULTS above and predict.CONFIG_DEFAULTS (the reference's conf/config.yaml) where they name the key."""
    from .predict import CONFIG_DEFAULTS as D
    ap = argparse.ArgumentParser(description="Train a water segmentation model on FloodPlanet rasters (fit.py of st_water_seg).")
    ap.add_argument("data_root", type=str, help="directory that holds CSDAP_complete/")
    ap.add_argument("--exp_dir", type=str, required=True, help="experiment directory (checkpoints/ goes under it)")
    ap.add_argument("--sensor", type=str, default=D["dataset"]["sensor"])
    ap.add_argument("--channels", type=str, default=D["dataset"]["channels"])
    ap.add_argument("--eval_region", type=str, nargs="*", default=[D["eval_region"]],
                    help="validation region(s); give the flag without a value for the seeded random split by image")
    ap.add_argument("--train_split_pct", type=float, default=D["train_split_pct"])
    ap.add_argument("--crop", type=int, nargs=2, metavar=("H", "W"), default=[D["crop_height"], D["crop_width"]])
    ap.add_argument("--stride", type=int, default=D["crop_stride"])
    ap.add_argument("--batch_size", type=int, default=D["batch_size"])
    ap.add_argument("--n_epochs", type=int, default=D["n_epochs"])
    ap.add_argument("--lr", type=float, default=D["lr"])
    ap.add_argument("--norm_mode", type=str, default="none", choices=["none", "local", "global"])
    ap.add_argument("--norm_params", type=str, default=None,
                    help="parameter file of norm_mode 'global' (python -m floodplanet_code_amd.datasets.stats writes it)")
    ap.add_argument("--model", type=str, default="ms_model", help="ms_model, ef_model or lf_model")
    ap.add_argument("--base_channels", type=int, default=64)
    ap.add_argument("--precision", type=str, default="fp32", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--loader", type=str, default="scene", choices=["scene", "tile"],
                    help="scene: device-resident scenes, one launch per batch; tile: DataLoader workers stream tiles")
    ap.add_argument("--n_workers", type=int, default=D["n_workers"],
                    help="tile: DataLoader workers; scene: processes of the one-time decode")
    ap.add_argument("--seed", type=int, default=D["seed_num"])
    ap.add_argument("--ignore_index", type=int, default=D["ignore_index"])
    ap.add_argument("--save_topk_models", type=int, default=D["save_topk_models"])
    ap.add_argument("--class_weights", type=str, nargs="+", default=None, metavar="W",
                    help="cross-entropy class weights: 'balanced' (from the TRAIN split's class frequencies) or one number "
                         "per class")
    ap.add_argument("--label_smoothing", type=float, default=0.0, help="cross-entropy label smoothing in [0, 1)")
    ap.add_argument("--focal_gamma", type=float, default=0.0, metavar="F",
                    help="focal loss: every pixel's cross-entropy term times (1 - p[target])^F, F >= 0 (default 0: plain "
                         "cross entropy); combines with --class_weights, not with --label_smoothing")
    ap.add_argument("--region_loss", type=str, default=None, choices=["dice", "jaccard", "tversky"],
                    help="add a soft region term over all classes to the cross entropy: dice (alpha = beta = 0.5), jaccard "
                         "(alpha = beta = 1) or tversky (--tversky A B); combines with every cross-entropy option")
    ap.add_argument("--region_weight", type=float, default=None, metavar="F",
                    help="the region term's weight, >= 0 (default 1 once --region_loss is given)")
    ap.add_argument("--tversky", type=float, nargs=2, default=None, metavar=("A", "B"),
                    help="--region_loss tversky: the weights of false positives (A) and false negatives (B)")
    ap.add_argument("--region_smooth", type=float, default=None, metavar="S",
                    help="the region term's smoothing, > 0 (default 1)")
    ap.add_argument("--ema_decay", type=float, default=None, metavar="F",
                    help="keep an exponential moving average of the weights with this decay in [0, 1): validation, the "
                         "checkpoint choice and the checkpoint's ema_state_dict use it (default: no EMA)")
    ap.add_argument("--no_ema_warmup", action="store_true",
                    help="use --ema_decay from the first update on (default: min(decay, (1 + n) / (10 + n)))")
    ap.add_argument("--grad_clip", type=float, default=None, metavar="F",
                    help="clip the global L2 norm of the gradients to F > 0 inside every optimiser step (clip_grad_norm_ "
                         "ahead of Adam, on the device; default: no clipping)")
    ap.add_argument("--weight_decay", type=float, default=None, metavar="F",
                    help="decoupled weight decay (AdamW) F > 0 inside the fused Adam step, on the conv and head weights "
                         "(every tensor with ndim >= 2; default: no decay)")
    ap.add_argument("--decay_all", action="store_true",
                    help="with --weight_decay: decay every tensor, biases and BatchNorm included")
    ap.add_argument("--lr_schedule", type=str, default=None, choices=list(LR_SCHEDULES),
                    help="learning rate after the warm-up: constant (default), or linear / cosine / poly (power 0.9) decay "
                         "from --lr to --min_lr over the run's optimiser steps")
    ap.add_argument("--warmup_steps", type=int, default=None, metavar="N",
                    help="raise the learning rate linearly over the first N optimiser steps (default 0)")
    ap.add_argument("--min_lr", type=float, default=None, metavar="F",
                    help="the learning rate a decaying --lr_schedule ends at, in [0, --lr] (default 0)")
    ap.add_argument("--tile_sampling", type=str, default=None, choices=["all", "labelled", "balanced"],
                    help="--loader scene, train split: which tiles an epoch sees -- all (default), labelled (drop the tiles "
                         "the loss ignores entirely) or balanced (a --water_share of tiles with water)")
    ap.add_argument("--min_trainable_frac", type=float, default=None, metavar="F",
                    help="labelled / balanced: keep a tile only if this share of it, in [0, 1], is not ignored (default 0: "
                         "one pixel)")
    ap.add_argument("--water_share", type=float, default=None, metavar="F",
                    help="balanced: the share of an epoch's tiles, in [0, 1], drawn from the tiles with water (default 0.5)")
    ap.add_argument("--min_water_frac", type=float, default=None, metavar="F",
                    help="balanced: a tile counts as a water tile if this share of it, in [0, 1], is water (default 0: "
                         "one pixel)")
    ap.add_argument("--crop_jitter", type=int, default=None, metavar="J",
                    help="--loader scene, train split: move every crop by its own offset in [-J, J]^2 each epoch (default 0)")
    ap.add_argument("--aug_gain", type=float, default=None, metavar="G",
                    help="--loader scene, train split: one gain per sample, uniform in [1 - G, 1 + G], in units of the "
                         "normalised batch (like every --aug_* option; default: none of them)")
    ap.add_argument("--aug_band_gain", type=float, default=None, metavar="G",
                    help="one more gain per band, uniform in [1 - G, 1 + G]")
    ap.add_argument("--aug_brightness", type=float, default=None, metavar="B",
                    help="one bias per sample, uniform in [-B, B]")
    ap.add_argument("--aug_noise", type=float, default=None, metavar="S",
                    help="additive unit-variance noise times a per-sample sigma, uniform in [0, S]")
    ap.add_argument("--aug_band_drop", type=float, default=None, metavar="P",
                    help="zero each band with probability P in [0, 1), never every band of a sample")
    ap.add_argument("--aug_likelihood", type=float, default=None, metavar="L",
                    help="one coin per sample for the gain / brightness / noise / band-drop group (default 1)")
    ap.add_argument("--aug_zoom", type=float, nargs=2, default=None, metavar=("ZMIN", "ZMAX"),
                    help="--loader scene, train split: resample every crop by its own factor, log-uniform in [ZMIN, ZMAX] "
                         "within [0.5, 2] (bilinear image, nearest labels; above 1 magnifies)")
    ap.add_argument("--no_transforms", action="store_true", help="train without hflip / vflip / rotate")
    ap.add_argument("--no_shuffle", action="store_true", help="train in data-set order")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


MODEL_KEYWORDS = ("optimizer_name", "base_channels", "precision")      # the reference's; the extensions follow them


def cfg_from_args(args, class_weights=None) -> dict:
    """The reference-style config of a command line: what fit_model trains with and dumps into the checkpoint.  Each concern
    is read and checked by its own options value -- LossOptions, OptimOptions, TileOptions, LrSchedule (.from_args) -- and
    recorded only where the command line set it, so a plain command line gives the config it always gave: the loss and
    optimiser keywords in model_kwargs, `sampling` and `augmentation` beside `model`, the schedule's keys at the top level.
    class_weights: the resolved numeric weights in place of the command line's (the data decides 'balanced', so main()
    resolves it; set_class_weights does the same to a finished config)."""
    loss, optim = LossOptions.from_args(args, N_CLASSES), OptimOptions.from_args(args)
    schedule, tiles = LrSchedule.from_args(args), TileOptions.from_args(args)
    cfg = dict(lr=args.lr, batch_size=args.batch_size, n_epochs=args.n_epochs, crop_height=args.crop[0],
               crop_width=args.crop[1], crop_stride=args.stride, ignore_index=args.ignore_index,
               save_topk_models=args.save_topk_models, seed_num=args.seed, n_workers=args.n_workers,
               eval_region=list(args.eval_region) if args.eval_region else None, train_split_pct=args.train_split_pct,
               norm_mode=None if args.norm_mode == "none" else args.norm_mode, norm_params=args.norm_params,
               dataset=dict(name="floodplanet", sensor=args.sensor, channels=args.channels, dataset_kwargs=None),
               model=dict(name=args.model, model_kwargs=dict(optimizer_name="adam", base_channels=args.base_channels,
                                                             precision=args.precision,
                                                             **loss.given_kwargs(getattr(args, "region_loss", None) is not None),
                                                             **optim.given_kwargs())))
    if class_weights is not None:
        set_class_weights(cfg, class_weights)
    if tiles.sampling_cfg():
        cfg["sampling"] = tiles.sampling_cfg()
    if tiles.augmentation_cfg():               # the training recipe's record; predict and infer do not read it
        cfg["augmentation"] = tiles.augmentation_cfg()
    if schedule is not None:
        cfg.update(schedule.given_cfg())
    return cfg


def set_class_weights(cfg: dict, weights) -> None:
    """The one class_weights entry of the config's model_kwargs, where cfg_from_args lists it: first of the extensions."""
    kwargs = cfg["model"]["model_kwargs"]
    items = [(k, v) for k, v in kwargs.items() if k != "class_weights"]
    items.insert(len(MODEL_KEYWORDS), ("class_weights", [float(v) for v in weights]))
    kwargs.clear()
    kwargs.update(items)


# --------------------------------------------------------------------------------------------------------- main's parts
def build_datasets(args, cfg: dict):
    """(train, valid) FloodplanetTiles as fit.py:25-53 makes them (the transforms run on the device, per batch)."""
    import copy
    from .datasets import FloodplanetTiles, generate_image_slice_object
    slice_params = generate_image_slice_object(cfg["crop_height"], cfg["crop_width"], cfg["crop_stride"])
    return tuple(FloodplanetTiles(args.data_root, split, slice_params, eval_region=copy.copy(cfg["eval_region"]),
                                  sensor=args.sensor, channels=args.channels, norm_mode=cfg["norm_mode"],
                                  ignore_index=cfg["ignore_index"], seed_num=cfg["seed_num"],
                                  train_split_pct=cfg["train_split_pct"], norm_params=cfg["norm_params"])
                 for split in ("train", "valid"))


def build_loaders(args, cfg: dict, model, train_ds, valid_ds):
    """(train, valid) loaders of --loader.  The scene loader borrows the device context of the model's net, so the model
    comes first; only the train split is shuffled, transformed and cut by the config's recipe (TileOptions.from_cfg)."""
    from .datasets import SceneTileLoader, TileLoader
    common = dict(seed=cfg["seed_num"], ignore_index=cfg["ignore_index"], num_workers=args.n_workers)
    train_only = dict(shuffle=not args.no_shuffle, transforms=None if args.no_transforms else {})
    if args.loader == "scene":
        train_only["options"] = TileOptions.from_cfg(cfg)

    def make(ds, **kw):
        if args.loader == "scene":
            return SceneTileLoader(ds, cfg["batch_size"], args.device, net=model.model, **common, **kw)
        return TileLoader(ds, cfg["batch_size"], args.device, device_assembly=True, device_resize=True, **common, **kw)
    return make(train_ds, **train_only), make(valid_ds)              # valid: every tile, where the grid puts it


def run_summary(cfg: dict, loader: str, checkpoint: str, n_train: int, n_valid: int, model, class_counts) -> dict:
    """The record main() prints as one JSON line."""
    out = {"checkpoint": checkpoint, "loader": loader, "train_tiles": n_train, "valid_tiles": n_valid,
           "history": model.history,
           "class_counts": None if class_counts is None else [int(v) for v in class_counts],
           "class_weights": None if model.class_weights is None else list(model.class_weights)}
    if "sampling" in cfg:
        out["tile_sampling"] = dict(cfg["sampling"])
    if "augmentation" in cfg:
        out["augmentation"] = dict(cfg["augmentation"])
    if model.weight_decay > 0.0:
        out["weight_decay"] = model.weight_decay
        out["decayed_tensors"] = len(model.model.decayed_parameter_names())
    return out


def main(argv: Optional[List[str]] = None) -> dict:
    from .datasets.class_weights import balanced_class_weights, dataset_label_boxes, label_class_counts_host
    ap = build_parser()
    args = ap.parse_args(argv)
    try:
        cfg = {**DEFAULTS, **cfg_from_args(args)}          # the one config: what fit_model merges and the checkpoint holds
    except ValueError as e:
        ap.error(str(e))
    balanced = parse_class_weights(args.class_weights) == BALANCED
    train_ds, valid_ds = build_datasets(args, cfg)
    wanted = cfg["model"]["model_kwargs"].get("class_weights")
    if wanted is not None and len(wanted) != train_ds.n_classes:
        ap.error(f"--class_weights: {len(wanted)} weights for {train_ds.n_classes} classes")
    class_counts = None
    if balanced and args.loader == "tile":
        # the streaming loader's label rasters are on the host: the contract of fu_label_class_counts in numpy, same boxes
        class_counts = label_class_counts_host(dataset_label_boxes(train_ds), cfg["ignore_index"], train_ds.n_classes)
        set_class_weights(cfg, balanced_class_weights(class_counts, cfg["ignore_index"]))
    torch.manual_seed(cfg["seed_num"])                     # the initial weights are drawn here, not in fit_model
    model = build_model(cfg["model"]["name"], train_ds.n_channels, train_ds.n_classes, cfg["lr"],
                        log_image_iter=cfg["log_image_iter"], to_rgb_fcn=None, ignore_index=cfg["ignore_index"],
                        **cfg["model"]["model_kwargs"]).to(args.device)
    train, valid = build_loaders(args, cfg, model, train_ds, valid_ds)
    if balanced and args.loader == "scene":                # counted on the device, from the label rasters resident there
        class_counts = train.class_counts().cpu().numpy()
        set_class_weights(cfg, balanced_class_weights(class_counts, cfg["ignore_index"]))
        model.replace_loss_options(class_weight=cfg["model"]["model_kwargs"]["class_weights"])
    best = fit_model(cfg, train, valid, train_ds.n_channels, train_ds.n_classes, exp_dir=args.exp_dir, device=args.device,
                     model=model)
    out = run_summary(cfg, args.loader, best, len(train_ds), len(valid_ds), model, class_counts)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
