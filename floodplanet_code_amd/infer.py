"""Label-free scene inference: restatement of st_water_seg/infer.py:17-184 (driven over folders of scenes by
Batch_infer.sh) for machines without omegaconf, tifffile, PIL, scipy or einops.

    python -m floodplanet_code_amd.infer <exp>/checkpoints/<name>.ckpt INPUT... --out_dir DIR [...]

INPUT: .tif files, or directories searched recursively for *.tif.  Per scene it writes <out_dir>/<region>_pred/<image>.tif,
uint8 [H, W] = clip(argmax of the overlap-averaged softmax, 0, 1) * 255 (infer.py:179-184), and <out_dir>/summary.json.
The region is the grandparent directory when the parent directory is named after the sensor (CSDAP_complete/<region>/S1/),
else the parent directory.  What runs differently:
  * no labels: the output grid is the raster's own size, or --size H W / --scale F (CSDAP chips were trained at their
    label grid, e.g. --size 1024 1024); the reference's dataset needs a label raster and resamples to it;
  * the host decodes each scene once (DataLoader workers: TIFF decode + band selection); the scene is uploaded once and
    resampled once on the device into a resident grid -- fu_resize_lanczos4_tiles with B = 1 and the whole grid as the
    tile, the tables and sensor scaling training uses -- and every crop is cut, normalised and padded from HBM
    (fu_scene_crops), so there is no per-crop host work;
  * crops of consecutive scenes are packed into full batches of batch_size (scene order, then get_crop_slices order);
    per batch one fu_scene_crops, one eval forward (or views forward + merge with --tta), one batched stitch;
  * a scene is finalised as soon as its last crop is stitched: class map and class counts on the device, one
    device-to-host read, then its grid and canvases are released -- memory is bounded by the scenes in flight;
  * the stride (default min(crop_h, crop_w), infer.py:64-65) is clamped per axis to the grid, so a scene smaller than a
    crop gets one padded crop where get_crop_slices raises; boxes are clipped to the grid (get_crop_slices' bottom-edge
    quirk swaps the crop sizes, which only matters for non-square crops);
  * extension: the input's GeoTIFF georeferencing goes along with the class map (the reference drops it through PIL),
    rescaled to the output grid (geo_tags_for_grid); GDAL_NODATA is dropped;
  * extension: --blend linear|hann weights every crop with a window that falls off towards the tile's border
    (stitch.blend_window), so a pixel is decided by the crops that see it with their interior; the stride then defaults
    to half the crop.  --write_probs u8|f32 writes the stitched probabilities as <image>_prob.tif ([k, H, W]; u8 =
    rint(p * 255)), --write_margin the top-1 minus top-2 probability as <image>_margin.tif (uint8 [H, W]), with the class
    map's georeferencing.  Class map, class counts and these rasters come from one fu_stitch_finalize_maps launch.
  * extension: --sieve N merges every connected patch of the class map smaller than N pixels into its largest
    neighbouring patch (postprocess.sieve_host is the rule; --sieve_connectivity 4|8, --sieve_passes P), on the device,
    between the finalisation and the scene's one device-to-host read, which also carries the two counts of what changed.
    Only the written class map is sieved: class_pixels, the probability and the margin raster stay what the network said.
  * extension: --water_threshold T [--threshold_class C] replaces the argmax by a one-versus-rest rule -- class C (default
    1, water) where its stitched probability is >= T, else the best of the other classes -- inside the finalisation launch
    (fu_stitch_finalize_maps_ex); --calibration FILE takes C and T from the calibration.json of predict --calibrate.
    class_pixels follows the rule, the sieve runs on the thresholded map, the probability and margin rasters do not
    change; the summary records the rule under "threshold".
Out of scope: multi-GPU inference, inputs besides ms_image (dem, slope, hand, preflood), RGB outputs, BigTIFF or
compressed output.
"""
from __future__ import annotations

import argparse
import json
import os
import time
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .predict import CONFIG_DEFAULTS, WEIGHT_CHOICES, _merge, load_checkpoint_model, resolve_cfg
from .postprocess import check_sieve_options
from .stitch import BLEND_KINDS
from .tta import VIEW_SETS, view_codes

SCALE_MODES = {"S1": 1, "S2": 2, "L8": 3}                    # PS: 4 when stored as uint16, else 0
EXTRA_SOURCES = ("dem", "slope", "preflood", "pre_post_difference", "chirps", "hand")
PROB_FORMATS = ("u8", "f32")


# ---------------------------------------------------------------------------------------------------------- host side
def find_inputs(inputs: Sequence[str]) -> List[str]:
    """.tif files as given, directories searched recursively for *.tif (sorted), in argument order."""
    out = []
    for p in inputs:
        if os.path.isdir(p):
            found = []
            for d, _, files in os.walk(p):
                found += [os.path.join(d, f) for f in files if f.endswith(".tif")]
            out += sorted(found)
        elif p.endswith(".tif") and os.path.isfile(p):
            out.append(p)
        else:
            raise FileNotFoundError(f"infer: {p} is neither a .tif file nor a directory")
    if not out:
        raise FileNotFoundError(f"infer: no .tif file under {list(inputs)}")
    return out


def region_name(path: str, sensor: str) -> str:
    parts = os.path.normpath(os.path.abspath(path)).split(os.sep)
    return parts[-3] if parts[-2] == sensor and len(parts) >= 3 else parts[-2]


def output_path(out_dir: str, path: str, sensor: str) -> str:
    """<out_dir>/<region>_pred/<image>.tif (infer.py:148-150, 180-182)."""
    name = os.path.splitext(os.path.basename(path))[0]
    return os.path.join(out_dir, region_name(path, sensor) + "_pred", name + ".tif")


def side_output_path(out_path: str, kind: str) -> str:
    """<image>_prob.tif / <image>_margin.tif beside the class map <image>.tif."""
    return out_path[:-len(".tif")] + f"_{kind}.tif"


def default_stride(crop_h: int, crop_w: int, blend: str = "uniform", stride: Optional[int] = None) -> int:
    """An explicit stride wins; else min(crop_h, crop_w) (infer.py:64-65) under "uniform", and half of that under a
    window blend -- without overlap there is nothing to blend."""
    if stride is not None:
        return int(stride)
    return min(crop_h, crop_w) if blend == "uniform" else max(1, min(crop_h, crop_w) // 2)


def grid_size(src_hw: Tuple[int, int], size: Optional[Sequence[int]] = None, scale: Optional[float] = None):
    """Output grid of a scene: --size H W, else round(--scale * source size), else the source size."""
    if size is not None and scale is not None:
        raise ValueError("infer: --size and --scale are mutually exclusive")
    if size is not None:
        h, w = int(size[0]), int(size[1])
    elif scale is not None:
        if not scale > 0:
            raise ValueError(f"infer: --scale must be > 0, got {scale}")
        h, w = int(round(src_hw[0] * scale)), int(round(src_hw[1] * scale))
    else:
        h, w = int(src_hw[0]), int(src_hw[1])
    if h < 1 or w < 1:
        raise ValueError(f"infer: empty output grid {h}x{w}")
    return h, w


def crop_boxes(H: int, W: int, crop_h: int, crop_w: int, stride: int) -> List[Tuple[int, int, int, int]]:
    """(h0, w0, hE, wE) of get_crop_slices(H, W, crop_h, crop_w, (min(stride, H), min(stride, W)), "exact"), clipped to
    the grid."""
    from .datasets.tiles import get_crop_slices
    out = []
    for h0, w0, h, w in get_crop_slices(H, W, crop_h, crop_w, (min(stride, H), min(stride, W)), mode="exact"):
        out.append((h0, w0, min(h0 + h, H), min(w0 + w, W)))
    return out


def geo_tags_for_grid(tags: Dict[int, object], src_hw: Tuple[int, int], grid_hw: Tuple[int, int]):
    """GeoTIFF tags of a source raster -> (tag, type, values) triples for the same footprint on the output grid:
    GeoKey directory, doubles and ASCII verbatim; ModelPixelScale times source / grid size per axis; ModelTiepoint's raster
    point scaled with the grid (the usual (0, 0) stays), and under PixelIsPoint (GeoKey 1025 = 2) its world point moved by
    half the change in pixel size; ModelTransformation's linear part scaled (and its translation moved likewise under
    PixelIsPoint); GDAL_NODATA dropped -- it does not apply to a 0 / 255 mask."""
    fy, fx = src_hw[0] / grid_hw[0], src_hw[1] / grid_hw[1]
    keys = tags.get(34735)
    point = False
    if keys is not None and len(keys) >= 4:
        for i in range(int(keys[3])):
            k = keys[4 + 4 * i: 8 + 4 * i]
            if len(k) == 4 and k[0] == 1025 and k[1] == 0:
                point = k[3] == 2
    out = []
    scale = tags.get(33550)
    if scale is not None:
        sx, sy = scale[0], scale[1]
        out.append((33550, 12, [sx * fx, sy * fy] + list(scale[2:])))
        tie = tags.get(33922)
        if tie is not None:
            t = list(tie)
            for j in range(0, len(t) - 5, 6):
                t[j] /= fx
                t[j + 1] /= fy
                if point:
                    t[j + 3] += (sx * fx - sx) / 2
                    t[j + 4] -= (sy * fy - sy) / 2
            out.append((33922, 12, t))
    elif 33922 in tags:
        out.append((33922, 12, list(tags[33922])))
    mt = tags.get(34264)
    if mt is not None and len(mt) == 16:
        m = list(mt)
        for r in range(3):
            a, b = m[4 * r], m[4 * r + 1]
            m[4 * r], m[4 * r + 1] = a * fx, b * fy
            if point:
                m[4 * r + 3] += 0.5 * (a * fx - a) + 0.5 * (b * fy - b)
        out.append((34264, 12, m))
    if keys is not None:
        out.append((34735, 3, list(keys)))
    if 34736 in tags:
        out.append((34736, 12, list(tags[34736])))
    if 34737 in tags:
        out.append((34737, 2, tags[34737]))
    return out


def resident_grid(raster: torch.Tensor, scale_mode: int, grid_hw: Tuple[int, int], device) -> torch.Tensor:
    """Upload a band-selected raster fp32 [C, h, w] once and resample it once into the output grid fp32 [C, H, W] on the
    device: fu_resize_lanczos4_tiles with B = 1, the whole raster as the window and the whole grid as the tile, with the
    tables of lanczos4_axis_window (identity tables when the sizes match) and the sensor scaling training uses -- so
    every crop of the grid equals the tile TileLoader(device_resize=True) makes of it."""
    from .datasets.assemble import resize_lanczos4_tiles
    from .datasets.resize import lanczos4_axis_window
    dev = torch.device(device)
    H, W = grid_hw
    iy, wy, _ = lanczos4_axis_window(raster.shape[1], H, 0, H, H)
    ix, wx, _ = lanczos4_axis_window(raster.shape[2], W, 0, W, W)
    tabs = [torch.from_numpy(t)[None].to(dev, non_blocking=True) for t in (iy, wy, ix, wx)]
    return resize_lanczos4_tiles(raster[None].to(dev, non_blocking=True), *tabs, scale_mode)[0]


class SceneFiles(torch.utils.data.Dataset):
    """Scene i of the input list, decoded: {"raster": fp32 [C, h, w] after band selection, "scale_mode", "tags", "index"}."""

    def __init__(self, paths: Sequence[str], sensor: str, channels: str):
        self.paths, self.sensor, self.channels = list(paths), sensor, channels

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from .datasets.floodplanet import select_bands
        from .datasets.tiff import read_geotiff_tags, read_tiff
        raster, was_u16 = select_bands(read_tiff(self.paths[i]), self.sensor, self.channels)
        mode = SCALE_MODES.get(self.sensor, 4 if was_u16 else 0)
        return {"raster": torch.from_numpy(raster), "scale_mode": mode, "tags": read_geotiff_tags(self.paths[i]),
                "index": i}


def threshold_rule(water_threshold: Optional[float] = None, threshold_class: Optional[int] = None,
                   calibration: Optional[str] = None) -> Optional[dict]:
    """The decision rule the options ask for -> None (the argmax) or {"class", "threshold", "source"}.  Host only; raises
    on contradictory options: a threshold together with a calibration file, a class without a threshold."""
    from .calibration import check_threshold, read_calibration
    if calibration is not None:
        if water_threshold is not None or threshold_class is not None:
            raise ValueError("infer: --calibration already names the class and the threshold; it excludes "
                             "--water_threshold and --threshold_class")
        cls, thr = read_calibration(calibration)
        source = str(calibration)
    elif water_threshold is not None:
        cls, thr, source = (1 if threshold_class is None else threshold_class), water_threshold, "option"
    elif threshold_class is not None:
        raise ValueError("infer: --threshold_class needs --water_threshold")
    else:
        return None
    cls, thr = check_threshold(thr, cls)
    return {"class": cls, "threshold": thr, "source": source}


def check_model_inputs(cfg: dict, norm_params=None) -> None:
    """infer feeds the model ms_image only: reject configs whose model also takes dem / slope / ... (before any GPU work).
    norm_mode 'global' is accepted only together with its parameters."""
    kw = cfg["dataset"].get("dataset_kwargs") or {}
    extra = [k for k in EXTRA_SOURCES if kw.get(k)]
    if extra:
        raise NotImplementedError(f"infer feeds the model the ms_image input only; this model also takes {extra}")
    if cfg["norm_mode"] == "global" and norm_params is not None:
        return
    if cfg["norm_mode"] not in (None, "local"):
        raise NotImplementedError(f'infer: norm_mode "{cfg["norm_mode"]}" is not supported (None or "local")')


# ---------------------------------------------------------------------------------------------------------- infer
def infer(checkpoint_path: str, inputs: Sequence[str], out_dir: str, *, cfg: Optional[dict] = None,
          size: Optional[Sequence[int]] = None, scale: Optional[float] = None, stride: Optional[int] = None,
          batch_size: Optional[int] = None, tta=None, n_workers: int = 0, device: str = "cuda:0",
          keep_probabilities: bool = False, norm_params=None, weights: str = "auto", blend: str = "uniform",
          write_probs: Optional[str] = None, write_margin: bool = False, sieve: Optional[int] = None,
          sieve_connectivity: int = 4, sieve_passes: int = 1, water_threshold: Optional[float] = None,
          threshold_class: Optional[int] = None, calibration: Optional[str] = None) -> dict:
    """Class maps of every input scene (see the module docstring).  cfg: the resolved config (default: resolve_cfg of
    the checkpoint's experiment).  Returns the summary.json dict; with keep_probabilities also "probabilities"
    {output path: fp32 [H, W, k] stitched canvas} (one more host read per scene; for tests and comparisons).
    norm_params: the parameter file of norm_mode 'global' (path, or the dict it holds; datasets.stats), looked up by the
    config's data set name and sensor; without it a 'global' config is rejected.  weights: 'auto', 'raw' or 'ema'
    (predict.checkpoint_weights); the summary records the choice made under "weights".  blend: "uniform", "linear" or
    "hann" (stitch.blend_window); write_probs: None, "u8" or "f32"; write_margin: also write the top-2 margin raster.
    sieve: None, or the minimum patch size in pixels of the written class map (postprocess.sieve on the device, with
    sieve_connectivity 4 or 8 and sieve_passes 1..8); class_pixels and the other rasters stay un-sieved.
    water_threshold / threshold_class / calibration: the one-versus-rest decision rule (threshold_rule) in place of the
    argmax; the summary records it under "threshold"."""
    from .datasets.floodplanet import _N_CHANNELS
    from .models import build_model

    t_start = time.perf_counter()
    if weights not in WEIGHT_CHOICES:
        raise ValueError(f"weights must be one of {list(WEIGHT_CHOICES)}, got {weights!r}")
    if blend not in BLEND_KINDS:
        raise ValueError(f"blend must be one of {list(BLEND_KINDS)}, got {blend!r}")
    if write_probs is not None and write_probs not in PROB_FORMATS:
        raise ValueError(f"write_probs must be one of {list(PROB_FORMATS)} or None, got {write_probs!r}")
    rule = threshold_rule(water_threshold, threshold_class, calibration)
    sieve_opts = None
    if sieve is not None:
        check_sieve_options(sieve, sieve_connectivity, sieve_passes)
        sieve_opts = {"min_pixels": int(sieve), "connectivity": int(sieve_connectivity), "passes": int(sieve_passes)}
    if cfg is None:
        experiment_dir = "/".join(checkpoint_path.split("/")[:-2])
        cfg = resolve_cfg(experiment_dir, checkpoint_path)
    cfg = _merge(CONFIG_DEFAULTS, cfg)
    ds_cfg = cfg["dataset"]
    sensor, channels = ds_cfg["sensor"], ds_cfg.get("channels") or "ALL"
    norm_params = norm_params if norm_params is not None else cfg.get("norm_params")
    check_model_inputs(cfg, norm_params)
    try:
        n_channels = {"ms_image": _N_CHANNELS[sensor][channels]}
    except KeyError:
        raise NotImplementedError(f'Cannot get number of {sensor} channels for channel query "{channels}"') from None
    global_params = None
    if cfg["norm_mode"] == "global":                     # host only: a bad file fails before any GPU work
        from .datasets.stats import sensor_norm_params
        gm, gs = sensor_norm_params(norm_params, ds_cfg.get("name") or "floodplanet", sensor, n_channels["ms_image"])
        global_params = (torch.from_numpy(gm).float(), torch.from_numpy(gs).float())
    ch, cw = int(cfg["crop_height"]), int(cfg["crop_width"])
    stride = default_stride(ch, cw, blend, stride)
    if stride < 1:
        raise ValueError(f"infer: stride must be >= 1, got {stride}")
    bs = int(batch_size or cfg["batch_size"])
    codes = view_codes(tta, ch, cw) if tta is not None else None
    paths = find_inputs(inputs)
    outs = [output_path(out_dir, p, sensor) for p in paths]
    if len(set(outs)) != len(outs):
        dup = sorted({o for o in outs if outs.count(o) > 1})
        raise ValueError(f"infer: several inputs map to the same output {dup[:3]}")
    if size is not None or scale is not None:            # option errors before any GPU work
        grid_size((1 << 20, 1 << 20), size, scale)

    from .datasets.assemble import scene_crops
    from .postprocess import sieve as sieve_map
    from .stitch import GpuImageStitcher
    from .datasets.synthetic import write_strip_tiff
    dev = torch.device(device)
    model_kwargs = {k: v for k, v in (cfg["model"].get("model_kwargs") or {}).items()
                    if k not in ("ema_decay", "ema_warmup")}
    model = build_model(cfg["model"]["name"], n_channels, 3, cfg["lr"], log_image_iter=cfg["log_image_iter"],
                        to_rgb_fcn=None, ignore_index=cfg["ignore_index"], **model_kwargs)
    model, chosen = load_checkpoint_model(model, checkpoint_path, weights, in_channels=n_channels, n_classes=3,
                                          lr=cfg["lr"], **model_kwargs)
    model._set_model_to_eval()
    model = model.to(dev)
    net = model.model
    k = net.n_classes
    if rule is not None and rule["class"] >= k:
        raise ValueError(f"infer: threshold class {rule['class']} not in 0..{k - 1}")
    T = len(codes) if codes is not None else 1
    net._get_ctx(dev, T * bs, ch, cw)                    # the context owns fu_scene_crops' table: make it at full size
    stitcher = GpuImageStitcher(net, dev, blend=blend)
    class_values = [0] + [255] * (k - 1)                 # clip(argmax, 0, 1) * 255
    C = n_channels["ms_image"]
    crop_buf = torch.empty(bs, C, ch, cw, dtype=torch.float32, device=dev)
    loader = torch.utils.data.DataLoader(SceneFiles(paths, sensor, channels), batch_size=None, shuffle=False,
                                         num_workers=n_workers, pin_memory=dev.type == "cuda")
    scenes_it = iter(loader)
    resident: "OrderedDict[int, dict]" = OrderedDict()   # scene index -> grid, boxes, ...
    pending: List[Tuple[int, Tuple[int, int, int, int]]] = []   # crops not yet run: (scene, box)
    records, probabilities = [], {}
    n_crops = max_resident = 0
    exhausted = False

    def upload(item):
        i = int(item["index"])
        raster = item["raster"]
        src_hw = (raster.shape[1], raster.shape[2])
        H, W = grid_size(src_hw, size, scale)
        grid = resident_grid(raster, int(item["scale_mode"]), (H, W), dev)
        boxes = crop_boxes(H, W, ch, cw, stride)
        resident[i] = {"grid": grid, "hw": (H, W), "src_hw": src_hw, "tags": item["tags"], "left": len(boxes),
                       "n": len(boxes)}
        pending.extend((i, b) for b in boxes)

    def finalize(i):
        sc = resident.pop(i)
        H, W = sc["hw"]
        key = str(i)
        maps = stitcher.combine_maps(key, class_values, probs=write_probs == "u8", margin=write_margin, counts=True,
                                     threshold=None if rule is None else (rule["class"], rule["threshold"]))
        if sieve_opts is not None:                       # in place, on the stream of the launch above; no host read
            _, sieve_stats = sieve_map(maps["class"], sieve_opts["min_pixels"], sieve_opts["connectivity"],
                                       passes=sieve_opts["passes"], out=maps["class"])
        parts = [maps["counts"].view(torch.uint8), maps["class"].view(-1)]
        parts += [maps[m].view(-1) for m in ("probs", "margin") if m in maps]
        if write_probs == "f32":                         # the normalised canvas itself, as bytes of the same read
            parts.append(maps["canvas"].view(torch.uint8).view(-1))
        if sieve_opts is not None:
            parts.append(sieve_stats.view(torch.uint8))
        packed = torch.cat(parts).cpu().numpy()          # one launch above, the one device-to-host read here
        if keep_probabilities:
            probabilities[outs[i]] = maps["canvas"].cpu().numpy()
        stitcher.drop(key)
        class_pixels = packed[:8 * k].view(np.int64).tolist()
        at = 8 * k
        cls_h = packed[at:at + H * W].reshape(H, W)
        at += H * W
        tags = geo_tags_for_grid(sc["tags"], sc["src_hw"], (H, W))
        write_strip_tiff(outs[i], cls_h, extra_tags=tags)
        rec = {"input": paths[i], "output": outs[i], "source_size": list(sc["src_hw"]), "grid_size": [H, W],
               "crops": sc["n"], "class_pixels": class_pixels}
        if write_probs == "u8":
            rec["probabilities"] = side_output_path(outs[i], "prob")
            write_strip_tiff(rec["probabilities"], packed[at:at + k * H * W].reshape(k, H, W), extra_tags=tags)
            at += k * H * W
        if write_margin:
            rec["margin"] = side_output_path(outs[i], "margin")
            write_strip_tiff(rec["margin"], packed[at:at + H * W].reshape(H, W), extra_tags=tags)
            at += H * W
        if write_probs == "f32":
            rec["probabilities"] = side_output_path(outs[i], "prob")
            canvas_h = packed[at:at + 4 * k * H * W].view(np.float32).reshape(H, W, k)
            write_strip_tiff(rec["probabilities"], np.ascontiguousarray(canvas_h.transpose(2, 0, 1)), extra_tags=tags)
        if sieve_opts is not None:
            merged, changed = packed[-16:].view(np.int64).tolist()
            rec["sieve"] = dict(sieve_opts, merged_components=merged, changed_pixels=changed)
        records.append(rec)

    with torch.no_grad():
        while True:
            while len(pending) < bs and not exhausted:
                try:
                    upload(next(scenes_it))
                except StopIteration:
                    exhausted = True
                max_resident = max(max_resident, len(resident))
            if not pending:
                break
            batch, pending = pending[:bs], pending[bs:]
            n = len(batch)
            x, _, _ = scene_crops(net._ctx, [(resident[i]["grid"], b) for i, b in batch], (ch, cw), cfg["norm_mode"],
                                  global_params, out=crop_buf)
            probs = None
            if codes is None:
                net._forward_raw(model._gather_sources({"image": x}), False, want_logits=False)
            else:
                net.forward_views(model._gather_sources({"image": x}), codes)
                probs, _ = net.merge_views(None, want_probs=True)
            stitcher.add_images(range(n), [str(i) for i, _ in batch], [b for _, b in batch],
                                [resident[i]["hw"][0] for i, _ in batch], [resident[i]["hw"][1] for i, _ in batch],
                                probs=probs)
            n_crops += n
            for i, _ in batch:
                resident[i]["left"] -= 1
            for i in [i for i, sc in resident.items() if sc["left"] == 0]:
                finalize(i)

    seconds = time.perf_counter() - t_start
    summary = {"scenes": records, "n_scenes": len(records), "n_crops": n_crops, "seconds": seconds,
               "crops_per_s": n_crops / seconds if seconds > 0 else None, "max_resident_scenes": max_resident,
               "tta": tta if (tta is None or isinstance(tta, str)) else list(codes), "weights": chosen,
               "blend": blend, "stride": stride}
    if rule is not None:
        summary["threshold"] = rule
    if sieve_opts is not None:
        summary["sieve"] = dict(sieve_opts, merged_components=sum(r["sieve"]["merged_components"] for r in records),
                                changed_pixels=sum(r["sieve"]["changed_pixels"] for r in records))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "summary.json"), "w") as fh:
        json.dump(summary, fh, indent=4)
    if keep_probabilities:
        summary["probabilities"] = probabilities
    return summary


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Water class maps of unlabelled scenes (infer.py of st_water_seg).")
    ap.add_argument("checkpoint_path", type=str)
    ap.add_argument("inputs", nargs="+", help=".tif files or directories (searched recursively for *.tif)")
    ap.add_argument("--out_dir", type=str, required=True)
    grid = ap.add_mutually_exclusive_group()
    grid.add_argument("--size", type=int, nargs=2, metavar=("H", "W"), default=None,
                      help="output grid of every scene (default: the raster's own size)")
    grid.add_argument("--scale", type=float, default=None, help="output grid = round(F * the raster's size)")
    ap.add_argument("--stride", type=int, default=None,
                    help="crop stride (default: min(crop_height, crop_width); half of that with --blend linear / hann, "
                         "since without overlap there is nothing to blend)")
    ap.add_argument("--blend", type=str, default="uniform", choices=list(BLEND_KINDS),
                    help="how overlapping crops are averaged: equal weights (uniform, the default) or a window that "
                         "falls off towards the crop's border (linear: triangle, hann: raised cosine)")
    ap.add_argument("--write_probs", type=str, default=None, choices=list(PROB_FORMATS),
                    help="also write the stitched class probabilities as <image>_prob.tif, [k, H, W]: uint8 "
                         "rint(p * 255) (u8) or float32 (f32)")
    ap.add_argument("--write_margin", action="store_true",
                    help="also write <image>_margin.tif, uint8 [H, W]: rint(255 * (top-1 minus top-2 probability))")
    ap.add_argument("--sieve", type=int, default=None, metavar="N",
                    help="merge every connected patch of the class map smaller than N pixels into its largest neighbouring "
                         "patch, on the device (default: off).  Only the written class map is sieved: class_pixels, the "
                         "probability raster and the margin raster stay what the network said, un-sieved")
    ap.add_argument("--sieve_connectivity", type=int, default=4, choices=[4, 8],
                    help="neighbours that join pixels of one class into a patch (default 4)")
    ap.add_argument("--sieve_passes", type=int, default=1, choices=list(range(1, 9)),
                    help="apply the sieve this many times, each on the previous result (default 1)")
    ap.add_argument("--water_threshold", type=float, default=None, metavar="T",
                    help="declare the threshold class where its stitched probability is >= T (in [0, 1]), else the best of "
                         "the other classes, instead of the argmax (default: the argmax)")
    ap.add_argument("--threshold_class", type=int, default=None, metavar="C",
                    help="the class --water_threshold applies to (default 1, water)")
    ap.add_argument("--calibration", type=str, default=None, metavar="FILE",
                    help="take the class and its best-F1 threshold from a calibration.json written by predict --calibrate "
                         "(excludes --water_threshold / --threshold_class)")
    ap.add_argument("--batch_size", type=int, default=None, help="crops per eval forward (default: the config's)")
    ap.add_argument("--tta", type=str, default=None, choices=sorted(VIEW_SETS),
                    help="test-time augmentation: average each crop's softmax over its flips / rotations")
    ap.add_argument("--weights", type=str, default="auto", choices=list(WEIGHT_CHOICES),
                    help="which weights of the checkpoint to serve: state_dict (raw), weight EMA (ema) or the EMA when the "
                         "checkpoint has one (auto, the default)")
    ap.add_argument("--n_workers", type=int, default=0,
                    help="scene decoding worker processes (default 0: decode in-process, the faster setting measured)")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--norm_params", type=str, default=None,
                    help="parameter file of norm_mode 'global' (python -m floodplanet_code_amd.datasets.stats writes it)")
    return ap


def main(argv: Optional[List[str]] = None) -> None:
    args = build_parser().parse_args(argv)
    threshold_rule(args.water_threshold, args.threshold_class, args.calibration)   # option errors before anything is read
    experiment_dir = "/".join(args.checkpoint_path.split("/")[:-2])
    cfg = resolve_cfg(experiment_dir, args.checkpoint_path)
    out = infer(args.checkpoint_path, args.inputs, args.out_dir, cfg=cfg, size=args.size, scale=args.scale,
                stride=args.stride, batch_size=args.batch_size, tta=args.tta, n_workers=args.n_workers,
                device=args.device, norm_params=args.norm_params, weights=args.weights, blend=args.blend,
                write_probs=args.write_probs, write_margin=args.write_margin, sieve=args.sieve,
                sieve_connectivity=args.sieve_connectivity, sieve_passes=args.sieve_passes,
                water_threshold=args.water_threshold, threshold_class=args.threshold_class, calibration=args.calibration)
    print(json.dumps({k: v for k, v in out.items() if k != "scenes"}))


if __name__ == "__main__":
    main()
