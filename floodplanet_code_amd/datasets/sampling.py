"""Content-aware tile sampling and crop jitter for SceneTileLoader: which tiles an epoch trains on, and where they are cut.

Water is a small share of the valid pixels of most chips, and a tile whose labels are all ignored costs a full step for a
zero gradient.  The scenes are resident on the device, so a crop at any position costs what a grid crop costs.  Both remedies
need the label content of every candidate box, separately:

  * `label_box_counts` on the device: one table of boxes of resident uint8 label rasters, one launch
    (fu_label_box_counts; integer arithmetic, exact) -> int64 [n, 3], row i = the pixels of box i by raw label category:
    column 0 = raw neither 0 nor 2 (decodes to class 0), column 1 = raw 2 (decodes to class 1), column 2 = raw 0 (no data).
  * `label_box_counts_host`: the same contract in numpy -- the specification the tests compare the device against, NOT a
    fallback for the device call.
  * `tile_stats(counts, ignore_index, n_classes)`: (trainable, water) pixels per box under the loader's decode.
  * `plan_order(stats, tile_area, policy, ...)`: the epoch's order of data-set indices under "all", "labelled" (drop the
    tiles with nothing to train on) or "balanced" (a fixed share of tiles with water), and what was planned.
  * `jitter_boxes(boxes, raster_hw, J, seed, epoch)`: every box moved by its own offset in [-J, J]^2, kept inside its raster.
  * `TileOptions`: the loader's whole recipe -- these options, the radiometric config and the zoom range -- as one checked
    value, built by `make` (keywords), `from_args` (the fit command line) or `from_cfg` (a fit config).

Everything but `label_box_counts` is host arithmetic (numpy / torch CPU) and runs without a GPU."""
from __future__ import annotations

import dataclasses
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..augment import PHOTOMETRIC_KEYS, check_photometric
from .class_weights import Box, _check_host_entries, _device_table
from .scene_loader import epoch_order

__all__ = ["POLICIES", "label_box_counts", "label_box_counts_host", "tile_stats", "plan_order", "jitter_boxes", "zoom_boxes",
           "zoom_tile_host", "zoom_axis_host", "check_zoom_range", "TileOptions"]

POLICIES = ("all", "labelled", "balanced")
JITTER_STREAM = 0x6A177E2        # third word of the jitter stream's seed: a stream of its own, not the transforms'
ZOOM_STREAM = 0x200A5CA1         # ... and of the zoom stream's
PHOTOMETRIC_STREAM = 0x9A0705    # ... and of the radiometric draws'
ZOOM_LIMITS = (0.5, 2.0)         # bilinear resampling without a pre-filter aliases beyond this range
BALANCED_STREAM = 0xBA1A2CED     # mixed into the seed of the "balanced" draws


# ------------------------------------------------------------------------------------------------------- census
def label_box_counts_host(entries: Sequence[Tuple[np.ndarray, Box]]) -> np.ndarray:
    """entries: [(raw uint8 label raster [H, W], (h0, w0, hE, wE)), ...] -> int64 [n, 3]: row i = the pixels of box i that are
    (neither 0 nor 2, 2, 0).  Every entry is checked before anything is counted."""
    fn = "label_box_counts"
    if len(entries) < 1:
        raise ValueError(f"{fn}: no entries")
    checked = _check_host_entries(entries, fn)
    out = np.zeros((len(checked), 3), dtype=np.int64)
    for i, (label, (h0, w0, hE, wE)) in enumerate(checked):
        raw = np.bincount(label[h0:hE, w0:wE].reshape(-1), minlength=256)
        out[i] = (int(raw.sum() - raw[2] - raw[0]), int(raw[2]), int(raw[0]))
    return out


def label_box_counts(ctx, entries: Sequence[Tuple[torch.Tensor, Box]], counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C ABI fu_label_box_counts: entries = [(raw uint8 label raster [H, W] on the ROCm device, box), ...] -> int64 [n, 3] on
    that device, WRITTEN (rows of `counts` beyond n are left alone when it is given).  One launch for the whole table.
    ctx: the fu_ctx whose table buffer the call borrows (HipUNet._get_ctx)."""
    from .. import _lib
    fn = "label_box_counts"
    if ctx is None:
        raise ValueError(f"{fn}: no fu_ctx (run or prepare a forward first)")
    table, dev = _device_table(entries, fn)
    n = len(entries)
    if counts is None:
        counts = torch.empty((n, 3), dtype=torch.int64, device=dev)
    elif (counts.dtype != torch.int64 or counts.dim() != 2 or counts.shape[0] < n or counts.shape[1] != 3 or
          not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"{fn}: counts must be contiguous int64 [>= {n}, 3] on {dev}")
    _lib.check(_lib.load().fu_label_box_counts(ctx, n, table, counts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return counts


def _resolve_ignore(ignore_index: Optional[int], n_classes: int) -> Optional[int]:
    """The model's rule (balanced_class_weights): None ignores nothing, -1 means the last class."""
    if ignore_index is None:
        return None
    return n_classes - 1 if int(ignore_index) == -1 else int(ignore_index)


def tile_stats(counts, ignore_index: Optional[int], n_classes: int) -> Tuple[np.ndarray, np.ndarray]:
    """counts int64 [n, 3] (label_box_counts) -> (trainable, water), int64 [n] each.  Column 0 decodes to class 0, column 1
    to class 1, column 2 (no data) to `ignore_index`, the loader's nodata_value.  trainable = the columns whose decoded
    class lies in [0, n_classes) and is not the ignored class (None ignores nothing, -1 means the last class); water =
    column 1 unless class 1 is the ignored class."""
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[1] != 3 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"tile_stats: counts must be integer [n, 3], got {c.dtype} {c.shape}")
    n_classes = int(n_classes)
    if n_classes < 1:
        raise ValueError(f"tile_stats: n_classes = {n_classes} (must be >= 1)")
    ignored = _resolve_ignore(ignore_index, n_classes)
    decoded = (0, 1, ignored)                    # what columns 0, 1, 2 decode to
    c = c.astype(np.int64)
    trainable = np.zeros(c.shape[0], dtype=np.int64)
    for col, d in enumerate(decoded):
        if d is not None and 0 <= d < n_classes and d != ignored:
            trainable += c[:, col]
    water = c[:, 1].copy() if (1 < n_classes and ignored != 1) else np.zeros(c.shape[0], dtype=np.int64)
    return trainable, water


# ------------------------------------------------------------------------------------------------------- planner
def _check_frac(name: str, v: float) -> float:
    v = float(v)
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"{name} must lie in [0, 1], got {v}")
    return v


def _take(stratum: np.ndarray, k: int, g: torch.Generator) -> List[int]:
    """k items of the stratum from successive fresh permutations of it: every item once before any repeats."""
    out: List[int] = []
    while len(out) < k:
        perm = stratum[torch.randperm(len(stratum), generator=g).numpy()]
        out += perm[:k - len(out)].tolist()
    return out


def plan_order(stats, tile_area: int, policy: str, *, min_trainable_frac: float = 0.0, water_share: float = 0.5,
               min_water_frac: float = 0.0, shuffle: bool, seed: int, epoch: int) -> Tuple[List[int], dict]:
    """-> (order, info): the epoch's data-set indices and what was planned.

    stats: (trainable, water) of every example (tile_stats), or for "all" just the number of examples.
    "all": epoch_order(n, shuffle, seed, epoch).
    "labelled": kept = the examples with trainable >= 1 and trainable >= min_trainable_frac * tile_area, ascending; the
      order is kept[j] for j in epoch_order(len(kept), shuffle, seed, epoch) -- plan_epoch's own when nothing is dropped.
    "balanced": W = the kept examples with water >= 1 and water >= min_water_frac * tile_area, D = the other kept ones.
      The epoch has L = len(kept) picks, n_w = round(water_share * L) of them from W and L - n_w from D.  Within a stratum
      the picks come from successive fresh permutations of it, so multiplicities differ by at most 1.  With shuffle the L
      picks are permuted together; without, they are the water picks then the dry picks, each ascending.  An empty W or D
      degrades to "labelled" (info["degraded"]).  The draws come from one torch.Generator seeded from (seed, epoch).
    info: policy, n_examples, n_kept, n_dropped, n_water (picks from W; None without a census), water_share_planned
      (n_water / len(order)) and degraded.  Nothing kept raises ValueError."""
    if policy not in POLICIES:
        raise ValueError(f"tile_sampling must be one of {POLICIES}, got {policy!r}")
    min_trainable_frac = _check_frac("min_trainable_frac", min_trainable_frac)
    water_share = _check_frac("water_share", water_share)
    min_water_frac = _check_frac("min_water_frac", min_water_frac)
    info = {"policy": policy, "degraded": False}
    if policy == "all":
        n = int(stats) if np.ndim(stats) == 0 else len(stats[0])
        info.update(n_examples=n, n_kept=n, n_dropped=0, n_water=None, water_share_planned=None)
        return epoch_order(n, shuffle, seed, epoch), info
    trainable, water = (np.asarray(v, dtype=np.int64).reshape(-1) for v in stats)
    if trainable.shape != water.shape:
        raise ValueError(f"plan_order: {trainable.shape[0]} trainable counts, {water.shape[0]} water counts")
    n = trainable.shape[0]
    keep = (trainable >= 1) & (trainable >= min_trainable_frac * tile_area)
    kept = np.flatnonzero(keep)
    if kept.size == 0:
        raise ValueError(f"tile_sampling {policy!r}: none of the {n} tiles has a trainable pixel and at least "
                         f"min_trainable_frac = {min_trainable_frac} of the tile area ({tile_area} pixels) trainable")
    is_w = keep & (water >= 1) & (water >= min_water_frac * tile_area)
    W, D = np.flatnonzero(is_w), np.flatnonzero(keep & ~is_w)
    L = int(kept.size)
    info.update(n_examples=n, n_kept=L, n_dropped=n - L)
    if policy == "balanced" and (W.size == 0 or D.size == 0):
        info["degraded"] = True
    if policy == "labelled" or info["degraded"]:
        order = [int(kept[j]) for j in epoch_order(L, shuffle, seed, epoch)]
        n_w = int(W.size)
    else:
        g = torch.Generator().manual_seed((((int(seed) * 1000003 + int(epoch)) * 2654435761) % (1 << 62)) ^ BALANCED_STREAM)
        n_w = int(round(water_share * L))
        picks = sorted(_take(W, n_w, g)) + sorted(_take(D, L - n_w, g))
        order = [picks[j] for j in torch.randperm(L, generator=g).tolist()] if shuffle else picks
    info.update(n_water=n_w, water_share_planned=n_w / L)
    return order, info


# ------------------------------------------------------------------------------------------------------- jitter
def jitter_boxes(boxes: Sequence[Box], raster_hw: Sequence[Tuple[int, int]], J: int, seed: int, epoch: int) -> List[Box]:
    """Every box moved by its own integer offset (oy, ox), uniform in [-J, J], drawn for all examples in data-set order from
    RandomState([seed, epoch, JITTER_STREAM]) -- not the transforms' stream, so a run's transforms do not depend on J.
    h0' = clip(h0 + oy, 0, H - dh), w0' = clip(w0 + ox, 0, W - dw); the size is kept.  J = 0: the boxes, without drawing."""
    J = int(J)
    if J < 0:
        raise ValueError(f"crop_jitter must be >= 0, got {J}")
    boxes = [tuple(int(v) for v in b) for b in boxes]
    if len(raster_hw) != len(boxes):
        raise ValueError(f"jitter_boxes: {len(boxes)} boxes, {len(raster_hw)} raster sizes")
    if J == 0 or not boxes:
        return boxes
    rs = np.random.RandomState([int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, JITTER_STREAM])
    off = rs.randint(-J, J + 1, size=(len(boxes), 2))
    out = []
    for (h0, w0, hE, wE), (H, W), (oy, ox) in zip(boxes, raster_hw, off):
        dh, dw = hE - h0, wE - w0
        h0 = min(max(h0 + int(oy), 0), int(H) - dh)
        w0 = min(max(w0 + int(ox), 0), int(W) - dw)
        out.append((h0, w0, h0 + dh, w0 + dw))
    return out


# ------------------------------------------------------------------------------------------------------- zoom
def check_zoom_range(zoom_range) -> Tuple[float, float]:
    """(zmin, zmax) with 0 < zmin <= zmax, both inside ZOOM_LIMITS."""
    try:
        zmin, zmax = (float(v) for v in zoom_range)
    except (TypeError, ValueError):
        raise ValueError(f"zoom takes (zmin, zmax), got {zoom_range!r}") from None
    if not 0.0 < zmin <= zmax:
        raise ValueError(f"zoom needs 0 < zmin <= zmax, got ({zmin}, {zmax})")
    if zmin < ZOOM_LIMITS[0] or zmax > ZOOM_LIMITS[1]:
        raise ValueError(f"zoom ({zmin}, {zmax}) must stay within [{ZOOM_LIMITS[0]}, {ZOOM_LIMITS[1]}]: bilinear resampling "
                         f"without a pre-filter aliases beyond it")
    return zmin, zmax


def zoom_boxes(boxes: Sequence[Box], raster_shapes: Sequence[Tuple[int, int]], zoom_range, seed: int,
               epoch: int) -> Tuple[List[Box], List[Tuple[int, int]]]:
    """-> (source boxes, output sizes).  Every box gets its own factor z, log-uniform in [zmin, zmax] (z > 1 magnifies),
    drawn for all examples in data-set order from RandomState([seed, epoch, ZOOM_STREAM]).  Per axis the source size is
    clamp(round(d / z), 1, raster size); the source box keeps the box's centre (to the half pixel below) and is shifted to
    lie inside its raster.  The output size stays the box's own (dh, dw), so an edge tile keeps its valid region."""
    zmin, zmax = check_zoom_range(zoom_range)
    boxes = [tuple(int(v) for v in b) for b in boxes]
    if len(raster_shapes) != len(boxes):
        raise ValueError(f"zoom_boxes: {len(boxes)} boxes, {len(raster_shapes)} raster sizes")
    rs = np.random.RandomState([int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, ZOOM_STREAM])
    z = np.exp(rs.uniform(np.log(zmin), np.log(zmax), size=len(boxes)))
    src, out = [], []
    for (h0, w0, hE, wE), (H, W), zi in zip(boxes, raster_shapes, z):
        dh, dw = hE - h0, wE - w0
        sh = min(max(int(round(dh / zi)), 1), int(H))
        sw = min(max(int(round(dw / zi)), 1), int(W))
        a = min(max((h0 + hE - sh) // 2, 0), int(H) - sh)
        b = min(max((w0 + wE - sw) // 2, 0), int(W) - sw)
        src.append((a, b, a + sh, b + sw))
        out.append((dh, dw))
    return src, out


# ------------------------------------------------------------------------------------------------------- the recipe
FRACTIONS = ("min_trainable_frac", "water_share", "min_water_frac")
SAMPLING_KEYWORDS = ("tile_sampling",) + FRACTIONS + ("crop_jitter",)           # the keys of a config's `sampling`
PHOTOMETRIC_FLAGS = {"aug_" + k: k for k in PHOTOMETRIC_KEYS}                   # --aug_* flag -> photometric key


def _check_sampling(dash: str, tile_sampling, min_trainable_frac, water_share, min_water_frac, crop_jitter):
    """The five tile-sampling options checked, in TileOptions' field order; dash: "--" where they are named as flags."""
    if tile_sampling not in POLICIES:
        raise ValueError(f"{dash}tile_sampling must be one of {POLICIES}, got {tile_sampling!r}")
    fractions = [_check_frac(dash + k, v) for k, v in zip(FRACTIONS, (min_trainable_frac, water_share, min_water_frac))]
    if int(crop_jitter) < 0:
        raise ValueError(f"{dash}crop_jitter must be >= 0, got {crop_jitter}")
    return (tile_sampling, *fractions, int(crop_jitter))


def _photometric_items(photometric, spoken_as: str):
    """A photometric config checked (augment.check_photometric), as the tuple of items TileOptions keeps; None stays None."""
    if photometric is None:
        return None
    check_photometric(photometric, spoken_as)
    return tuple(dict(photometric).items())


@dataclasses.dataclass(frozen=True)
class TileOptions:
    """SceneTileLoader's sampling and augmentation recipe as one checked value; SceneTileLoader.__init__ says what each
    option does.  photometric_items holds the `photometric` config's items (read it as `photometric`, a dict of its own per
    read); `given` names the options a command line or a config stated, which is what a config records, and does not
    enter comparisons."""
    tile_sampling: str = "all"
    min_trainable_frac: float = 0.0
    water_share: float = 0.5
    min_water_frac: float = 0.0
    crop_jitter: int = 0
    photometric_items: Optional[Tuple[Tuple[str, Any], ...]] = None
    zoom: Optional[Tuple[float, float]] = None
    given: Tuple[str, ...] = dataclasses.field(default=(), compare=False)

    @classmethod
    def make(cls, *, tile_sampling="all", min_trainable_frac=0.0, water_share=0.5, min_water_frac=0.0, crop_jitter=0,
             photometric=None, zoom=None) -> "TileOptions":
        """The recipe checked, every check once (SceneTileLoader's keywords, in the order it checked them)."""
        sampling = _check_sampling("", tile_sampling, min_trainable_frac, water_share, min_water_frac, crop_jitter)
        zoom = None if zoom is None else check_zoom_range(zoom)
        return cls(*sampling, _photometric_items(photometric, "photometric"), zoom)

    @classmethod
    def from_args(cls, args) -> "TileOptions":
        """The recipe a fit command line gave: make's checks, with an option named as its flag, and between them, where fit
        always ran them, the rules that hold on the command line only -- the options belong to --loader scene, and
        --aug_likelihood alone varies nothing."""
        sampling = {k: getattr(args, k, None) for k in SAMPLING_KEYWORDS}
        sampling = {k: v for k, v in sampling.items() if v is not None}
        photometric = {key: getattr(args, flag, None) for flag, key in PHOTOMETRIC_FLAGS.items()}
        photometric = {k: float(v) for k, v in photometric.items() if v is not None}
        zoom = getattr(args, "aug_zoom", None)
        streaming = getattr(args, "loader", "scene") != "scene"
        if sampling and streaming:
            raise ValueError("--" + ", --".join(sampling) + " need --loader scene: the streaming loader cuts a fixed grid")
        checked = _check_sampling("--", **{**{k: getattr(cls, k) for k in SAMPLING_KEYWORDS}, **sampling})
        augmentation = ["aug_" + k for k in photometric] + (["aug_zoom"] if zoom is not None else [])
        if augmentation and streaming:
            raise ValueError("--" + ", --".join(augmentation) + " need --loader scene: the fused scene-tile kernel applies them")
        if set(photometric) == {"likelihood"}:
            raise ValueError("--aug_likelihood needs one of --aug_gain, --aug_band_gain, --aug_brightness, --aug_noise, "
                             "--aug_band_drop")
        given = tuple(sampling) + (("photometric",) if photometric else ()) + (("zoom",) if zoom is not None else ())
        return cls(*checked, _photometric_items(photometric or None, "--aug_*"),
                   None if zoom is None else check_zoom_range(zoom), given)

    @classmethod
    def from_cfg(cls, cfg: dict) -> "TileOptions":
        """The recipe a config records under `sampling` and `augmentation` (either may be absent)."""
        keywords = {**cfg.get("sampling", {}), **cfg.get("augmentation", {})}
        return dataclasses.replace(cls.make(**keywords), given=tuple(keywords))

    @property
    def photometric(self) -> Optional[dict]:
        return None if self.photometric_items is None else dict(self.photometric_items)

    def sampling_cfg(self) -> dict:
        """A config's `sampling`: the tile-sampling options that were given, {} for none."""
        return {k: getattr(self, k) for k in SAMPLING_KEYWORDS if k in self.given}

    def augmentation_cfg(self) -> dict:
        """A config's `augmentation`: `photometric` and `zoom` (a list) where given, {} for neither."""
        out = {"photometric": self.photometric} if "photometric" in self.given else {}
        if "zoom" in self.given:
            out["zoom"] = list(self.zoom)
        return out

    @property
    def needs_plan(self) -> bool:
        """Does an epoch need sampling's plan (its own boxes or order) rather than the grid's?"""
        return self.tile_sampling != "all" or self.crop_jitter > 0 or self.zoom is not None

    @property
    def needs_draws(self) -> bool:
        """Does an epoch draw per-example parameters (radiometric terms, zoomed source boxes)?"""
        return self.photometric_items is not None or self.zoom is not None


def zoom_axis_host(src: int, out: int):
    """One axis of the zoom of fu_scene_train_tiles_ex, for the pixels 0 .. out - 1 at once, in float32 with every operation
    rounded on its own: scale = src / out; c = (i + 0.5) * scale; f = max(c - 0.5, 0); i0 = min(floor(f), src - 1);
    i1 = min(i0 + 1, src - 1); w = f - i0; nearest = min(floor(c), src - 1).  -> (i0, i1, w float32, nearest)."""
    scale = np.float32(src) / np.float32(out)
    c = (np.arange(out, dtype=np.float32) + np.float32(0.5)) * scale
    f = np.maximum(c - np.float32(0.5), np.float32(0.0))
    i0 = np.minimum(np.floor(f).astype(np.int64), src - 1)
    i1 = np.minimum(i0 + 1, src - 1)
    w = f - i0.astype(np.float32)
    nearest = np.minimum(np.floor(c).astype(np.int64), src - 1)
    return i0, i1, w.astype(np.float32), nearest


def zoom_tile_host(image: Optional[np.ndarray], label: Optional[np.ndarray], out_hw: Tuple[int, int]):
    """The numpy statement of the zoom: image float32 [C, sh, sw] and / or raw label [sh, sw] -> (image [C, oh, ow], label
    [oh, ow]) (None where not given).  Half-pixel centres; the image is interpolated along x first, then along y, with
    lerp(p, q, w) = p + w * (q - p) in float32; the label takes the byte at `nearest` per axis (torch's 'nearest-exact').
    src == out returns the input's values.  This, not torch, is the definition the device is compared against."""
    oh, ow = int(out_hw[0]), int(out_hw[1])
    sh, sw = (image.shape[1:] if image is not None else label.shape)
    y0, y1, wy, ny = zoom_axis_host(int(sh), oh)
    x0, x1, wx, nx = zoom_axis_host(int(sw), ow)
    img = lab = None
    if image is not None:
        a = np.asarray(image, dtype=np.float32)
        rows = []
        for yy in (y0, y1):
            p, q = a[:, yy][:, :, x0], a[:, yy][:, :, x1]
            rows.append(p + wx[None, None, :] * (q - p))
        img = rows[0] + wy[None, :, None] * (rows[1] - rows[0])
        assert img.dtype == np.float32
    if label is not None:
        lab = np.asarray(label)[ny][:, nx]
    return img, lab
