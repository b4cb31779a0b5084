"""Training batches cut from scenes that live on the device.

TileLoader streams: DataLoader workers decode, cut windows and build tap tables per tile and per step, and the device then
runs three passes over each batch (resample, assemble, augment).  A FloodPlanet data set fits the card many times over, so
SceneTileLoader does what infer.py does for inference: every raster of the data set's example list is decoded ONCE, uploaded
once and resampled once to its label raster's grid (infer.resident_grid: a crop of that grid is the tile
TileLoader(device_resize=True) makes), the raw uint8 label raster is uploaded beside it, and from then on a batch is one
table of boxes and transforms and one fu_scene_train_tiles launch (two with norm_mode 'local') that crops, normalises, pads,
decodes the labels and applies hflip / vflip / rotate in a single pass.  No tensor enters or leaves the device per step.

What stays on the host: the epoch's order (plan_epoch), the draw of the transforms (augment.sample_transforms, the numpy
stream TileLoader uses) and the table itself.  Optionally the loader chooses which tiles an epoch sees and where they are
cut (tile_sampling, crop_jitter; datasets/sampling.py): the label content of every box comes from one
fu_label_box_counts launch over the resident label rasters, the plan is host arithmetic.  Optionally the same launch varies the
input as well (photometric, zoom: fu_scene_train_tiles_ex -- per-band gain, bias and noise, a per-sample resampling of a
smaller or larger source box); the host only draws the parameters.  These options are one checked value,
sampling.TileOptions, which the loader holds as `options` and reads nowhere else: a new one is a field and its check in
TileOptions.make, its flag in TileOptions.from_args and fit.build_parser, and the place below that acts on it.  What the
loader does not do: stream scenes in and out of HBM -- a data set that exceeds the residency budget raises
SceneResidencyError; TileLoader is the streaming loader."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

__all__ = ["SceneTileLoader", "SceneResidencyError", "epoch_order", "order_batches", "plan_epoch", "resident_bytes"]

FREE_MEMORY_FRACTION = 0.5       # default max_resident_bytes: this share of the device's free memory at construction


class SceneResidencyError(RuntimeError):
    """The data set's scenes do not fit the residency budget."""


# ------------------------------------------------------------------------------------------------------- epoch planner
def epoch_order(n_items: int, shuffle: bool, seed: int, epoch: int) -> List[int]:
    """Data-set order, or with shuffle the (epoch + 1)-th permutation a torch.Generator seeded with `seed` draws: a fresh
    permutation per epoch, the same for the same seed."""
    if not shuffle:
        return list(range(n_items))
    g = torch.Generator().manual_seed(int(seed))
    perm = None
    for _ in range(int(epoch) + 1):
        perm = torch.randperm(n_items, generator=g)
    return perm.tolist()


def order_batches(order: List[int], batch_size: int, drop_last: bool = False,
                  shard: Optional[Tuple[int, int]] = None) -> List[List[int]]:
    """An epoch's order (any list of data-set indices, repeats allowed) cut into batches.  shard = (rank, world): the rank's
    strided share of the order, cut to len(order) // world items so that every rank runs the same number of steps (the tail
    of fewer than `world` items is dropped)."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    if shard is not None:
        rank, world = int(shard[0]), int(shard[1])
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"shard = (rank, world) with 0 <= rank < world, got {tuple(shard)}")
        order = order[rank::world][:len(order) // world]
    batches = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
    if drop_last and batches and len(batches[-1]) < batch_size:
        batches.pop()
    return batches


def plan_epoch(n_items: int, batch_size: int, epoch: int = 0, shuffle: bool = False, seed: int = 0,
               drop_last: bool = False, shard: Optional[Tuple[int, int]] = None) -> List[List[int]]:
    """The batches (lists of data-set indices) of one epoch over every item: order_batches of epoch_order."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    return order_batches(epoch_order(n_items, shuffle, seed, epoch), batch_size, drop_last, shard)


# ------------------------------------------------------------------------------------------------------- residency
def _scene_list(dataset) -> List[Tuple[str, str, int, int]]:
    """(image path, label path, label height, label width) of every raster the example list names, in order of first use."""
    seen, out = set(), []
    for ex in dataset.dataset:
        if ex["image_path"] not in seen:
            seen.add(ex["image_path"])
            cp = ex["crop_params"]
            out.append((ex["image_path"], ex["label_path"], cp.og_height, cp.og_width))
    return out


def resident_bytes(dataset) -> int:
    """Device bytes the data set's scenes occupy once resident, from the TIFF headers alone: per scene the fp32 grid
    [C, label_h, label_w] and the uint8 label raster, plus the largest source raster (it is on the device only while its
    scene is resampled)."""
    from .geotiff import raster_size
    C = dataset.n_channels["ms_image"]
    total = transient = 0
    for image_path, _, H, W in _scene_list(dataset):
        total += C * H * W * 4 + H * W
        h, w = raster_size(image_path)
        transient = max(transient, C * h * w * 4)
    return total + transient


class _SceneRasters(torch.utils.data.Dataset):
    """Scene i decoded on the host: the band-selected raster (as infer.SceneFiles makes it) and the raw label raster."""

    def __init__(self, scenes, sensor: str, channels: str):
        self.scenes, self.sensor, self.channels = scenes, sensor, channels

    def __len__(self):
        return len(self.scenes)

    def __getitem__(self, i):
        from ..infer import SCALE_MODES
        from .floodplanet import read_image, select_bands
        image_path, label_path, H, W = self.scenes[i]
        raster, was_u16 = select_bands(read_image(image_path), self.sensor, self.channels)
        label = np.asarray(read_image(label_path))
        if label.shape != (H, W):
            raise ValueError(f"label raster {label_path} is {label.shape}, its header says {(H, W)}")
        if label.dtype != np.uint8:      # only 0 and 2 are told apart from the rest: keep exactly that
            label = np.where(label == 2, 2, np.where(label == 0, 0, 1)).astype(np.uint8)
        return {"raster": torch.from_numpy(raster), "label": torch.from_numpy(np.ascontiguousarray(label)),
                "scale_mode": SCALE_MODES.get(self.sensor, 4 if was_u16 else 0), "index": i}


# ------------------------------------------------------------------------------------------------------- loader
class SceneTileLoader:
    def __init__(self, dataset, batch_size: int, device, net, shuffle: bool = False, seed: int = 0, drop_last: bool = False,
                 transforms: Optional[dict] = None, ignore_index: int = 0, max_resident_bytes: Optional[int] = None,
                 shard: Optional[Sequence[int]] = None, num_workers: int = 0, tile_sampling: str = "all",
                 min_trainable_frac: float = 0.0, water_share: float = 0.5, min_water_frac: float = 0.0,
                 crop_jitter: int = 0, photometric: Optional[dict] = None, zoom: Optional[Sequence[float]] = None,
                 options=None):
        """dataset: FloodplanetTiles.  net: the HipUNet whose context owns the table's device buffer.  transforms: None, or
        the reference's `transforms` config dict ({} = its defaults), drawn from RandomState(seed) as TileLoader draws them.
        ignore_index: the fill of the target where the augmentation leaves the tile; the data set pads edge crops with its
        own ignore_index, and the kernel has one fill for both, so the two must agree.  max_resident_bytes: the budget of
        resident_bytes(dataset) (default: FREE_MEMORY_FRACTION of the device's free memory now).  num_workers: processes
        for the one-time decode.  options: the sampling and augmentation recipe as a sampling.TileOptions, in place of
        the seven keywords that follow (TileOptions.make checks them), not beside them; the loader reads `self.options` only:

        tile_sampling: "all" (every box of the grid once per epoch), "labelled" (only tiles with at least one pixel, and at
        least min_trainable_frac of the tile, that the loss does not ignore) or "balanced" (an epoch of as many tiles, a
        water_share of them tiles with at least one water pixel and min_water_frac of the tile water); sampling.plan_order
        states the policies.  crop_jitter = J > 0: every epoch moves every box by its own offset in [-J, J]^2, kept inside
        its raster (sampling.jitter_boxes).  With a policy other than "all" the label content of the epoch's boxes is
        counted at the start of the epoch (one fu_label_box_counts launch, one read of [n, 3] counts); without jitter the
        boxes never change, so it is counted once.  With the defaults nothing of this runs.  While an option is active,
        batches carry "boxes", the (h0, w0, hE, wE) actually cut (metadata keeps the grid's crop_params), and
        `last_plan` holds what the latest epoch planned.

        photometric: None, or augment.sample_photometric's config dict (gain, band_gain, brightness, noise, band_drop,
        likelihood; units of the normalised batch) -- gain, bias and noise applied by the batch's own launch
        (fu_scene_train_tiles_ex) to the pixels that come from the scene.  zoom = (zmin, zmax): every epoch every box is
        replaced by a source box 1 / z its size around the same centre, z log-uniform in the range, resampled to the box's
        own size in the same launch (sampling.zoom_boxes; bilinear image, nearest-exact labels).  Both draw for all examples
        in data-set order from RandomStates of their own, seeded with (seed, epoch, purpose): the stream of the transforms
        is consumed as before, and with both off every batch is what it was.  The noise of an example is keyed by
        noise_stream = epoch * len(dataset) + its index and a noise_key derived from `seed`.  Batches then carry
        "photometric" (the gain / bias / sigma rows, noise_key, noise_stream) and, with zoom, "src_boxes" (the boxes read)
        beside "boxes" (the boxes they stand for).  The tile-sampling census keeps counting the grid's (jittered) boxes,
        not the zoomed ones; under 'local' mean / std are those of the zoomed source box."""
        from .sampling import TileOptions
        self.dataset, self.batch_size, self.device = dataset, int(batch_size), torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SceneTileLoader keeps the scenes on a ROCm GPU and cuts the batches there; there is no CPU "
                               "fallback (TileLoader assembles on the host)")
        if int(dataset.ignore_index) != int(ignore_index):
            raise ValueError(f"SceneTileLoader: the data set pads targets with ignore_index {dataset.ignore_index} and the "
                             f"augmentation would fill with {ignore_index}; fu_scene_train_tiles has one fill for both")
        if not 0 <= int(ignore_index) <= 255:
            # the host path stores decoded labels as uint8: a no-data pixel would read ignore_index % 256 while the padding
            # and the augmentation fill read ignore_index itself -- two different "ignore" values in one batch
            raise ValueError(f"SceneTileLoader: ignore_index must lie in 0..255 (labels are decoded as uint8), got {ignore_index}")
        self.net, self.transforms, self.ignore_index = net, transforms, int(ignore_index)
        self.shuffle, self.seed, self.drop_last = bool(shuffle), int(seed), bool(drop_last)
        self.shard = None if shard is None else (int(shard[0]), int(shard[1]))
        self.num_workers = int(num_workers)
        stated = TileOptions.make(tile_sampling=tile_sampling, min_trainable_frac=min_trainable_frac, water_share=water_share,
                                  min_water_frac=min_water_frac, crop_jitter=crop_jitter, photometric=photometric,
                                  zoom=zoom)                                           # argument errors now
        if options is not None and not isinstance(options, TileOptions):
            raise TypeError(f"SceneTileLoader(): options must be a TileOptions, got {type(options).__name__}")
        if options is not None and stated != TileOptions():
            raise TypeError("SceneTileLoader(): options together with recipe keywords; give one or the other")
        self.options = stated if options is None else options
        self.noise_key = (self.seed * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & (2 ** 64 - 1)
        self._drawn = None               # (epoch, photometric draws, zoomed boxes) of the latest epoch
        self.last_plan = None            # what the latest planned epoch holds (sampling.plan_order's info)
        self._census = None              # (trainable, water) of the grid's boxes: cached, they never change
        self._planned = None             # (epoch, batches, boxes) of the latest plan
        plan_epoch(len(dataset), self.batch_size, 0, False, 0, self.drop_last, self.shard)       # argument errors now
        self.resident_bytes = resident_bytes(dataset)
        if max_resident_bytes is None:
            free, _ = torch.cuda.mem_get_info(self.device)
            max_resident_bytes = int(free * FREE_MEMORY_FRACTION)
        self.max_resident_bytes = int(max_resident_bytes)
        if self.resident_bytes > self.max_resident_bytes:
            raise SceneResidencyError(
                f"SceneTileLoader: the data set's {len(_scene_list(dataset))} scenes need {self.resident_bytes} bytes on the "
                f"device, more than max_resident_bytes = {self.max_resident_bytes}; nothing was uploaded. Use TileLoader, "
                f"which streams tiles from the host, for data sets that do not fit.")
        self._rng = np.random.RandomState(self.seed)
        self._epoch = 0
        self._items = None               # example i -> (grid, label, (h0, w0, hE, wE))
        self._global = None
        cp = dataset.dataset[0]["crop_params"] if len(dataset) else None
        self.tile_hw = (cp.max_crop_height, cp.max_crop_width) if cp is not None else None

    def __len__(self):
        """Batches per epoch; under a policy other than "all" the planned number for the next epoch (this takes the
        census, so the scenes become resident)."""
        if self.options.tile_sampling == "all":
            return len(plan_epoch(len(self.dataset), self.batch_size, 0, False, 0, self.drop_last, self.shard))
        return len(self._plan(self._epoch)[0])

    def _plan(self, epoch: int):
        """(batches, boxes) of an epoch under the sampling options: the epoch's boxes (jittered when crop_jitter > 0), their
        census unless the policy is "all" (every rank counts the whole split), the planned order, sharded and batched."""
        from . import sampling
        o = self.options
        if self._planned is not None and self._planned[0] == epoch:
            return self._planned[1:]
        if self._items is None:
            self._make_resident()
        boxes = [box for _, _, box in self._items]
        if o.crop_jitter > 0:
            boxes = sampling.jitter_boxes(boxes, [tuple(label.shape) for _, label, _ in self._items], o.crop_jitter,
                                          self.seed, epoch)
        th, tw = self.tile_hw
        stats = len(boxes)
        if o.tile_sampling != "all":
            stats = self._census
            if stats is None:
                ctx = self.net._get_ctx(self.device, self.batch_size, th, tw)
                counts = sampling.label_box_counts(ctx, [(label, box) for (_, label, _), box in zip(self._items, boxes)])
                stats = sampling.tile_stats(counts.cpu().numpy(), self.ignore_index, int(self.dataset.n_classes))
                if o.crop_jitter == 0:
                    self._census = stats
        order, info = sampling.plan_order(stats, th * tw, o.tile_sampling, min_trainable_frac=o.min_trainable_frac,
                                          water_share=o.water_share, min_water_frac=o.min_water_frac,
                                          shuffle=self.shuffle, seed=self.seed, epoch=epoch)
        batches = order_batches(order, self.batch_size, self.drop_last, self.shard)
        self._planned, self.last_plan = (epoch, batches, boxes), info
        return batches, boxes

    def _make_resident(self):
        """Decode, upload and resample every scene once; upload its label raster."""
        from ..infer import resident_grid
        ds, dev = self.dataset, self.device
        scenes = _scene_list(ds)
        loader = torch.utils.data.DataLoader(_SceneRasters(scenes, ds.sensor, ds.channels), batch_size=None, shuffle=False,
                                             num_workers=self.num_workers, pin_memory=True)
        store = {}
        for item in loader:
            image_path, _, H, W = scenes[int(item["index"])]
            grid = resident_grid(item["raster"], int(item["scale_mode"]), (H, W), dev)
            store[image_path] = (grid, item["label"].to(dev, non_blocking=True), H, W)
        items = []
        for ex in ds.dataset:
            grid, label, H, W = store[ex["image_path"]]
            cp = ex["crop_params"]
            items.append((grid, label, (cp.h0, cp.w0, min(cp.hE, H), min(cp.wE, W))))     # clipped, as the host's slicing clips
        if ds.norm_mode == "global":     # the kernel takes fp32 parameters: the fp64 ones are rounded once, as TileLoader does
            p = ds.global_norm_params[ds.sensor]
            self._global = (torch.from_numpy(p["mean"]).float().to(dev), torch.from_numpy(p["std"]).float().to(dev))
        torch.cuda.synchronize(dev)      # the pinned host rasters may go once the uploads are done
        self._items = items

    def class_counts(self) -> torch.Tensor:
        """Pixels per class over every example of the split: int64 [n_classes] on the device, from the resident label
        rasters -- one table of all the boxes, one launch (fu_label_class_counts).  Labels decode as the batches' targets
        do (no data -> ignore_index); overlapping tiles count as often as they are trained on.  A sharded loader still
        counts the whole split.  These are the frequencies of the grid's boxes: under tile_sampling "balanced" (tiles
        repeated or left out) or crop_jitter the frequencies trained on differ from them."""
        from .class_weights import label_class_counts
        if self._items is None:
            self._make_resident()
        n_classes = int(self.dataset.n_classes)
        if not self._items:
            return torch.zeros(n_classes, dtype=torch.int64, device=self.device)
        th, tw = self.tile_hw
        ctx = self.net._get_ctx(self.device, self.batch_size, th, tw)
        return label_class_counts(ctx, [(label, box) for _, label, box in self._items], self.ignore_index, n_classes)

    def _draws(self, epoch: int, boxes):
        """(photometric draws, (zoomed source boxes, output sizes)) of an epoch, for every example in data-set order, each
        from a RandomState of its own; None for an option that is off.  boxes: the epoch's boxes (zoom needs them)."""
        from .. import augment
        from . import sampling
        if self._drawn is not None and self._drawn[0] == epoch:
            return self._drawn[1:]
        photo = zoomed = None
        photometric, zoom = self.options.photometric, self.options.zoom
        if photometric is not None:
            rs = np.random.RandomState([self.seed & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, sampling.PHOTOMETRIC_STREAM])
            photo = augment.sample_photometric(len(self.dataset), self.dataset.n_channels["ms_image"], photometric, rs)
        if zoom is not None:
            zoomed = sampling.zoom_boxes(boxes, [tuple(label.shape) for _, label, _ in self._items], zoom, self.seed, epoch)
        self._drawn = (epoch, photo, zoomed)
        return photo, zoomed

    def _batch(self, index: List[int], boxes: Optional[List[Tuple[int, int, int, int]]] = None, epoch: int = 0) -> dict:
        from .. import augment
        from .assemble import scene_train_tiles
        n = len(index)
        photo, zoomed = self._draws(epoch, boxes) if self.options.needs_draws else (None, None)
        if self.transforms is not None:
            flags, angles = augment.sample_transforms(n, self.transforms, self._rng)
        else:
            flags, angles = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
        th, tw = self.tile_hw
        ctx = self.net._get_ctx(self.device, self.batch_size, th, tw)
        if boxes is None:
            entries = [self._items[i] + (int(flags[k]), float(angles[k])) for k, i in enumerate(index)]
        else:                            # the epoch's boxes (zoomed: the source boxes) in place of the grid's
            cut = boxes if zoomed is None else zoomed[0]
            entries = [self._items[i][:2] + (cut[i], int(flags[k]), float(angles[k])) for k, i in enumerate(index)]
        extra = {}
        if photo is not None:
            rows = np.asarray(index, dtype=np.int64)
            extra["photometric"] = {k: (None if v is None else np.ascontiguousarray(v[rows])) for k, v in photo.items()}
            extra["photometric"]["noise_key"] = self.noise_key
            extra["photometric"]["noise_stream"] = (int(epoch) * len(self.dataset) + rows).astype(np.uint64)
        if zoomed is not None:
            extra["zoom"] = ([zoomed[1][i][0] for i in index], [zoomed[1][i][1] for i in index])
        image, target, mean, std = scene_train_tiles(ctx, entries, (th, tw), self.dataset.norm_mode, self._global,
                                                     nodata_value=self.ignore_index,
                                                     target_fill=self.ignore_index, **extra)
        out = {"image": image, "target": target, "mean": mean, "std": std, "index": list(index), "flags": flags,
               "angles": angles}
        if boxes is not None:
            out["boxes"] = [boxes[i] for i in index]
        if photo is not None:
            out["photometric"] = extra["photometric"]
        if zoomed is not None:
            out["src_boxes"] = [zoomed[0][i] for i in index]
        if self.dataset.output_metadata:
            out["metadata"] = [{"image_path": ex["image_path"], "crop_params": ex["crop_params"],
                                "region_name": ex["region_name"]} for ex in (self.dataset.dataset[i] for i in index)]
        return out

    def __iter__(self):
        if self._items is None:
            self._make_resident()
        epoch, self._epoch = self._epoch, self._epoch + 1
        if self.options.needs_plan:
            batches, boxes = self._plan(epoch)
            for index in batches:
                yield self._batch(index, boxes, epoch)
            return
        for index in plan_epoch(len(self.dataset), self.batch_size, epoch, self.shuffle, self.seed, self.drop_last,
                                self.shard):
            yield self._batch(index, None, epoch)
