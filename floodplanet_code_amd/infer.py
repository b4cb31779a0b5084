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
    rescaled to the output grid (geo_tags_for_grid); the input's GDAL_NODATA does not go along (it does not describe a
    0 / 255 mask) -- with --nodata the class map carries one of its own, see below;
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
  * extension: --nodata auto|V makes the run aware of pixels that hold no data (swath edges, collars, fill).  The rule is
    datasets/valid_mask.py's: a source pixel is valid when every band is finite and not every band equals V (auto: the
    scene's GDAL_NODATA tag when it parses as a finite number, else 0), a grid pixel when nothing it was resampled from
    was fill.  The mask is derived on the device from the uploaded scene (fu_scene_valid_mask), next to the resample and
    from the same upload and tables.  Where it is 0 the class map is --nodata_out N (default 127) instead of 0 / 255, the
    probability and margin rasters are 0, the pixel is not counted in class_pixels and, under --sieve, is neither merged
    nor a donor (frozen_value) -- all inside the one finalisation launch (fu_stitch_finalize_maps_masked).  The class map
    carries GDAL_NODATA = "N" (tag 42113); the probability and margin rasters carry none, 0 is a value there.  Crops
    without a single valid pixel are not forwarded (one census launch per scene, fu_mask_box_counts, and one small read;
    --keep_empty_crops forwards them): a valid pixel lies only in boxes that contain it, so it loses no covering crop and
    its sequence of stitch additions does not change.  A scene without any valid pixel never enters a batch and is
    written as all N.  --write_valid writes the mask as <image>_valid.tif (uint8 0 / 1).  The records gain
    "valid_pixels", "skipped_crops" and "nodata" (the value used), "crops" counts the crops forwarded, and the summary
    gains "nodata".  Not part of it: norm_mode 'local' still takes a crop's statistics over all its pixels, fill included,
    exactly as without the option, so a valid pixel's probabilities are the same with and without --nodata; the
    resampling is not mask-aware; predict (labelled evaluation) and training are not touched.  Without --nodata nothing
    of this runs and every file is byte for byte what it was.
  * extension: scenes need not be classic uncompressed strip TIFFs.  datasets/geotiff.py reads classic and BigTIFF, strips
    and tiles, Deflate / LZW / PackBits, predictors 2 and 3, and with them the georeferencing and GDAL_NODATA of a BigTIFF
    scene.  --decode auto|host|device (InferOptions.decode) says where the samples are unpacked: under auto, the default, a
    file the strict reader takes goes exactly the way it always went -- nothing new runs, every output byte is what it
    was -- and every other file is entropy-decoded on the host (--decode_threads threads, default 4) and its bytes are
    uploaded as stored and unpacked by ONE kernel launch (fu_tiff_unpack: predictor, byte swap, tiles, band choice,
    conversion) into the very fp32 tensor the host route uploads; device does so for every file, host puts every file
    through the numpy statement.  Everything behind that tensor is the same code, so the routes write identical files.
    Out of scope: JPEG / ZSTD / LERC, sub-byte samples, reading a scene from an overview or a mask IFD (the first IFD is the
    scene; geotiff.read_raster(ifd=...) reads the others), entropy decoding on the GPU.
  * extension: --write_vectors writes the water bodies as polygons, <image>.geojson beside <image>.tif: one Polygon
    feature, outer ring and holes, per connected patch (--vector_connectivity 4|8, default the sieve's, else 4) of the
    values --vector_values (default 255) of the class map as written, so after the threshold, the mask and the sieve.
    vectorize.py holds the rule.  On the device, between the sieve and the scene's one large read: components
    (fu_map_components), the pixel edges between unlike pixels and their device-wide scan (fu_map_edge_offsets), one
    4-byte read of the edge count, each edge's successor and the rings by pointer jumping (fu_map_edge_rings); the five
    int32 arrays per edge ride in that read, and the host sorts them into rings, keeps the corners and writes.  The
    properties are value, label, pixels, area (pixels times the pixel area in CRS units, null without georeferencing)
    and bbox_px; coordinates stay in the raster's CRS (no reprojection) and an EPSG code in the GeoKeys becomes the "crs"
    member.  A scene with more than --vector_max_edges edges (default 2^24) gets "vectors": {"skipped"} in its record
    and no file; a scene without a selected pixel, or without a crop under --nodata, an empty FeatureCollection.  The
    records and the summary gain "vectors".  Without --write_vectors nothing of this runs and every file is byte for
    byte what it was.  Out of scope: simplification and smoothing, MultiPolygons by value, Shapefile / GeoPackage,
    vectors in predict.
  * extension: the rasters need not be classic uncompressed strip TIFFs either.  --out_compress deflate [--out_level 1..9]
    [--out_predictor auto|off], --out_tile [N], --out_bigtiff auto|yes|no and --out_threads T choose Deflate (zlib, per
    segment, on a pool of T threads, default 4), the predictor (auto: horizontal differencing for the uint8 rasters, the
    floating-point predictor for fp32), N x N tiles (N a multiple of 16, 256 when the flag stands alone) instead of 16-row
    strips, and BigTIFF (auto: only where classic TIFF cannot hold the file).  datasets/geotiff_write.py holds the byte
    layout (pack_host) and the container (write_raster).  With any of them set, what happens to the samples ahead of the
    entropy coder -- planes, tiles, edge padding by replication, the predictor -- happens on the device, one launch per
    raster (fu_tiff_pack, the inverse of fu_tiff_unpack) on the same stream after the sieve: the class map as written,
    "probs", "margin", "valid" and the fp32 canvas straight from its [H, W, k] strides (no host transpose), and the packed
    buffers ride in the scene's one read in place of the tensors (the one-byte class map rides along when
    --write_vectors needs it on the host).  The host deflates segments and writes the container, with the georeferencing
    and the class map's GDAL_NODATA as always; a scene without a valid pixel is packed on the host (pack_host).  The
    records and the summary gain "output_format".  With every out_* option at its default nothing of this runs and every
    file is byte for byte what it was -- except that a file classic TIFF cannot hold (above 4 GiB; that only raised) is
    written as BigTIFF strips by the new writer.  Out of scope: LZW / PackBits / ZSTD encoders, chunky or big-endian
    output, predict's outputs, entropy coding on the GPU.
  * extension: --out_overviews auto|N puts N reduced-resolution images behind every written raster, and --out_cog is the
    preset for cloud-optimised files (tiles of 512 and overviews "auto" unless given).  The levels are cut on the device,
    after the sieve and from the rasters as they are written (datasets/overviews.py holds the rule; fu_map_overviews, six
    levels per launch from one read of the raster): the class map by its most frequent value (ties to the smaller value,
    nodata_out never wins under --nodata), probabilities, margin and the fp32 canvas by the mean over the valid pixels, the
    valid raster by `any`.  Each level goes through fu_tiff_pack with a layout of its own size and rides in the scene's one
    read; write_raster puts every directory in front of the data and the smallest image's data first.  Such a run is a
    packed-output run; the records' "output_format" gains "overviews" and "cog" (geotiff.cog_report of the written files).
    Without either flag nothing of this runs.  Out of scope: GDAL's ghost block and tile leaders, overviews of predict's
    outputs, other resampling kinds, reading a scene from an overview under --scale.
How infer() is put together: the options travel as one checked InferOptions (infer_options.py; the keywords of infer() and
the command line both go through InferOptions.make); predict.load_eval_model serves the model; a SceneQueue owns the
scenes in flight and deals their crops out in batches; per batch scene_crops, predict.eval_forward and one batched stitch;
per finished scene finalize_scene (the launches and the one read, stitch.PackedRead) and write_scene (host only).
Out of scope: multi-GPU inference, inputs besides ms_image (dem, slope, hand, preflood), RGB outputs.
"""
from __future__ import annotations

import argparse
import functools
import json
import os
import time
from collections import OrderedDict
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .infer_options import (BLEND_KINDS, DECODE_CHOICES, DECODE_THREADS_DEFAULT, NODATA_OUT_DEFAULT,  # noqa: F401
                            OUT_BIGTIFF_CHOICES, OUT_COMPRESS_CHOICES, OUT_LEVEL_DEFAULT, OUT_PREDICTOR_CHOICES,
                            OUT_THREADS_DEFAULT, OUT_TILE_FLAG, OUT_TILE_STRIPS, PROB_FORMATS, WEIGHT_CHOICES, InferOptions,
                            default_stride, grid_size, scene_nodata, threshold_rule)
from .predict import CONFIG_DEFAULTS, _merge, eval_forward, load_eval_model, resolve_cfg
from .tta import VIEW_SETS, recorded
from .vectorize import ARRAYS as VECTOR_ARRAYS

SCALE_MODES = {"S1": 1, "S2": 2, "L8": 3}                    # PS: 4 when stored as uint16, else 0
EXTRA_SOURCES = ("dem", "slope", "preflood", "pre_post_difference", "chirps", "hand")


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
    PixelIsPoint); the source's GDAL_NODATA is not copied -- it does not apply to a 0 / 255 mask (write_scene adds the
    class map's own under --nodata)."""
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
    source, tabs = upload_source(raster, grid_hw, device)
    return resize_lanczos4_tiles(source[None], *tabs, scale_mode)[0]


def upload_source(raster, grid_hw: Tuple[int, int], device):
    """The one upload of a scene -> (the raster fp32 [C, h, w] on the device, the four tap tables of
    lanczos4_axis_window for the whole grid, each with resize_lanczos4_tiles' leading 1).  Both the resample and the
    valid mask are taken from these.  raster: the band-selected fp32 tensor, or the encoded item of SceneFiles
    ({"encoded", "layout", "bands"}): its bytes are uploaded as stored and unpacked there (geotiff.unpack_on_device, one
    launch) into the same tensor."""
    from .datasets import geotiff
    from .datasets.resize import lanczos4_axis_window
    dev = torch.device(device)
    H, W = grid_hw
    encoded = isinstance(raster, dict)
    h, w = (int(raster["layout"]["height"]), int(raster["layout"]["width"])) if encoded else raster.shape[1:]
    iy, wy, _ = lanczos4_axis_window(h, H, 0, H, H)
    ix, wx, _ = lanczos4_axis_window(w, W, 0, W, W)
    tabs = [torch.from_numpy(t)[None].to(dev, non_blocking=True) for t in (iy, wy, ix, wx)]
    if encoded:
        return geotiff.unpack_on_device(raster["encoded"], raster["layout"], raster["bands"], dev), tabs
    return raster.to(dev, non_blocking=True), tabs


class SceneFiles(torch.utils.data.Dataset):
    """Scene i of the input list, decoded: {"raster": fp32 [C, h, w] after band selection, "scale_mode", "tags", "index"},
    or, on the device route, entropy-decoded only: {"encoded": uint8 [n] (geotiff.read_raster_encoded), "layout", "bands"
    (select_band_indices), "scale_mode", "tags", "index"} -- the host neither widens, transposes nor selects.  decode:
    "auto" -- a file the strict reader takes (classic, strips, uncompressed) gives the first item through that reader, as
    always, every other file the second; "host" -- the first item for every file, through geotiff.read_raster; "device" --
    the second for every file."""

    def __init__(self, paths: Sequence[str], sensor: str, channels: str, decode: str = "auto", decode_threads: int = 4):
        from .infer_options import check_decode
        self.paths, self.sensor, self.channels = list(paths), sensor, channels
        self.decode, self.decode_threads = check_decode(decode, decode_threads)

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from .datasets import geotiff
        from .datasets.floodplanet import select_band_indices, select_bands
        from .datasets.tiff import read_tiff
        path = self.paths[i]
        tags = geotiff.raster_geotiff_tags(path)
        route = self.decode
        if route == "auto":
            route = "strict" if geotiff.strict_reader_accepts(path) else "device"
        if route == "device":
            encoded, layout = geotiff.read_raster_encoded(path, self.decode_threads)
            h, w, n = layout["height"], layout["width"], layout["samples"]
            shape, axis = ((h, w), 0) if n == 1 else ((n, h, w), 0) if layout["planar"] else ((h, w, n), 2)
            bands = select_band_indices(shape, axis, self.sensor, self.channels)
            was_u16 = layout["sample_kind"] == 1 and layout["bytes_per_sample"] == 2
            mode = SCALE_MODES.get(self.sensor, 4 if was_u16 else 0)
            return {"encoded": torch.from_numpy(encoded), "layout": layout, "bands": bands, "scale_mode": mode,
                    "tags": tags, "index": i}
        image = read_tiff(path) if route == "strict" else geotiff.read_raster(path, self.decode_threads)
        raster, was_u16 = select_bands(image, self.sensor, self.channels)
        mode = SCALE_MODES.get(self.sensor, 4 if was_u16 else 0)
        return {"raster": torch.from_numpy(raster), "scale_mode": mode, "tags": tags, "index": i}


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
def model_inputs(cfg: dict, norm_params=None):
    """What the config's model is fed -> (sensor, channels, {"ms_image": C}, the 'global' norm's (mean, std) or None).
    Host only: an unsupported model or a bad parameter file fails here, before any GPU work."""
    from .datasets.floodplanet import _N_CHANNELS
    ds_cfg = cfg["dataset"]
    sensor, channels = ds_cfg["sensor"], ds_cfg.get("channels") or "ALL"
    norm_params = norm_params if norm_params is not None else cfg.get("norm_params")
    check_model_inputs(cfg, norm_params)
    try:
        n_channels = {"ms_image": _N_CHANNELS[sensor][channels]}
    except KeyError:
        raise NotImplementedError(f'Cannot get number of {sensor} channels for channel query "{channels}"') from None
    global_params = None
    if cfg["norm_mode"] == "global":
        from .datasets.stats import sensor_norm_params
        gm, gs = sensor_norm_params(norm_params, ds_cfg.get("name") or "floodplanet", sensor, n_channels["ms_image"])
        global_params = (torch.from_numpy(gm).float(), torch.from_numpy(gs).float())
    return sensor, channels, n_channels, global_params


def scene_outputs(inputs: Sequence[str], out_dir: str, sensor: str) -> Tuple[List[str], List[str]]:
    """-> (the input scenes, their class maps' paths); two inputs may not share an output."""
    paths = find_inputs(inputs)
    outs = [output_path(out_dir, p, sensor) for p in paths]
    if len(set(outs)) != len(outs):
        dup = sorted({o for o in outs if outs.count(o) > 1})
        raise ValueError(f"infer: several inputs map to the same output {dup[:3]}")
    return paths, outs


def upload_scene(item: dict, options: InferOptions, crop_hw: Tuple[int, int], device, ctx=None):
    """A decoded scene (SceneFiles, either item) -> (its index, the scene as it stays resident: its grid on the device,
    sizes, tags and crop count, its crop boxes).  With options.nodata the scene also holds "valid" (uint8 [H, W] on the device),
    "n_valid" (int64 [1] there), "nodata" (the value used) and "skipped"; with skip_empty only the boxes with at least one
    valid pixel are returned (one census launch through ctx, a zero-argument callable that gives the fu_ctx, and one
    small read).  A scene left without a box keeps nothing on the device."""
    from .datasets.assemble import resize_lanczos4_tiles
    if "encoded" in item:                                # the device route: upload_source unpacks the bytes there
        raster = item
        src_hw = (int(item["layout"]["height"]), int(item["layout"]["width"]))
    else:
        raster = item["raster"]
        src_hw = (raster.shape[1], raster.shape[2])
    H, W = options.grid(src_hw)
    source, tabs = upload_source(raster, (H, W), device)
    grid = resize_lanczos4_tiles(source[None], *tabs, int(item["scale_mode"]))[0]
    boxes = crop_boxes(H, W, crop_hw[0], crop_hw[1], options.stride)
    scene = {"grid": grid, "hw": (H, W), "src_hw": src_hw, "tags": item["tags"], "n": len(boxes)}
    if options.nodata is not None:
        from .datasets.valid_mask import box_valid_counts, scene_valid_mask
        value = scene_nodata(options.nodata, item["tags"])
        valid, n_valid = scene_valid_mask(source, value, tabs)
        scene.update(valid=valid, n_valid=n_valid, nodata=value, skipped=0)
        if options.skip_empty:
            counts = box_valid_counts(ctx(), valid, boxes).cpu().tolist()
            boxes = [b for b, c in zip(boxes, counts) if c > 0]
            scene.update(skipped=scene["n"] - len(boxes), n=len(boxes))
            if not boxes:
                scene.update(grid=None, valid=None, n_valid=None)
    return int(item["index"]), scene, boxes


class SceneQueue:
    """The scenes in flight and their crops that have not run yet.  scenes: an iterable of decoded scenes; upload(scene)
    -> (scene index, what stays resident of it, its crop boxes).  batches() yields lists of up to batch_size
    (scene index, box), in scene order and then box order, and uploads the next scene only while fewer than batch_size
    crops are pending; after a batch is stitched, stitched(batch) hands out the scenes it completed, in scene order,
    and forgets them.  resident: scene index -> the uploaded scene; max_resident: the most there were at once.
    A scene whose box list is empty (all fill: it holds nothing on the device) never enters resident or a batch: it waits
    in scene order -- uploads come in increasing scene index -- and stitched() hands it out as completed once no earlier
    scene is in flight; after the last batch, stitched(()) hands out those that came behind the last crop."""

    def __init__(self, scenes: Iterable, upload: Callable, batch_size: int):
        self._scenes, self._upload, self._batch_size = iter(scenes), upload, int(batch_size)
        self.resident: "OrderedDict[int, object]" = OrderedDict()
        self.max_resident = 0
        self._left: Dict[int, int] = {}                  # scene index -> crops not yet stitched
        self._pending: List[Tuple[int, tuple]] = []      # crops not yet run: (scene index, box)
        self._empty: List[Tuple[int, object]] = []       # scenes without a box, not handed out yet
        self._exhausted = False

    def batches(self) -> Iterator[List[Tuple[int, tuple]]]:
        while True:
            while len(self._pending) < self._batch_size and not self._exhausted:
                try:
                    i, scene, boxes = self._upload(next(self._scenes))
                    if not boxes:
                        self._empty.append((i, scene))
                        continue
                    self.resident[i], self._left[i] = scene, len(boxes)
                    self._pending.extend((i, b) for b in boxes)
                except StopIteration:
                    self._exhausted = True
                self.max_resident = max(self.max_resident, len(self.resident))
            if not self._pending:
                return
            batch, self._pending = self._pending[:self._batch_size], self._pending[self._batch_size:]
            yield batch

    def stitched(self, batch: Sequence[Tuple[int, tuple]]) -> List[Tuple[int, object]]:
        for i, _ in batch:
            self._left[i] -= 1
        done = [i for i in self.resident if self._left[i] == 0]
        for i in done:
            del self._left[i]
        out = [(i, self.resident.pop(i)) for i in done]
        while self._empty and all(self._empty[0][0] < i for i in self.resident):
            out.append(self._empty.pop(0))
        return sorted(out, key=lambda t: t[0])


def empty_scene_arrays(scene: dict, n_classes: int, options: InferOptions) -> Dict[str, np.ndarray]:
    """finalize_scene's arrays for a scene without a valid pixel, which never had a canvas: the class map all
    nodata_out, zero side rasters, zero counts.  Host only."""
    H, W = scene["hw"]
    arrays = {"counts": np.zeros(n_classes, dtype=np.int64), "class": np.full((H, W), options.nodata_out, dtype=np.uint8),
              "n_valid": np.zeros(1, dtype=np.int64)}
    if options.write_probs == "u8":
        arrays["probs"] = np.zeros((n_classes, H, W), dtype=np.uint8)
    if options.write_margin:
        arrays["margin"] = np.zeros((H, W), dtype=np.uint8)
    if options.write_probs == "f32":
        arrays["canvas"] = np.zeros((H, W, n_classes), dtype=np.float32)
    if options.sieve is not None:
        arrays["sieve"] = np.zeros(2, dtype=np.int64)
    if options.write_valid:
        arrays["valid"] = np.zeros((H, W), dtype=np.uint8)
    if options.keep_probabilities:
        arrays["kept"] = np.zeros((H, W, n_classes), dtype=np.float32)
    if options.write_vectors:
        arrays.update({k: np.zeros(0, dtype=np.int32) for k in VECTOR_ARRAYS}, edges=0)      # no crop: no polygon
    if options.packed_output:                            # what finalize_scene packs on the device, here on the host
        from .datasets.geotiff_write import pack_host
        for name in PACKED_RASTERS:
            if name in arrays:
                raster = arrays[name].transpose(2, 0, 1) if name == "canvas" else arrays[name]
                arrays["packed_" + name] = pack_host(raster, output_layout(options, raster.dtype, raster.shape))
                levels = raster_overviews(raster, name, options, np.zeros((H, W), dtype=np.uint8))
                for l, level in enumerate(levels, 1):
                    arrays[f"packed_{name}_ov{l}"] = pack_host(level, output_layout(options, level.dtype, level.shape))
                if name != "class" or not options.write_vectors:
                    del arrays[name]
    return arrays


PACKED_RASTERS = ("class", "probs", "margin", "valid", "canvas")     # the arrays of finalize_scene that become files
# how each of them is reduced to its overview levels (datasets/overviews.py)
OVERVIEW_KINDS = {"class": "mode_u8", "probs": "mean_u8", "margin": "mean_u8", "valid": "any_u8", "canvas": "mean_f32"}


def raster_overviews(raster, name: str, options: InferOptions, valid) -> list:
    """The overview levels of one output raster ([H, W] or [k, H, W]; a device tensor goes through fu_map_overviews, an
    array through the numpy statement), options.overview_levels of them: the class map by mode_u8 with nodata_out as the
    nodata value under --nodata, probabilities and margin by mean_u8 and the fp32 canvas by mean_f32 over the scene's valid
    mask (valid: uint8 [H, W], looked at under --nodata only), the valid raster by any_u8."""
    from .datasets.overviews import overviews_host, overviews_on_device
    n_levels = options.overview_levels(tuple(raster.shape[-2:]))
    if n_levels == 0:
        return []
    reduce = overviews_on_device if torch.is_tensor(raster) else overviews_host
    kind, masked = OVERVIEW_KINDS[name], options.nodata is not None
    if kind == "mode_u8":
        return reduce(raster, kind, n_levels, nodata_value=options.nodata_out if masked else None)
    if kind == "any_u8":
        return reduce(raster, kind, n_levels)
    return reduce(raster, kind, n_levels, valid=valid if masked else None)[0]


def output_layout(options: InferOptions, dtype, shape) -> dict:
    """The byte layout (fu_tiff_layout dict) of an output raster [H, W] or [k, H, W] under the out_* options: out_tile x
    out_tile tiles or 16-row strips, the predictor of options.predictor_for."""
    from .datasets.geotiff_write import raster_layout
    samples, (H, W) = (1 if len(shape) == 2 else int(shape[0])), shape[-2:]
    return raster_layout(dtype, int(H), int(W), samples, tile=options.out_tile, predictor=options.predictor_for(dtype))


def finalize_scene(stitcher, key: str, class_values: Sequence[int], options: InferOptions,
                   scene: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """A stitched scene -> its host arrays, with one finalisation launch, the optional sieve (in place, on the same
    stream) and ONE device-to-host read: "counts" int64 [k], "class" uint8 [H, W], and as the options ask "probs" uint8
    [k, H, W], "margin" uint8 [H, W], "canvas" fp32 [H, W, k] (write_probs "f32"), "sieve" int64 [2].  With
    keep_probabilities one more read: "kept", the canvas.  The scene's canvases are dropped.  With options.nodata (scene:
    the uploaded scene, which holds the mask) the finalisation is the masked one, the sieve freezes nodata_out, and the
    read also carries "n_valid" int64 [1] and, with write_valid, "valid" uint8 [H, W]; a scene without a crop has no
    canvas: empty_scene_arrays.  With options.write_vectors the crack edges of the written map's vector_values and their
    rings are taken on the same stream after the sieve (vectorize.count_and_rings: components, offsets, one 4-byte read
    of the edge count, rings) and the read also carries "start", "comp", "ring", "rank", "flags" int32 [n_edges]; "edges"
    is the count, and a scene with more than vector_max_edges has the count alone.  With options.packed_output (an out_*
    option is set) every raster that becomes a file is packed for its writer on the same stream after the sieve
    (geotiff_write.pack_on_device, one launch each; the canvas from its [H, W, k] strides) and the read carries
    "packed_class", "packed_probs", ... uint8 [n] in place of the rasters; "class" itself only under write_vectors.  With
    options.out_overviews each of those rasters is reduced to its overview levels after the sieve, from the raster as it is
    written (raster_overviews: fu_map_overviews, one launch per six levels), every level is packed with a layout of its own
    size, and the read also carries "packed_class_ov1", "packed_class_ov2", ..."""
    from .postprocess import sieve as sieve_map
    from .stitch import PackedRead
    masked = options.nodata is not None
    if masked and scene["n"] == 0:
        return empty_scene_arrays(scene, len(class_values), options)
    maps = stitcher.combine_maps(key, class_values, probs=options.write_probs == "u8", margin=options.write_margin,
                                 counts=True, threshold=None if options.threshold is None else options.threshold[:2],
                                 valid=scene["valid"] if masked else None,
                                 nodata_value=options.nodata_out if masked else None)
    read = PackedRead()
    packed = options.packed_output
    rasters = {}                                         # the tensors that become files, by their array names
    for name in ("counts", "class", "probs", "margin"):
        if name in maps:
            if packed and name != "counts":
                rasters[name] = maps[name]
            else:
                read.add(name, maps[name])
    if options.write_probs == "f32":
        if packed:
            rasters["canvas"] = maps["canvas"].permute(2, 0, 1)
        else:
            read.add("canvas", maps["canvas"])
    if options.sieve is not None:
        min_pixels, connectivity, passes = options.sieve
        _, stats = sieve_map(maps["class"], min_pixels, connectivity, passes=passes, out=maps["class"],
                             **({"frozen_value": options.nodata_out} if masked else {}))
        read.add("sieve", stats)
    if masked:
        read.add("n_valid", scene["n_valid"])
        if options.write_valid:
            if packed:
                rasters["valid"] = scene["valid"]
            else:
                read.add("valid", scene["valid"])
    if packed:                                           # after the sieve: the class map as it is written
        from .datasets.geotiff_write import pack_on_device
        for name, t in rasters.items():
            dtype = np.float32 if t.dtype == torch.float32 else np.uint8
            read.add("packed_" + name, pack_on_device(t, output_layout(options, dtype, tuple(t.shape))))
            for l, level in enumerate(raster_overviews(t, name, options, scene["valid"] if masked else None), 1):
                read.add(f"packed_{name}_ov{l}", pack_on_device(level, output_layout(options, dtype, tuple(level.shape))))
        if options.write_vectors:
            read.add("class", maps["class"])             # one byte per pixel: the host sorts the rings with it
    if options.write_vectors:                            # of the map as it is written: after the sieve
        from .vectorize import count_and_rings, select_flags
        n_edges, rings = count_and_rings(maps["class"], select_flags(options.vector_values), options.vector_connectivity,
                                         max_edges=options.vector_max_edges)
        for name in VECTOR_ARRAYS if rings is not None else ():
            read.add(name, rings[name])
    arrays = read.read()
    if options.write_vectors:
        arrays["edges"] = n_edges                        # without the five arrays: the scene is over vector_max_edges
    if options.keep_probabilities:
        arrays["kept"] = maps["canvas"].cpu().numpy()
    stitcher.drop(key)
    return arrays


def write_scene(arrays: Dict[str, np.ndarray], scene: dict, options: InferOptions, path: str, out_path: str) -> dict:
    """Host only: write a scene's class map and the side rasters the options ask for from finalize_scene's arrays, with
    the input's georeferencing on the output grid (scene: "tags", "src_hw", "hw", "n") -> its summary.json record.  With
    options.nodata (scene: also "nodata", "skipped"; arrays: also "n_valid") the class map carries GDAL_NODATA =
    str(nodata_out) (tag 42113) beside the georeferencing -- the side rasters do not, 0 is a value there -- and
    write_valid writes arrays["valid"] as <image>_valid.tif.  With options.write_vectors (arrays: also the ring arrays
    and "edges") it writes <image>.geojson: write_scene_vectors.  With options.packed_output the arrays hold the packed
    bytes ("packed_class", ...) and every raster goes through geotiff_write.write_raster (write_output_raster); the record
    gains "output_format", with "bigtiff" per file.  With options.out_overviews every file also holds its overview images
    ("packed_class_ov1", ...; write_raster's overviews) and "output_format" gains "overviews", their number, and "cog":
    --out_cog was given and geotiff.cog_report of every file written is empty."""
    H, W = scene["hw"]
    tags = geo_tags_for_grid(scene["tags"], scene["src_hw"], (H, W))
    masked = options.nodata is not None
    big = {}                                             # file kind -> whether it was written as BigTIFF
    cog = {}                                             # ... -> whether it follows the cloud-optimised layout

    def put(file_path, kind, name, extra_tags):
        big[kind] = write_output_raster(file_path, arrays, name, options, extra_tags, (H, W))
        if options.out_cog:
            from .datasets.geotiff import cog_report
            cog[kind] = not cog_report(file_path)
        return file_path

    put(out_path, "class", "class", tags + [(42113, 2, str(options.nodata_out))] if masked else tags)
    rec = {"input": path, "output": out_path, "source_size": list(scene["src_hw"]), "grid_size": [H, W],
           "crops": scene["n"], "class_pixels": arrays["counts"].tolist()}
    if masked:
        rec.update(valid_pixels=int(arrays["n_valid"][0]), skipped_crops=int(scene["skipped"]), nodata=scene["nodata"])
        if options.write_valid:
            rec["valid"] = put(side_output_path(out_path, "valid"), "valid", "valid", tags)
    if options.write_probs == "u8":
        rec["probabilities"] = put(side_output_path(out_path, "prob"), "probabilities", "probs", tags)
    if options.write_margin:
        rec["margin"] = put(side_output_path(out_path, "margin"), "margin", "margin", tags)
    if options.write_probs == "f32":
        rec["probabilities"] = put(side_output_path(out_path, "prob"), "probabilities", "canvas", tags)
    if options.packed_output or any(big.values()):
        rec["output_format"] = options.output_format(big, options.overview_levels((H, W)), bool(cog) and all(cog.values()))
    if options.sieve is not None:
        merged, changed = arrays["sieve"].tolist()
        rec["sieve"] = dict(options.sieve_options, merged_components=merged, changed_pixels=changed)
    if options.write_vectors:
        rec["vectors"] = write_scene_vectors(arrays, scene, options, vector_output_path(out_path))
    return rec


def write_output_raster(file_path: str, arrays: Dict[str, np.ndarray], name: str, options: InferOptions, extra_tags,
                        hw: Tuple[int, int]) -> bool:
    """Write one raster of finalize_scene's arrays ("class", "probs", "margin", "valid", or "canvas", which is written as
    [k, H, W]) -> whether the file is BigTIFF.  With every out_* option at its default: write_strip_tiff, as always, but for
    a file classic TIFF cannot hold, which goes through geotiff_write.write_raster as BigTIFF strips (the canvas as a
    transposed view, cut per strip).  Else arrays["packed_" + name], the bytes finalize_scene packed, through
    write_raster."""
    from .datasets.geotiff_write import CLASSIC_LIMIT, classic_size, raster_layout, write_raster
    from .datasets.synthetic import write_strip_tiff
    if options.packed_output:
        shape = ((len(arrays["counts"]),) if name in ("probs", "canvas") else ()) + tuple(hw)
        dtype = np.float32 if name == "canvas" else np.uint8
        layout = output_layout(options, dtype, shape)
        overviews = None
        if options.out_overviews is not None:
            from .datasets.overviews import overview_sizes
            overviews = [(arrays[f"packed_{name}_ov{l}"], output_layout(options, dtype, shape[:-2] + size))
                         for l, size in enumerate(overview_sizes(hw[0], hw[1], options.overview_levels(hw)), 1)]
        return write_raster(file_path, arrays["packed_" + name], layout, compress=options.out_compress,
                            level=options.out_level, bigtiff=options.out_bigtiff, extra_tags=extra_tags,
                            threads=options.out_threads, overviews=overviews)["bigtiff"]
    array = arrays["canvas"].transpose(2, 0, 1) if name == "canvas" else arrays[name]
    n_segments = (1 if array.ndim == 2 else array.shape[0]) * -(-array.shape[-2] // 16)
    if classic_size(array.nbytes, n_segments, extra_tags) <= CLASSIC_LIMIT:
        write_strip_tiff(file_path, np.ascontiguousarray(array), extra_tags=extra_tags)
        return False
    layout = raster_layout(array.dtype, array.shape[-2], array.shape[-1], 1 if array.ndim == 2 else array.shape[0])
    return write_raster(file_path, array, layout, bigtiff="auto", extra_tags=extra_tags,
                        classic_limit=CLASSIC_LIMIT)["bigtiff"]


def vector_output_path(out_path: str) -> str:
    """<image>.geojson beside the class map <image>.tif."""
    return out_path[:-len(".tif")] + ".geojson"


def write_scene_vectors(arrays: Dict[str, np.ndarray], scene: dict, options: InferOptions, path: str) -> dict:
    """Host only: the polygons of a scene's written class map (vectorize.rings_to_polygons of finalize_scene's ring arrays,
    one per connected patch of options.vector_values) as GeoJSON in the raster's CRS -> the record's "vectors".  A scene
    over vector_max_edges gets {"skipped"} and no file; a scene without a selected pixel an empty FeatureCollection."""
    from .vectorize import crs_from_tags, grid_transform, rings_to_polygons, write_geojson
    if "start" not in arrays:
        return {"skipped": f"{arrays['edges']} edges > {options.vector_max_edges}"}
    polygons = rings_to_polygons(arrays, scene["hw"], arrays["class"])
    write_geojson(path, polygons, grid_transform(scene["tags"], scene["src_hw"], scene["hw"]), crs_from_tags(scene["tags"]))
    return {"path": path, "polygons": len(polygons), "rings": sum(len(p["rings"]) for p in polygons),
            "edges": int(arrays["edges"]), "values": list(options.vector_values),
            "connectivity": options.vector_connectivity}


def run_summary(records: List[dict], n_crops: int, seconds: float, max_resident: int, options: InferOptions,
                weights: str) -> dict:
    """summary.json of a run from its scene records and the resolved options."""
    summary = {"scenes": records, "n_scenes": len(records), "n_crops": n_crops, "seconds": seconds,
               "crops_per_s": n_crops / seconds if seconds > 0 else None, "max_resident_scenes": max_resident,
               "tta": recorded(options.tta, options.codes), "weights": weights, "blend": options.blend,
               "stride": options.stride}
    if options.threshold is not None:
        summary["threshold"] = options.rule
    if options.sieve is not None:
        summary["sieve"] = dict(options.sieve_options,
                                merged_components=sum(r["sieve"]["merged_components"] for r in records),
                                changed_pixels=sum(r["sieve"]["changed_pixels"] for r in records))
    if options.nodata is not None:
        summary["nodata"] = {"value": options.nodata, "out": options.nodata_out, "skip_empty": options.skip_empty,
                             "valid_pixels": sum(r["valid_pixels"] for r in records),
                             "skipped_crops": sum(r["skipped_crops"] for r in records)}
    if options.write_vectors:
        written = [r["vectors"] for r in records if "skipped" not in r["vectors"]]
        summary["vectors"] = {"values": list(options.vector_values), "connectivity": options.vector_connectivity,
                              "max_edges": options.vector_max_edges, "polygons": sum(v["polygons"] for v in written),
                              "rings": sum(v["rings"] for v in written), "edges": sum(v["edges"] for v in written),
                              "skipped_scenes": len(records) - len(written)}
    formats = [r["output_format"] for r in records if "output_format" in r]
    if options.packed_output or formats:                 # "bigtiff": whether any file of the run is BigTIFF
        summary["output_format"] = options.output_format(any(any(f["bigtiff"].values()) for f in formats),
                                                         max((f.get("overviews") or 0 for f in formats), default=0),
                                                         bool(formats) and all(f.get("cog") for f in formats))
    return summary


def infer(checkpoint_path: str, inputs: Sequence[str], out_dir: str, *, cfg: Optional[dict] = None, norm_params=None,
          options: Optional[InferOptions] = None, **keywords) -> dict:
    """Class maps of every input scene (see the module docstring).  cfg: the resolved config (default: resolve_cfg of
    the checkpoint's experiment).  norm_params: the parameter file of norm_mode 'global' (path, or the dict it holds;
    datasets.stats), looked up by the config's data set name and sensor; without it a 'global' config is rejected.
    options: an InferOptions, or in its place the keywords of InferOptions.make (infer_options.KEYWORDS) -- size / scale,
    stride, batch_size, tta, weights ('auto', 'raw' or 'ema'), blend, write_probs (None, "u8" or "f32"), write_margin,
    sieve / sieve_connectivity / sieve_passes (only the written class map is sieved), water_threshold / threshold_class
    / calibration (the one-versus-rest rule in place of the argmax), nodata / nodata_out / skip_empty / write_valid (the
    valid-pixel mask, see the module docstring), decode / decode_threads (where a scene's samples are unpacked),
    write_vectors / vector_values / vector_connectivity / vector_max_edges (polygons of the written class map),
    out_compress / out_level / out_predictor / out_tile / out_bigtiff / out_threads (the format of the written rasters),
    out_overviews / out_cog (overview images behind them, in the cloud-optimised order),
    n_workers, device, keep_probabilities.  Returns the
    summary.json dict, which records the weights served, the blend, the stride and, when set, "threshold" and "sieve";
    with keep_probabilities also "probabilities" {output path: fp32 [H, W, k] stitched canvas} (one more host read per
    scene; for tests and comparisons)."""
    from .datasets.assemble import scene_crops
    from .stitch import GpuImageStitcher

    t_start = time.perf_counter()
    if options is None:
        options = InferOptions.make(**keywords)
    elif keywords:
        raise TypeError(f"infer(): options together with the keywords {sorted(keywords)}; give one or the other")
    if cfg is None:
        cfg = resolve_cfg("/".join(checkpoint_path.split("/")[:-2]), checkpoint_path)
    cfg = _merge(CONFIG_DEFAULTS, cfg)
    sensor, channels, n_channels, global_params = model_inputs(cfg, norm_params)
    ch, cw = int(cfg["crop_height"]), int(cfg["crop_width"])
    options = options.resolve(ch, cw, cfg["batch_size"])
    paths, outs = scene_outputs(inputs, out_dir, sensor)

    dev = torch.device(options.device)
    model, chosen = load_eval_model(cfg, checkpoint_path, options.weights, n_channels, 3, dev)
    net = model.model
    options.check_classes(net.n_classes)
    net._get_ctx(dev, options.n_views * options.batch_size, ch, cw)   # the context owns fu_scene_crops' table: full size
    stitcher = GpuImageStitcher(net, dev, blend=options.blend)
    class_values = [0] + [255] * (net.n_classes - 1)     # clip(argmax, 0, 1) * 255
    crop_buf = torch.empty(options.batch_size, n_channels["ms_image"], ch, cw, dtype=torch.float32, device=dev)
    loader = torch.utils.data.DataLoader(SceneFiles(paths, sensor, channels, options.decode, options.decode_threads),
                                         batch_size=None, shuffle=False,
                                         num_workers=options.n_workers, pin_memory=dev.type == "cuda")
    queue = SceneQueue(loader, functools.partial(upload_scene, options=options, crop_hw=(ch, cw), device=dev,
                                                 ctx=lambda: net._ctx), options.batch_size)
    records, probabilities, n_crops = [], {}, 0

    def finish(done):
        for i, scene in done:
            arrays = finalize_scene(stitcher, str(i), class_values, options, scene)
            if options.keep_probabilities:
                probabilities[outs[i]] = arrays.pop("kept")
            records.append(write_scene(arrays, scene, options, paths[i], outs[i]))

    with torch.no_grad():
        for batch in queue.batches():
            scenes = [queue.resident[i] for i, _ in batch]
            x, _, _ = scene_crops(net._ctx, [(sc["grid"], b) for sc, (_, b) in zip(scenes, batch)], (ch, cw),
                                  cfg["norm_mode"], global_params, out=crop_buf)
            probs, _ = eval_forward(net, model._gather_sources({"image": x}), options.codes, want_probs=True)
            stitcher.add_images(range(len(batch)), [str(i) for i, _ in batch], [b for _, b in batch],
                                [sc["hw"][0] for sc in scenes], [sc["hw"][1] for sc in scenes], probs=probs)
            n_crops += len(batch)
            finish(queue.stitched(batch))
        finish(queue.stitched(()))                       # all-fill scenes behind the last crop (none without --nodata)

    summary = run_summary(records, n_crops, time.perf_counter() - t_start, queue.max_resident, options, chosen)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "summary.json"), "w") as fh:
        json.dump(summary, fh, indent=4)
    if options.keep_probabilities:
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
    ap.add_argument("--nodata", type=str, default=None, metavar="auto|V",
                    help="treat pixels that hold no data as such: a pixel is fill when a band is not finite or every band "
                         "equals V (auto: the scene's GDAL_NODATA tag, else 0).  Fill gets --nodata_out in the class map, 0 "
                         "in the probability and margin rasters, is not counted in class_pixels, and crops that are all fill "
                         "are not forwarded (default: off, every pixel is classified)")
    ap.add_argument("--nodata_out", type=int, default=NODATA_OUT_DEFAULT, metavar="N",
                    help="the class map's value of a pixel without data, in 1..254 (default 127); written as the class map's "
                         "GDAL_NODATA tag.  Needs --nodata")
    ap.add_argument("--keep_empty_crops", dest="skip_empty", action="store_false",
                    help="forward also the crops without a single valid pixel (default: skip them).  Needs --nodata")
    ap.add_argument("--write_valid", action="store_true",
                    help="also write the valid-pixel mask as <image>_valid.tif, uint8 [H, W] 0 / 1.  Needs --nodata")
    ap.add_argument("--decode", type=str, default="auto", choices=list(DECODE_CHOICES),
                    help="how a scene's samples reach the device.  auto (the default): a classic, uncompressed strip TIFF "
                         "is decoded on the host as always, every other file (tiles, Deflate / LZW / PackBits, predictors, "
                         "BigTIFF) is entropy-decoded on the host and unpacked on the device; device: every file that way; "
                         "host: every file through the numpy reader")
    ap.add_argument("--decode_threads", type=int, default=DECODE_THREADS_DEFAULT,
                    help="threads that inflate a scene's tiles or strips, 1..16 (default 4)")
    ap.add_argument("--write_vectors", action="store_true",
                    help="also write <image>.geojson: one polygon, with its holes, per connected patch of the written class "
                         "map (after --sieve), traced on the device, in the raster's CRS (default: off)")
    ap.add_argument("--vector_values", type=int, nargs="+", default=None, metavar="V",
                    help="the class-map values that get polygons, each in 0..255 (default 255, water).  Needs --write_vectors")
    ap.add_argument("--vector_connectivity", type=int, default=None, choices=[4, 8],
                    help="neighbours that join pixels into one polygon (default: --sieve_connectivity under --sieve, else "
                         "4).  Needs --write_vectors")
    ap.add_argument("--vector_max_edges", type=int, default=None, metavar="N",
                    help="a scene whose polygons have more than N pixel edges gets no .geojson; its record says so "
                         "(default 16777216).  Needs --write_vectors")
    ap.add_argument("--out_compress", type=str, default="none", choices=list(OUT_COMPRESS_CHOICES),
                    help="compression of the written rasters: none (the default) or deflate (zlib, per strip or tile)")
    ap.add_argument("--out_level", type=int, default=OUT_LEVEL_DEFAULT, metavar="L",
                    help="zlib level, 1..9 (default 6).  Needs --out_compress deflate")
    ap.add_argument("--out_predictor", type=str, default="auto", choices=list(OUT_PREDICTOR_CHOICES),
                    help="auto (the default): under deflate, horizontal differencing for the uint8 rasters and the "
                         "floating-point predictor for float32 probabilities; off: no predictor")
    def tile_side(text):                                 # N, or the explicit spelling of the default layout
        return text if text == OUT_TILE_STRIPS else int(text)

    ap.add_argument("--out_tile", type=tile_side, nargs="?", const=OUT_TILE_FLAG,
                    default=None, metavar="N",
                    help="write N x N tiles instead of 16-row strips; N a multiple of 16 (256 when the flag stands alone); "
                         "'strips' says the default explicitly")
    ap.add_argument("--out_bigtiff", type=str, default="auto", choices=list(OUT_BIGTIFF_CHOICES),
                    help="auto (the default): BigTIFF only for a file classic TIFF cannot hold; yes: always; no: never, and "
                         "a file above 4 GiB is an error")
    ap.add_argument("--out_threads", type=int, default=OUT_THREADS_DEFAULT, metavar="T",
                    help="threads that deflate a raster's strips or tiles, 1..16 (default 4)")
    ap.add_argument("--out_overviews", type=str, default=None, metavar="auto|N",
                    help="put N reduced-resolution images (each half the size of the one before) behind every written "
                         "raster, cut on the device; auto: until the smallest fits one tile (256 pixels for strips).  "
                         "Directories first, the smallest image's data first: the cloud-optimised order (default: none)")
    ap.add_argument("--out_cog", action="store_true",
                    help="cloud-optimised GeoTIFFs: --out_tile 512 and --out_overviews auto unless given; the records say "
                         "whether every written file passes the layout check")
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
    options = InferOptions.from_args(args)               # option errors before anything is read
    experiment_dir = "/".join(args.checkpoint_path.split("/")[:-2])
    cfg = resolve_cfg(experiment_dir, args.checkpoint_path)
    out = infer(args.checkpoint_path, args.inputs, args.out_dir, cfg=cfg, norm_params=args.norm_params, options=options)
    print(json.dumps({k: v for k, v in out.items() if k != "scenes"}))


if __name__ == "__main__":
    main()
