"""Writer for the GeoTIFFs a GIS expects of a scene's outputs: strips or tiles, compression none or Deflate, predictor 1 / 2 /
3, classic TIFF or BigTIFF, little-endian, planar-separate.  The mirror of datasets/geotiff.py, split at the same place:

  1. everything in front of the entropy coder -- planes, tiles or strips, edge padding, the predictor: pack_host is the
     numpy statement and the specification; pack_on_device is the same thing as one kernel launch (C ABI fu_tiff_pack) on a
     strided device tensor, so scene inference packs its rasters in HBM, before its one device-to-host read.
  2. entropy coder and container, on the host: write_raster deflates every segment with the standard library's zlib on a
     thread pool of min(threads, segments) workers (default 4, capped at 16, never sized from the machine's CPU count; zlib
     releases the interpreter lock) and writes the directory, the tag payloads and the segments.

The byte layout (`layout` is geotiff.py's fu_tiff_layout dict).  pack_host is the exact inverse of geotiff.unpack_host:
unpack_host(pack_host(a, L), L) == a, bit for bit.
  * Segments lie back to back at their nominal size in the order of geotiff._segments(layout): a tile is always seg_h x
    seg_w, the last strip holds the rows that are left.
  * A tile position outside the image holds the nearest image pixel (the index clamped per axis: edge replication), before
    the predictor, so padded runs difference to zeros and compress away.
  * Predictor 2 (integers): per segment row v[x] - v[x - 1] modulo 2^bits, the first value as it is.
  * Predictor 3 (IEEE samples): the row's values as bytes_per_sample byte planes of seg_w bytes, most significant first, then
    the whole row of bytes_per_sample * seg_w bytes differenced byte-wise -- across the plane boundaries, as unpack_host's
    running sum runs across them -- the first byte as it is.
  * Supported: little-endian, 1 / 2 / 4-byte unsigned / signed samples and 4-byte floats, 1..16 samples, planar-separate
    whenever there are several (inside a segment there is always one sample per pixel), strips or tiles whose sides are
    multiples of 16.

Several images in one file: write_raster(overviews=[...]) puts reduced-resolution images (datasets/overviews.py) behind the
full resolution in the order of the published cloud-optimised layout -- every IFD and tag payload in front of the data,
the data of the smallest image first -- which geotiff.cog_report checks.

Out of scope: LZW / PackBits / ZSTD encoders, GDAL's structural-metadata ghost block and per-tile leaders / trailers (their
exact text cannot be checked without GDAL, and validators treat them as optional), chunky or big-endian output, entropy
coding on the GPU.
"""
from __future__ import annotations

import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Tuple

import numpy as np

from .geotiff import _KINDS, _segments
from .tiff import TiffError

__all__ = ["pack_host", "pack_on_device", "write_raster", "raster_layout", "check_pack_layout", "classic_size",
           "WRITE_THREADS_DEFAULT", "WRITE_THREADS_MAX", "PACK_MAX_SAMPLES", "CLASSIC_LIMIT"]

WRITE_THREADS_DEFAULT, WRITE_THREADS_MAX = 4, 16
PACK_MAX_SAMPLES = 16           # FU_TIFF_MAX_BANDS
CLASSIC_LIMIT = 2 ** 32 - 1     # the largest file 32-bit offsets describe
_TYPE_SIZE = {2: 1, 3: 2, 4: 4, 12: 8, 16: 8}          # ASCII, SHORT, LONG, DOUBLE, LONG8
_TYPE_FMT = {3: "H", 4: "I", 12: "d", 16: "Q"}


# ------------------------------------------------------------------------------------------- in front of the entropy coder
def raster_layout(dtype, height: int, width: int, samples: int = 1, *, tile: Optional[int] = None, rows_per_strip: int = 16,
                  predictor: int = 1) -> dict:
    """The fu_tiff_layout dict of an output raster: little-endian, planar-separate, tiles of tile x tile or strips of
    rows_per_strip rows."""
    dt = np.dtype(dtype)
    kind = {"u": 1, "i": 2, "f": 3}.get(dt.kind)
    if kind is None:
        raise ValueError(f"unsupported sample type {dt}")
    tiled = tile is not None
    return {"width": int(width), "height": int(height), "samples": int(samples), "bytes_per_sample": dt.itemsize,
            "sample_kind": kind, "big_endian": 0, "planar": int(samples > 1), "tiled": int(tiled),
            "seg_w": int(tile) if tiled else int(width), "seg_h": int(tile) if tiled else min(int(rows_per_strip), int(height)),
            "predictor": int(predictor)}


def check_pack_layout(layout: dict) -> int:
    """What fu_tiff_pack checks of a layout, with its causes -> the layout's arithmetic total in bytes."""
    L = layout
    if L["width"] < 1 or L["height"] < 1 or L["seg_w"] < 1 or L["seg_h"] < 1:
        raise ValueError(f"bad layout {L}")
    if L["bytes_per_sample"] not in (1, 2, 4) or L["sample_kind"] not in (1, 2, 3) or L["predictor"] not in (1, 2, 3):
        raise ValueError(f"bad layout {L}")
    if L["sample_kind"] == 3 and L["bytes_per_sample"] != 4:
        raise ValueError(f"{L['bytes_per_sample']}-byte float samples are not supported")
    if L["big_endian"]:
        raise ValueError("big-endian output is not supported")
    if not 1 <= L["samples"] <= PACK_MAX_SAMPLES:
        raise ValueError(f"samples = {L['samples']} not in 1..{PACK_MAX_SAMPLES}")
    if L["samples"] > 1 and not L["planar"]:
        raise ValueError(f"chunky output of {L['samples']} samples is not supported (planar-separate only)")
    if L["predictor"] == 3 and L["sample_kind"] != 3:
        raise ValueError("predictor 3 (floating point) on integer samples")
    if L["predictor"] == 2 and L["sample_kind"] == 3:
        raise ValueError("predictor 2 (horizontal differencing) on floating-point samples")
    if L["tiled"]:
        if L["seg_w"] % 16 or L["seg_h"] % 16:
            raise ValueError(f"tile sides {L['seg_h']}x{L['seg_w']} are not multiples of 16")
        rows = L["samples"] * -(-L["width"] // L["seg_w"]) * -(-L["height"] // L["seg_h"]) * L["seg_h"]
    else:
        if L["seg_w"] != L["width"]:
            raise ValueError("strips are as wide as the image")
        rows = L["samples"] * L["height"]
    return rows * L["seg_w"] * L["bytes_per_sample"]


def _layout_dtype(layout: dict) -> np.dtype:
    return np.dtype(f"<{_KINDS[layout['sample_kind']]}{layout['bytes_per_sample']}")


def _as_planes(array, layout: dict):
    """array [H, W] or [samples, H, W], any strides (a transposed [H, W, k] canvas is a view) -> the [samples, H, W] view."""
    a = array if array.ndim == 3 else array[None]
    want = (layout["samples"], layout["height"], layout["width"])
    if array.ndim not in (2, 3) or tuple(a.shape) != want:
        raise ValueError(f"array of shape {tuple(array.shape)}, the layout describes {want} ([samples,] height, width)")
    return a


def pack_host(array: np.ndarray, layout: dict) -> np.ndarray:
    """The numpy statement of everything in front of the entropy coder and the specification of fu_tiff_pack: array ([H, W]
    or [samples, H, W] with any strides; same-size samples of the layout's kind) -> uint8 [n], the segments back to back
    (see the module docstring)."""
    L = layout
    total = check_pack_layout(L)
    a = _as_planes(np.asarray(array), L)
    dt = _layout_dtype(L)
    if a.dtype.kind != dt.kind or a.dtype.itemsize != dt.itemsize:
        raise ValueError(f"array of {a.dtype}, the layout describes {dt.name}")
    W, H, bps, seg_w = L["width"], L["height"], L["bytes_per_sample"], L["seg_w"]
    out = np.empty(total, dtype=np.uint8)
    pos = 0
    for p, y0, x0, rows, nbytes in _segments(L):
        ys = np.minimum(np.arange(y0, y0 + rows), H - 1)
        xs = np.minimum(np.arange(x0, x0 + seg_w), W - 1)
        block = np.ascontiguousarray(a[p][np.ix_(ys, xs)]).astype(dt, copy=False)       # [rows, seg_w], little-endian
        if L["predictor"] == 2:
            u = block.view(np.dtype(f"<u{bps}"))
            d = u.copy()
            d[:, 1:] = u[:, 1:] - u[:, :-1]                                            # modulo 2^bits
            seg = d.view(np.uint8)
        elif L["predictor"] == 3:
            planes = block.view(np.uint8).reshape(rows, seg_w, bps)[:, :, ::-1]       # most significant byte first
            row = np.ascontiguousarray(planes.transpose(0, 2, 1)).reshape(rows, bps * seg_w)
            seg = row.copy()
            seg[:, 1:] = row[:, 1:] - row[:, :-1]                                      # modulo 256, across the planes
        else:
            seg = block.view(np.uint8)
        out[pos:pos + nbytes] = seg.reshape(-1)
        pos += nbytes
    return out


def pack_on_device(tensor, layout: dict):
    """C ABI fu_tiff_pack: a tensor on the ROCm device, [H, W] or [samples, H, W] with any non-negative strides (canvas
    .permute(2, 0, 1) is a source without a copy) -> uint8 [n] on the device, bit for bit pack_host of the same array.  One
    launch on the current stream; no host pass over the samples."""
    import torch

    from .. import _lib
    from .geotiff import layout_struct
    if not torch.is_tensor(tensor) or tensor.device.type != "cuda":
        raise RuntimeError("pack_on_device runs only on a ROCm GPU tensor; the host statement is pack_host")
    total = check_pack_layout(layout)
    a = _as_planes(tensor, layout)
    dt = _layout_dtype(layout)
    if a.dtype != getattr(torch, {"u1": "uint8", "u2": "uint16", "u4": "uint32", "i1": "int8", "i2": "int16", "i4": "int32",
                                  "f4": "float32"}[dt.str[1:]], None):
        raise ValueError(f"tensor of {a.dtype}, the layout describes {dt.name}")
    strides = [int(s) for s in a.stride()]
    if min(strides) < 0:
        raise ValueError("pack_on_device: negative strides are not supported")
    out = torch.empty(total, dtype=torch.uint8, device=a.device)
    _lib.check(_lib.load().fu_tiff_pack(a.data_ptr(), strides[0], strides[1], strides[2], layout_struct(layout),
                                        _lib.ptr(out), total, torch.cuda.current_stream(a.device).cuda_stream))
    return out


# ------------------------------------------------------------------------------------------------------------ container
def check_write_threads(threads) -> int:
    if isinstance(threads, bool) or int(threads) != threads or not 1 <= int(threads) <= WRITE_THREADS_MAX:
        raise ValueError(f"threads must be an integer in 1..{WRITE_THREADS_MAX}, got {threads!r}")
    return int(threads)


def _payload(typ: int, vals) -> bytes:
    if typ == 2:                                 # ASCII: the string and its terminating NUL
        return vals.encode("ascii") + b"\0"
    if isinstance(vals, np.ndarray):
        return vals.astype(np.dtype("<" + {3: "u2", 4: "u4", 12: "f8", 16: "u8"}[typ])).tobytes()
    return struct.pack("<" + _TYPE_FMT[typ] * len(vals), *vals)


def _directories(images, big: bool) -> Tuple[bytes, List[np.ndarray]]:
    """Header and, for every image in file order, its IFD and tag payloads; images: [(tags, counts, offsets_tag)].  The
    segments follow them, the LAST image's first and the first image's last, inside an image with the byte counts `counts`
    in their order -> (those bytes, the segments' offsets per image).  Payloads longer than an entry's value field start
    on word boundaries, in tag order; the IFDs are chained through their next-IFD fields."""
    head, entry, inline = (16, 20, 8) if big else (8, 12, 4)
    cursor = head
    raws, where, starts = [], [], []
    for tags, counts, offsets_tag in images:
        starts.append(cursor)
        cursor += (8 if big else 2) + entry * len(tags) + (8 if big else 4)
        raws.append({}), where.append({})
        for tag, typ, vals in tags:
            if tag == offsets_tag:
                size = _TYPE_SIZE[typ] * len(counts)
            else:
                raws[-1][tag] = _payload(typ, vals)
                size = len(raws[-1][tag])
            if size > inline:
                where[-1][tag] = cursor
                cursor += size + (size & 1)
    offsets: List = [None] * len(images)
    for i in reversed(range(len(images))):                           # the data: the smallest image first
        counts = images[i][1]
        offsets[i] = cursor + np.concatenate([[0], np.cumsum(counts[:-1], dtype=np.int64)]).astype(np.int64)
        cursor = int(offsets[i][-1] + counts[-1])
    out = [b"II" + (struct.pack("<HHHQ", 43, 8, 0, 16) if big else struct.pack("<HI", 42, 8))]
    for i, (tags, counts, offsets_tag) in enumerate(images):
        entries, blobs = [], []
        for tag, typ, vals in tags:
            raw = _payload(typ, offsets[i]) if tag == offsets_tag else raws[i][tag]
            cnt = len(raw) // _TYPE_SIZE[typ]
            e = struct.pack("<HHQ" if big else "<HHI", tag, typ, cnt)
            if len(raw) <= inline:
                entries.append(e + raw.ljust(inline, b"\0"))
            else:
                entries.append(e + struct.pack("<Q" if big else "<I", where[i][tag]))
                blobs.append(raw + b"\0" * (len(raw) & 1))
        following = starts[i + 1] if i + 1 < len(images) else 0
        out.append(struct.pack("<Q" if big else "<H", len(tags)) + b"".join(entries)
                   + struct.pack("<Q" if big else "<I", following) + b"".join(blobs))
    return b"".join(out), offsets


def _image_tags(layout: dict, compression: int, counts, big: bool, extra_tags) -> Tuple[list, int]:
    L = layout
    n, spp = len(counts), L["samples"]
    size_t = lambda v: 3 if v < 65536 else 4                                         # noqa: E731
    off_t = 16 if big else 4
    tags = [(256, size_t(L["width"]), [L["width"]]), (257, size_t(L["height"]), [L["height"]]),
            (258, 3, [8 * L["bytes_per_sample"]] * spp), (259, 3, [compression]), (262, 3, [1]), (277, 3, [spp]),
            (284, 3, [2 if spp > 1 else 1]), (339, 3, [L["sample_kind"]] * spp)]
    if L["predictor"] != 1:
        tags.append((317, 3, [L["predictor"]]))
    if L["tiled"]:
        offsets_tag = 324
        tags += [(322, size_t(L["seg_w"]), [L["seg_w"]]), (323, size_t(L["seg_h"]), [L["seg_h"]]), (324, off_t, None),
                 (325, off_t, counts)]
    else:
        offsets_tag = 273
        tags += [(273, off_t, None), (278, size_t(L["seg_h"]), [L["seg_h"]]), (279, off_t, counts)]
    if extra_tags:
        own = {t for t, _, _ in tags}
        for tag, typ, vals in extra_tags:
            if tag in own or typ not in (2, 3, 4, 12):
                raise ValueError(f"write_raster: extra tag {tag} of type {typ} is not supported")
        tags = tags + [(int(t), int(ty), v) for t, ty, v in extra_tags]
    return sorted(tags, key=lambda t: t[0]), offsets_tag


def classic_size(array_bytes: int, n_segments: int, extra_tags=None) -> int:
    """An upper bound of the size of the classic, uncompressed file of array_bytes samples in n_segments segments."""
    extra = sum(16 + (len(v) + 1 if isinstance(v, str) else 8 * len(v)) for _, _, v in (extra_tags or ()))
    return 8 + 2 + 12 * 16 + 4 + 8 * n_segments + 64 * PACK_MAX_SAMPLES + extra + array_bytes


NODATA_TAG = 42113              # GDAL_NODATA: the one extra tag that goes on the overview IFDs as well


def _segment_views(segments_or_array, layout: dict) -> List:
    """The packed bytes of one image (or the image itself, through pack_host) cut into its segments."""
    total = check_pack_layout(layout)
    data = np.asarray(segments_or_array)
    if not (data.ndim == 1 and data.dtype == np.uint8 and data.size == total):
        data = pack_host(data, layout)
    view = memoryview(np.ascontiguousarray(data))
    bounds = np.concatenate([[0], np.cumsum([s[4] for s in _segments(layout)], dtype=np.int64)])
    return [view[int(a):int(b)] for a, b in zip(bounds[:-1], bounds[1:])]


def write_raster(path: str, segments_or_array, layout: dict, *, compress: str = "none", level: int = 6,
                 bigtiff: str = "auto", extra_tags=None, threads: int = WRITE_THREADS_DEFAULT,
                 classic_limit: int = CLASSIC_LIMIT, overviews=None) -> dict:
    """Write a TIFF: its full-resolution image and, with `overviews`, the reduced-resolution images behind it.
    segments_or_array: the packed bytes (uint8 [n] with n the layout's total: pack_host's or pack_on_device's buffer, read
    to the host) or the image itself ([H, W] or [samples, H, W]), which goes through pack_host.  compress: "none"
    (Compression 1) or "deflate" (8: zlib.compress(segment, level) per segment, level 1..9).  bigtiff: "auto" -- classic
    TIFF if and only if the finished file's size is <= classic_limit, else BigTIFF (version 43, 8-byte offsets, 20-byte
    entries, LONG8 offsets and byte counts); "yes" forces BigTIFF; "no" forces classic and raises a TiffError naming the
    size when the file does not fit.  extra_tags: (tag, type, values) triples with write_strip_tiff's rules (type 2 ASCII, 3
    SHORT, 4 LONG, 12 DOUBLE; none of the image's own tags), e.g. the georeferencing.  File order: directory, tag payloads
    on word boundaries, segments.  All compressed segments are held in memory before the directory is written, so every
    offset is exact.  -> {"bigtiff", "size", "segments"}.
    overviews: None (the file is byte for byte what it always was) or [(segments_or_array, layout), ...] in decreasing
    size, e.g. datasets/overviews.py's levels.  Then the file is laid out as a cloud-optimised reader wants it: the header;
    IFD 0 with its payloads; every overview IFD with its payloads, in decreasing size, chained through the next-IFD
    pointers; then the segment data, the smallest overview first and the full resolution last.  Overview IFDs carry
    NewSubfileType (254) = 1; extra_tags go on IFD 0 only, except GDAL_NODATA (42113), which every IFD of a file that has
    it carries.  The classic / BigTIFF decision is made on the size of the whole file, and the segments of all images are
    deflated on one thread pool.  The result also has "overviews": their number, and "segments" counts all images'."""
    if compress not in ("none", "deflate"):
        raise ValueError(f"compress must be 'none' or 'deflate', got {compress!r}")
    if isinstance(level, bool) or int(level) != level or not 1 <= int(level) <= 9:
        raise ValueError(f"level must be an integer in 1..9, got {level!r}")
    if bigtiff not in ("auto", "yes", "no"):
        raise ValueError(f"bigtiff must be 'auto', 'yes' or 'no', got {bigtiff!r}")
    threads = check_write_threads(threads)
    layouts = [layout] + [L for _, L in overviews or ()]
    for big_one, small in zip(layouts[:-1], layouts[1:]):
        if small["width"] > big_one["width"] or small["height"] > big_one["height"] or \
                (small["width"], small["height"]) == (big_one["width"], big_one["height"]):
            raise ValueError("write_raster: overviews come in decreasing size")
    per_image = [_segment_views(segments_or_array, layout)] + [_segment_views(a, L) for a, L in overviews or ()]
    parts: List = [seg for image in per_image for seg in image]
    if compress == "deflate":
        deflate = lambda seg: zlib.compress(seg, int(level))                        # noqa: E731
        if threads > 1 and len(parts) > 1:
            with ThreadPoolExecutor(max_workers=min(threads, len(parts))) as pool:
                parts = list(pool.map(deflate, parts))
        else:
            parts = [deflate(seg) for seg in parts]
    ends = np.cumsum([len(image) for image in per_image])
    per_image = [parts[int(e) - len(image):int(e)] for e, image in zip(ends, per_image)]
    counts = [np.array([len(p) for p in image], dtype=np.int64) for image in per_image]
    scheme = 8 if compress == "deflate" else 1
    reduced_tags = [(254, 4, [1])] + [t for t in extra_tags or () if t[0] == NODATA_TAG]

    def directories(big):
        images = [_image_tags(L, scheme, c, big, reduced_tags if i else extra_tags) + (c,)
                  for i, (L, c) in enumerate(zip(layouts, counts))]
        head, offsets = _directories([(tags, c, offsets_tag) for tags, offsets_tag, c in images], big)
        return head, int(offsets[0][-1] + counts[0][-1])             # the full resolution's data ends the file

    big = bigtiff == "yes"
    if not big:
        head, size = directories(False)
        if size > classic_limit:
            if bigtiff == "no":
                raise TiffError(f"{path}: a file of {size} bytes does not fit classic TIFF (limit {classic_limit}); "
                                "write it as BigTIFF")
            big = True
    if big:
        head, size = directories(True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(head)
        for image in reversed(per_image):
            for p in image:
                fh.write(p)
    result = {"bigtiff": big, "size": size, "segments": len(parts)}
    if overviews is not None:
        result["overviews"] = len(overviews)
    return result

