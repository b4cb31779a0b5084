"""Reader for the GeoTIFFs people actually have: classic and BigTIFF, both byte orders, strips and tiles, chunky and
planar-separate samples, compression none / Deflate (8, 32946) / LZW (5) / PackBits (32773), predictor 1 / 2 / 3, 8/16/32/64-
bit unsigned / signed / IEEE samples.  The first IFD unless asked otherwise: raster_ifds counts a file's images and the ifd
keyword of raster_info / raster_size / read_raster / read_raster_encoded picks one (an overview, a mask); cog_report checks
the cloud-optimised layout geotiff_write.write_raster(overviews=...) writes.  `datasets/tiff.py` stays the
strict reader of the rasters bundled with the reference and is not touched; for a file it accepts, read_raster returns
read_tiff's array.

Two stages, split where the work changes character:
  1. container and entropy codecs, on the host: parse the IFD through an mmap of the file (a file above 4 GB is not copied
     twice), inflate every segment to its nominal size into ONE contiguous byte buffer, segments back to back in the order
     of the file's offset array -- read_raster_encoded(path) -> (bytes, layout).  Deflate is the standard library's zlib;
     LZW and PackBits are the library's fu_tiff_lzw_decode / fu_tiff_packbits_decode (plain C++, csrc/fu_tiff_codec.cpp: no
     HIP call, so a DataLoader worker that decodes never opens the GPU), with slow pure-Python statements here
     (lzw_decode_host, packbits_decode_host; codec="python" routes through them).  Segments are decoded by a thread pool
     of at most decode_threads (default 4, capped at 16, never sized from the machine's CPU count); zlib and the ctypes
     calls release the interpreter lock.
  2. everything after it -- undo the predictor, swap bytes, take tiles apart, crop edge tiles, convert: unpack_host is the
     numpy statement and the specification; unpack_on_device is the same thing as one kernel launch (C ABI
     fu_tiff_unpack) that also picks the bands and writes the fp32 [bands, H, W] raster scene inference uploads.

read_raster(path) = unpack_host(*read_raster_encoded(path)), with read_tiff's return conventions: one sample per pixel ->
[H, W]; planar-separate -> [bands, H, W]; chunky with several samples -> [H, W, bands]; native-endian, C-contiguous.

Predictors.  2 is horizontal differencing on integers: after the byte swap, per sample component, per row of the segment,
a running sum modulo 2^bits.  3 is the floating-point predictor on 32/64-bit IEEE samples: with wc = segment width x samples
per pixel in the segment, per segment row a byte-wise running sum modulo 256 with stride = samples per pixel in the segment;
then byte b (most significant first) of value i is byte b * wc + i of the row, in both file byte orders.

Not supported (TiffError naming the cause): JPEG, ZSTD, LERC, WebP and every other scheme, sub-byte samples, mixed sample
types.  Writing is datasets/geotiff_write.py: pack_host there is the exact inverse of unpack_host here.
"""
from __future__ import annotations

import mmap
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Sequence, Tuple

import numpy as np

from .tiff import GEOTIFF_TAGS, TiffError

__all__ = ["raster_info", "raster_size", "raster_ifds", "cog_report", "raster_geotiff_tags", "read_raster",
           "read_raster_encoded", "unpack_host", "unpack_on_device", "lzw_decode_host", "packbits_decode_host",
           "strict_reader_accepts", "check_decode_threads", "DECODE_THREADS_DEFAULT", "DECODE_THREADS_MAX", "UNPACK_CHUNK", "UNPACK_MAX_BANDS"]

DECODE_THREADS_DEFAULT, DECODE_THREADS_MAX = 4, 16
UNPACK_CHUNK = 256         # FU_TIFF_UNPACK_CHUNK: the pixels of a segment row fu_tiff_unpack takes per pass
UNPACK_MAX_BANDS = 16      # FU_TIFF_MAX_BANDS
_TYPE_FMT = {1: "B", 2: "c", 3: "H", 4: "I", 5: "II", 6: "b", 7: "B", 8: "h", 9: "i", 10: "ii", 11: "f", 12: "d", 13: "I",
             16: "Q", 17: "q", 18: "Q"}
_DECODE_TAGS = (256, 257, 258, 259, 273, 277, 278, 279, 284, 317, 322, 323, 324, 325, 339)
_ARRAY_TAGS = (273, 279, 324, 325)          # offsets and byte counts: kept as int64 arrays, a COG has many thousands
_SCHEME_NAMES = {1: "none", 2: "CCITT RLE", 3: "CCITT T.4", 4: "CCITT T.6", 5: "LZW", 6: "old-style JPEG", 7: "JPEG",
                 8: "Deflate", 32773: "PackBits", 32946: "Deflate", 34712: "JPEG 2000", 34887: "LERC", 34925: "LZMA",
                 50000: "ZSTD", 50001: "WebP", 50002: "JPEG XL"}
_SUPPORTED_SCHEMES = (1, 5, 8, 32773, 32946)
_KINDS = {1: "u", 2: "i", 3: "f"}


def check_decode_threads(decode_threads) -> int:
    if isinstance(decode_threads, bool) or int(decode_threads) != decode_threads or not 1 <= int(decode_threads) <= \
            DECODE_THREADS_MAX:
        raise ValueError(f"decode_threads must be an integer in 1..{DECODE_THREADS_MAX}, got {decode_threads!r}")
    return int(decode_threads)


# ------------------------------------------------------------------------------------------------------------ container
def _map(path: str):
    with open(path, "rb") as fh:
        try:
            return mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
        except ValueError:
            raise TiffError("file too short for a TIFF header") from None


def _header(buf) -> Tuple[str, bool, int]:
    """-> (byte order, is BigTIFF, offset of the first IFD)."""
    size = len(buf)
    if size < 8:
        raise TiffError("file too short for a TIFF header")
    head = bytes(buf[:2])
    if head == b"II":
        bo = "<"
    elif head == b"MM":
        bo = ">"
    else:
        raise TiffError("not a TIFF file (bad byte-order mark)")
    (magic,) = struct.unpack(bo + "H", buf[2:4])
    if magic == 42:
        (ifd,) = struct.unpack(bo + "I", buf[4:8])
        return bo, False, ifd
    if magic == 43:
        if size < 16:
            raise TiffError("file too short for a BigTIFF header")
        off_size, zero, ifd = struct.unpack(bo + "HHQ", buf[4:16])
        if off_size != 8 or zero != 0:
            raise TiffError(f"BigTIFF with {off_size}-byte offsets is not supported")
        return bo, True, ifd
    raise TiffError(f"not a TIFF file (magic {magic})")


def _ifd_extent(buf, bo: str, big: bool, ifd: int) -> Tuple[int, int]:
    """-> (number of entries, offset of the next IFD or 0) of the IFD at `ifd`, checked against the file's size."""
    count_fmt, entry_size, off_fmt = ("Q", 20, "Q") if big else ("H", 12, "I")
    count_size, off_size = struct.calcsize(count_fmt), struct.calcsize(off_fmt)
    if ifd + count_size > len(buf):
        raise TiffError("IFD offset beyond the end of the file")
    (n,) = struct.unpack(bo + count_fmt, buf[ifd:ifd + count_size])
    end = ifd + count_size + entry_size * n
    if end > len(buf):
        raise TiffError("truncated IFD")
    following = struct.unpack(bo + off_fmt, buf[end:end + off_size])[0] if end + off_size <= len(buf) else 0
    return n, following


def _ifd_offsets(buf) -> Tuple[str, bool, List[int]]:
    """-> (byte order, is BigTIFF, the offsets of the chain's IFDs in order); a chain that loops raises TiffError."""
    bo, big, ifd = _header(buf)
    chain: List[int] = []
    while ifd:
        if ifd in chain:
            raise TiffError("the IFD chain loops")
        chain.append(ifd)
        ifd = _ifd_extent(buf, bo, big, ifd)[1]
    if not chain:
        raise TiffError("the file has no IFD")
    return bo, big, chain


def _parse_ifd(buf, keep=(), ifd: int = 0, spans=None) -> Tuple[str, bool, Dict[int, object]]:
    """-> (byte order, is BigTIFF, {tag number: values}) of IFD number `ifd` of the chain (0: the first, which needs no walk):
    the decoding tags and the tags in keep.  Offsets and byte counts come as int64 arrays, ASCII values of kept tags as str,
    everything else as tuples.  spans: a list that receives (start, end) of the IFD and of every value stored outside it."""
    size = len(buf)
    if isinstance(ifd, bool) or int(ifd) != ifd or int(ifd) < 0:
        raise ValueError(f"ifd must be an integer >= 0, got {ifd!r}")
    if ifd == 0:
        bo, big, at = _header(buf)
    else:
        bo, big, chain = _ifd_offsets(buf)
        if ifd >= len(chain):
            raise TiffError(f"IFD {ifd} lies beyond the chain of {len(chain)} image{'s' if len(chain) != 1 else ''}")
        at = chain[int(ifd)]
    ifd = at
    count_fmt, entry_size, inline, off_fmt = ("Q", 20, 8, "Q") if big else ("H", 12, 4, "I")
    count_size = struct.calcsize(count_fmt)
    n, _ = _ifd_extent(buf, bo, big, ifd)
    if spans is not None:
        spans.append((ifd, ifd + count_size + entry_size * n + struct.calcsize(off_fmt)))
    tags: Dict[int, object] = {}
    for i in range(n):
        e = buf[ifd + count_size + entry_size * i: ifd + count_size + entry_size * (i + 1)]
        tag, typ, cnt = struct.unpack(bo + ("HHQ" if big else "HHI"), e[:entry_size - inline])
        fmt = _TYPE_FMT.get(typ)
        if spans is not None and fmt is not None and struct.calcsize(bo + fmt) * cnt > inline:
            (off,) = struct.unpack(bo + off_fmt, e[entry_size - inline:])
            spans.append((off, off + struct.calcsize(bo + fmt) * cnt))
        if tag not in _DECODE_TAGS and tag not in keep:
            continue
        if fmt is None:
            raise TiffError(f"tag {tag}: unknown field type {typ}")
        nbytes = struct.calcsize(bo + fmt) * cnt
        if nbytes <= inline:
            raw = bytes(e[entry_size - inline: entry_size - inline + nbytes])
        else:
            (off,) = struct.unpack(bo + off_fmt, e[entry_size - inline:])
            if off + nbytes > size:
                raise TiffError(f"tag {tag}: value beyond the end of the file")
            raw = bytes(buf[off:off + nbytes])
        if typ == 2 and tag in keep:
            tags[tag] = raw.split(b"\0", 1)[0].decode("ascii", "replace")
        elif tag in _ARRAY_TAGS and fmt in ("H", "I", "Q"):
            tags[tag] = np.frombuffer(raw, dtype=np.dtype(bo + {"H": "u2", "I": "u4", "Q": "u8"}[fmt])).astype(np.int64)
        else:
            tags[tag] = struct.unpack(bo + fmt[0] * (cnt * len(fmt)), raw)
    return bo, big, tags


def _first(tags, tag, default):
    v = tags.get(tag)
    return default if v is None or len(v) == 0 else int(v[0])


def _describe(bo: str, big: bool, tags: Dict[int, object]) -> dict:
    """The first image as the decoder needs it; every unsupported feature is named here, before any sample is touched."""
    for req, name in ((256, "width"), (257, "height")):
        if req not in tags:
            raise TiffError(f"missing required tag: {name}")
    width, height = int(tags[256][0]), int(tags[257][0])
    if width < 1 or height < 1:
        raise TiffError(f"empty image {height}x{width}")
    spp = _first(tags, 277, 1)
    if not 1 <= spp <= 64:
        raise TiffError(f"{spp} samples per pixel are not supported (1..64)")
    bits = tags.get(258, (1,) * spp)
    if len(set(bits)) != 1 or len(bits) not in (1, spp):
        raise TiffError(f"mixed bits per sample {bits} are not supported")
    bits = int(bits[0])
    scheme = _first(tags, 259, 1)
    if scheme not in _SUPPORTED_SCHEMES:
        raise TiffError(f"compression scheme {scheme} ({_SCHEME_NAMES.get(scheme, 'unknown')}) is not supported")
    if bits < 8:
        raise TiffError(f"sub-byte samples ({bits} bits per sample) are not supported")
    fmt = tags.get(339, (1,))
    if len(set(fmt)) != 1:
        raise TiffError(f"mixed sample formats {fmt} are not supported")
    kind = _KINDS.get(int(fmt[0]))
    if kind is None or bits not in (8, 16, 32, 64) or (kind == "f" and bits < 32):
        raise TiffError(f"unsupported sample type: format {fmt[0]}, {bits} bits")
    planar = _first(tags, 284, 1)
    if planar not in (1, 2):
        raise TiffError(f"bad PlanarConfiguration {planar}")
    predictor = _first(tags, 317, 1)
    if predictor not in (1, 2, 3):
        raise TiffError(f"unknown predictor {predictor}")
    if predictor == 3 and kind != "f":
        raise TiffError(f"predictor 3 (floating point) on integer samples ({kind}{bits // 8})")
    if predictor == 2 and kind == "f":
        raise TiffError(f"predictor 2 (horizontal differencing) on floating-point samples (f{bits // 8})")
    tiled = 322 in tags or 324 in tags
    if tiled:
        for req, name in ((322, "tile_width"), (323, "tile_length"), (324, "tile_offsets"), (325, "tile_byte_counts")):
            if req not in tags:
                raise TiffError(f"missing required tag: {name}")
        seg_w, seg_h = int(tags[322][0]), int(tags[323][0])
        if seg_w < 1 or seg_h < 1:
            raise TiffError(f"bad tile size {seg_h}x{seg_w}")
        offsets, counts = tags[324], tags[325]
        per_plane = -(-width // seg_w) * -(-height // seg_h)
    else:
        for req, name in ((273, "strip_offsets"), (279, "strip_bytes")):
            if req not in tags:
                raise TiffError(f"missing required tag: {name}")
        rps = _first(tags, 278, height)
        seg_w, seg_h = width, (min(rps, height) if rps > 0 else height)
        offsets, counts = tags[273], tags[279]
        per_plane = -(-height // seg_h)
    planes = spp if planar == 2 else 1
    offsets, counts = np.asarray(offsets, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    if len(offsets) != per_plane * planes or len(counts) != len(offsets):
        raise TiffError(f"{len(offsets)} {'tiles' if tiled else 'strips'}, expected {per_plane * planes}")
    return {"height": height, "width": width, "samples": spp, "dtype": np.dtype(f"{kind}{bits // 8}").name,
            "planar": planar, "tiled": tiled, "seg_w": seg_w, "seg_h": seg_h, "rows_per_strip": None if tiled else seg_h,
            "byteorder": bo, "bigtiff": big, "compression": scheme, "predictor": predictor, "kind": kind,
            "bytes_per_sample": bits // 8, "offsets": offsets, "counts": counts}


def raster_info(path: str, ifd: int = 0) -> dict:
    """Header fields only (image number `ifd` of the file; 0, the default, is the first IFD): tiff_info's keys -- height,
    width, samples, dtype, planar, rows_per_strip (None for tiles), byteorder -- plus bigtiff, tiled, seg_w, seg_h,
    compression, predictor.  An ifd beyond the chain raises TiffError."""
    info = _describe(*_parse_ifd(_map(path), ifd=ifd))
    return {k: v for k, v in info.items() if k not in ("offsets", "counts", "kind", "bytes_per_sample")}


def raster_size(path: str, ifd: int = 0) -> Tuple[int, int]:
    """(height, width), as tiff_size."""
    info = raster_info(path, ifd)
    return info["height"], info["width"]


def raster_ifds(path: str) -> int:
    """The number of images (IFDs) in the file: 1 + its overviews and whatever else its chain holds."""
    return len(_ifd_offsets(_map(path))[2])


def cog_report(path: str) -> List[str]:
    """The rules of the published cloud-optimised GeoTIFF layout the file violates; an empty list means compliant.  Host
    only, the statement the tests use:
      * every image is tiled;
      * every IFD and tag payload lies before the first byte of segment data;
      * the IFDs are in decreasing size, and every one but the first is marked reduced-resolution (NewSubfileType bit 0);
      * each image's data lies after the data of every smaller image;
      * an image with a side above its tile side has overviews down to at most one tile.
    Not looked at: GDAL's structural-metadata ghost block and the per-tile leaders / trailers, which are optional."""
    buf = _map(path)
    n = len(_ifd_offsets(buf)[2])
    spans: List[Tuple[int, int]] = []
    images = []
    for i in range(n):
        bo, big, tags = _parse_ifd(buf, keep=(254,), ifd=i, spans=spans)
        images.append((_describe(bo, big, tags), _first(tags, 254, 0)))
    out = []
    for i, (info, _) in enumerate(images):
        if not info["tiled"]:
            out.append(f"every image is tiled: IFD {i} is stored in strips")
    stored = [(int(info["offsets"][info["counts"] > 0].min(initial=len(buf))),
               int((info["offsets"] + info["counts"]).max())) for info, _ in images]
    first_data = min(s[0] for s in stored)
    late = max(end for _, end in spans)
    if late > first_data:
        out.append(f"every IFD and tag payload lies before the segment data: directory bytes end at {late}, the data "
                   f"starts at {first_data}")
    for i in range(1, n):
        (a, _), (b, sub) = images[i - 1], images[i]
        if b["height"] > a["height"] or b["width"] > a["width"] or (b["height"], b["width"]) == (a["height"], a["width"]):
            out.append(f"the IFDs are in decreasing size: IFD {i} is {b['height']}x{b['width']} after "
                       f"{a['height']}x{a['width']}")
        if not sub & 1:
            out.append(f"every IFD but the first is marked reduced-resolution: IFD {i} has NewSubfileType {sub}")
        if stored[i - 1][0] < stored[i][1]:
            out.append(f"each image's data lies after the data of every smaller image: IFD {i - 1} starts at "
                       f"{stored[i - 1][0]}, IFD {i} ends at {stored[i][1]}")
    full, smallest = images[0][0], images[-1][0]
    if full["tiled"] and (full["height"] > full["seg_h"] or full["width"] > full["seg_w"]) and \
            (smallest["height"] > full["seg_h"] or smallest["width"] > full["seg_w"]):
        out.append(f"an image larger than its tile has overviews down to at most one tile: the smallest image is "
                   f"{smallest['height']}x{smallest['width']}, the tile {full['seg_h']}x{full['seg_w']}")
    return out


def raster_geotiff_tags(path: str) -> Dict[int, object]:
    """read_geotiff_tags for every container this module reads: the GEOTIFF_TAGS of the first IFD, {tag: tuple of numbers,
    or str for ASCII}; the samples are not decoded."""
    _, _, tags = _parse_ifd(_map(path), keep=GEOTIFF_TAGS)
    return {k: (tuple(v.tolist()) if isinstance(v, np.ndarray) else v) for k, v in tags.items() if k in GEOTIFF_TAGS}


def strict_reader_accepts(path: str) -> bool:
    """Whether datasets/tiff.py's read_tiff takes the file: classic TIFF, strips, no compression, no predictor.  Decided
    from the header alone."""
    try:
        info = raster_info(path)
    except TiffError:
        return False
    return not (info["bigtiff"] or info["tiled"] or info["compression"] != 1 or info["predictor"] != 1)


# --------------------------------------------------------------------------------------------------------------- codecs
def lzw_decode_host(data: bytes, n_dst: int) -> bytes:
    """The statement of fu_tiff_lzw_decode (TIFF 6.0 section 13), slow: MSB-first codes of 9..12 bits, Clear = 256,
    EndOfInformation = 257, the width grows one code early, a code equal to the next free entry is the previous string
    plus its own first byte; stops at n_dst bytes, at EndOfInformation or where the stream ends.  TiffError on a code that
    cannot occur and on the LSB-first variant of old writers."""
    data = bytes(data)
    if len(data) >= 2 and data[0] == 0 and data[1] & 1:
        raise TiffError("LZW: the LSB-first variant of old writers is not supported")
    table: List[bytes] = [bytes([i]) for i in range(256)] + [b"", b""]
    out = bytearray()
    nbits, old, pos, total = 9, None, 0, 8 * len(data)
    while len(out) < n_dst and pos + nbits <= total:
        byte, shift = divmod(pos, 8)
        window = int.from_bytes(data[byte:byte + 3].ljust(3, b"\0"), "big")
        code = (window >> (24 - shift - nbits)) & ((1 << nbits) - 1)
        pos += nbits
        if code == 257:
            break
        if code == 256:
            del table[258:]
            nbits, old = 9, None
            continue
        if old is None:
            if code > 255:
                raise TiffError(f"LZW: code {code} right after a Clear")
            out += table[code]
            old = code
            continue
        if code < len(table):
            entry = table[code]
        elif code == len(table) and len(table) < 4096:
            entry = table[old] + table[old][:1]
        else:
            raise TiffError(f"LZW: code {code} with {len(table)} table entries")
        if len(table) < 4096:
            table.append(table[old] + entry[:1])
        out += entry
        old = code
        if len(table) >= (1 << nbits) - 1 and nbits < 12:
            nbits += 1
    return bytes(out[:n_dst])


def packbits_decode_host(data: bytes, n_dst: int) -> bytes:
    """The statement of fu_tiff_packbits_decode (TIFF 6.0 section 9): header n; 0..127: n + 1 literal bytes; -127..-1: the
    next byte 1 - n times; -128: nothing.  Stops at n_dst bytes; TiffError where a run is cut off by the end of the input."""
    data = bytes(data)
    out = bytearray()
    i = 0
    while i < len(data) and len(out) < n_dst:
        n = data[i] - 256 if data[i] > 127 else data[i]
        i += 1
        if n >= 0:
            if i + n + 1 > len(data):
                raise TiffError("PackBits: literal bytes cut off by the end of the data")
            out += data[i:i + n + 1]
            i += n + 1
        elif n != -128:
            if i >= len(data):
                raise TiffError("PackBits: a run without its byte")
            out += data[i:i + 1] * (1 - n)
            i += 1
    return bytes(out[:n_dst])


_CODEC_ERRORS = {-1: "bad arguments", -2: "corrupt stream", -3: "the LSB-first LZW variant of old writers is not supported"}


def _native_decode(name: str, raw: np.ndarray, dst: np.ndarray) -> int:
    """fu_tiff_lzw_decode / fu_tiff_packbits_decode into dst -> the bytes written."""
    from .. import _lib
    fn = getattr(_lib.load(), name)
    got = int(fn(raw.ctypes.data if raw.size else None, raw.size, dst.ctypes.data if dst.size else None, dst.size))
    if got < 0:
        raise TiffError(f"{name}: {_CODEC_ERRORS.get(got, got)}")
    return got


def _decode_segment(raw: np.ndarray, dst: np.ndarray, scheme: int, codec: str, what: str) -> None:
    """Entropy-decode the stored bytes of one segment into dst, whose length is the segment's nominal size."""
    nominal = dst.size
    if scheme == 1:
        got = min(raw.size, nominal)
        dst[:got] = raw[:got]
    elif scheme in (8, 32946):
        try:
            data = zlib.decompressobj().decompress(raw, nominal)
        except zlib.error as e:
            raise TiffError(f"{what}: Deflate: {e}") from None
        got = len(data)
        dst[:got] = np.frombuffer(data, dtype=np.uint8)
    elif codec == "python":
        data = (lzw_decode_host if scheme == 5 else packbits_decode_host)(raw.tobytes(), nominal)
        got = len(data)
        dst[:got] = np.frombuffer(data, dtype=np.uint8)
    else:
        got = _native_decode("fu_tiff_lzw_decode" if scheme == 5 else "fu_tiff_packbits_decode", raw, dst)
    if got < nominal:
        raise TiffError(f"{what} inflates to {got} bytes, less than its nominal {nominal}")


def _segments(L: dict) -> List[Tuple[int, int, int, int, int]]:
    """(plane, y0, x0, rows, bytes) of every segment at its nominal size, in the order of the file's offset array."""
    planar = bool(L["planar"]) and L["samples"] > 1
    planes, sps = (L["samples"], 1) if planar else (1, L["samples"])
    row_bytes = L["seg_w"] * sps * L["bytes_per_sample"]
    out = []
    for p in range(planes):
        for y0 in range(0, L["height"], L["seg_h"]):
            rows = L["seg_h"] if L["tiled"] else min(L["seg_h"], L["height"] - y0)
            for x0 in range(0, L["width"], L["seg_w"]):
                out.append((p, y0, x0, rows, rows * row_bytes))
    return out


def read_raster_encoded(path: str, decode_threads: int = DECODE_THREADS_DEFAULT, codec: str = "native", ifd: int = 0):
    """-> (the entropy-decoded segments as one contiguous uint8 array, layout): what fu_tiff_unpack / unpack_on_device and
    unpack_host take.  Every segment lies at its nominal size (a tile seg_h x seg_w, strip s min(seg_h, height - s * seg_h)
    rows), back to back in the order of the file's offset array; a segment that decodes to more is truncated, one that
    decodes to less -- or lies beyond the file -- raises TiffError.  layout: the fields of fu_tiff_layout as a dict of ints
    (width, height, samples, bytes_per_sample, sample_kind 1 uint / 2 int / 3 float, big_endian, planar, tiled, seg_w,
    seg_h, predictor).  codec: "native" (the library's LZW / PackBits decoders) or "python" (the statements here).  ifd:
    which image of the file (0: the first; an overview is 1, 2, ...); beyond the chain: TiffError."""
    if codec not in ("native", "python"):
        raise ValueError(f"codec must be 'native' or 'python', got {codec!r}")
    threads = check_decode_threads(decode_threads)
    buf = _map(path)
    info = _describe(*_parse_ifd(buf, ifd=ifd))
    layout = {"width": info["width"], "height": info["height"], "samples": info["samples"],
              "bytes_per_sample": info["bytes_per_sample"], "sample_kind": {"u": 1, "i": 2, "f": 3}[info["kind"]],
              "big_endian": int(info["byteorder"] == ">"), "planar": int(info["planar"] == 2 and info["samples"] > 1),
              "tiled": int(info["tiled"]), "seg_w": info["seg_w"], "seg_h": info["seg_h"], "predictor": info["predictor"]}
    segs = _segments(layout)
    name = "tile" if info["tiled"] else "strip"
    stored = np.frombuffer(buf, dtype=np.uint8)
    starts = np.concatenate([[0], np.cumsum([s[4] for s in segs], dtype=np.int64)])
    enc = np.empty(int(starts[-1]), dtype=np.uint8)
    jobs = []
    for i, (o, n) in enumerate(zip(info["offsets"].tolist(), info["counts"].tolist())):
        if o < 0 or n < 0 or o + n > stored.size:
            raise TiffError(f"{name} {i}: offset {o} + {n} bytes lies beyond the end of the file ({stored.size} bytes)")
        jobs.append((stored[o:o + n], enc[starts[i]:starts[i + 1]], info["compression"], codec, f"{name} {i}"))
    if threads > 1 and len(jobs) > 1 and info["compression"] != 1:
        with ThreadPoolExecutor(max_workers=min(threads, len(jobs))) as pool:
            list(pool.map(lambda j: _decode_segment(*j), jobs))
    else:
        for j in jobs:
            _decode_segment(*j)
    return enc, layout


# ------------------------------------------------------------------------------------------- after the entropy decoder
def _check_layout(layout: dict, n_bytes: int) -> None:
    L = layout
    if L["bytes_per_sample"] not in (1, 2, 4, 8) or L["sample_kind"] not in (1, 2, 3) or L["predictor"] not in (1, 2, 3):
        raise ValueError(f"bad layout {L}")
    if L["predictor"] == 3 and L["sample_kind"] != 3:
        raise ValueError("predictor 3 (floating point) on integer samples")
    if L["predictor"] == 2 and L["sample_kind"] == 3:
        raise ValueError("predictor 2 (horizontal differencing) on floating-point samples")
    if not L["tiled"] and L["seg_w"] != L["width"]:
        raise ValueError("strips are as wide as the image")
    total = sum(s[4] for s in _segments(L))
    if n_bytes != total:
        raise ValueError(f"{n_bytes} bytes, the layout holds {total}")


def unpack_host(encoded: np.ndarray, layout: dict) -> np.ndarray:
    """The numpy statement of everything behind the entropy decoder, and the specification of fu_tiff_unpack: the buffer
    of read_raster_encoded -> the image, with read_tiff's shapes and a native-endian dtype."""
    L = layout
    enc = np.ascontiguousarray(encoded, dtype=np.uint8).reshape(-1)
    _check_layout(L, enc.size)
    W, H, spp, bps = L["width"], L["height"], L["samples"], L["bytes_per_sample"]
    kind = _KINDS[L["sample_kind"]]
    planar = bool(L["planar"]) and spp > 1
    planes, sps = (spp, 1) if planar else (1, spp)
    file_dt = np.dtype(f"{'>' if L['big_endian'] else '<'}{kind}{bps}")
    dt = file_dt.newbyteorder("=")
    seg_w, wc = L["seg_w"], L["seg_w"] * sps
    out = np.empty((planes, H, W, sps), dtype=dt)
    pos = 0
    for p, y0, x0, rows, nbytes in _segments(L):
        seg = enc[pos:pos + nbytes].reshape(rows, wc * bps)
        pos += nbytes
        if L["predictor"] == 3:
            acc = np.cumsum(seg.reshape(rows, bps * seg_w, sps), axis=1, dtype=np.uint8)      # stride sps, modulo 256
            msb_first = np.ascontiguousarray(acc.reshape(rows, bps, wc).transpose(0, 2, 1))   # [row, value, byte]
            vals = msb_first.view(np.dtype(f">{kind}{bps}"))[..., 0].astype(dt)
        else:
            vals = seg.view(file_dt).astype(dt)
            if L["predictor"] == 2:
                u = np.dtype(f"u{bps}")
                vals = np.cumsum(vals.view(u).reshape(rows, seg_w, sps), axis=1, dtype=u).view(dt)   # modulo 2^bits
        vals = vals.reshape(rows, seg_w, sps)
        h, w = min(rows, H - y0), min(seg_w, W - x0)
        out[p, y0:y0 + h, x0:x0 + w] = vals[:h, :w]
    if planar:
        return out[..., 0]
    return out[0, :, :, 0] if spp == 1 else out[0]


def read_raster(path: str, decode_threads: int = DECODE_THREADS_DEFAULT, codec: str = "native", ifd: int = 0) -> np.ndarray:
    """Decode image number `ifd` of the file (0, the default: the first), with read_tiff's return conventions (see the
    module docstring)."""
    return np.ascontiguousarray(unpack_host(*read_raster_encoded(path, decode_threads, codec, ifd)))


def layout_struct(layout: dict):
    from .. import _lib
    return _lib.FuTiffLayout(*[int(layout[name]) for name, _ in _lib.FuTiffLayout._fields_[:-1]], 0)


def unpack_on_device(encoded, layout: dict, bands: Sequence[int], device):
    """C ABI fu_tiff_unpack: the buffer of read_raster_encoded (uint8 array or 1-D uint8 tensor, on the host or already on
    the device) -> fp32 [len(bands), height, width] on the ROCm device, out[n] = sample bands[n]: bit for bit
    np.float32(read_raster(path)) with that band selection.  One upload of the bytes as they are stored (a uint16 scene is
    half the bytes of its fp32 raster) and one launch; no host pass over the samples."""
    import torch

    from .. import _lib
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("unpack_on_device runs only on a ROCm GPU; the host statement is unpack_host")
    enc = encoded if torch.is_tensor(encoded) else torch.from_numpy(np.ascontiguousarray(encoded, dtype=np.uint8))
    if enc.dtype != torch.uint8 or enc.dim() != 1:
        raise ValueError(f"unpack_on_device: encoded must be 1-D uint8, got {tuple(enc.shape)} {enc.dtype}")
    bands = [int(b) for b in bands]
    if not 1 <= len(bands) <= UNPACK_MAX_BANDS:
        raise ValueError(f"unpack_on_device: {len(bands)} bands, 1..{UNPACK_MAX_BANDS} are supported")
    enc = enc.contiguous().to(dev, non_blocking=True)
    out = torch.empty(len(bands), int(layout["height"]), int(layout["width"]), dtype=torch.float32, device=dev)
    import ctypes
    table = (ctypes.c_int32 * len(bands))(*bands)
    _lib.check(_lib.load().fu_tiff_unpack(_lib.ptr(enc), enc.numel(), layout_struct(layout), table, len(bands), _lib.ptr(out),
                                          torch.cuda.current_stream(dev).cuda_stream))
    return out
