"""InferOptions: the options of label-free scene inference (infer.infer) as one checked value.

The command line (from_args) and infer()'s keywords both build one through InferOptions.make, which performs every check
that needs no config; what depends on the model's crop size -- the default stride, the batch size, the view codes of
test-time augmentation -- is filled in by resolve().  infer() reads the options and decides nothing about them itself.
predict() shares check_weights, check_blend and tta.view_codes.  A new option is one field here, its keyword and check
in make, and one flag in infer.build_parser.  Host arithmetic only: neither torch nor the GPU library is imported.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence, Tuple, Union

WEIGHT_CHOICES = ("auto", "raw", "ema")          # predict.checkpoint_weights
BLEND_KINDS = ("uniform", "linear", "hann")      # stitch.blend_window
PROB_FORMATS = ("u8", "f32")
# the keywords of InferOptions.make, which are infer()'s option keywords and, but for keep_probabilities, its flags
KEYWORDS = ("size", "scale", "stride", "batch_size", "tta", "n_workers", "device", "keep_probabilities", "weights",
            "blend", "write_probs", "write_margin", "sieve", "sieve_connectivity", "sieve_passes", "water_threshold",
            "threshold_class", "calibration", "nodata", "nodata_out", "skip_empty", "write_valid", "decode",
            "decode_threads", "write_vectors", "vector_values", "vector_connectivity", "vector_max_edges", "out_compress",
            "out_level", "out_predictor", "out_tile", "out_bigtiff", "out_threads", "out_overviews", "out_cog")
NODATA_OUT_DEFAULT = 127                         # the class map's byte where the input holds no data
DECODE_CHOICES = ("auto", "host", "device")      # how a scene's samples reach the device (infer.SceneFiles)
DECODE_THREADS_DEFAULT, DECODE_THREADS_MAX = 4, 16   # datasets/geotiff.py's; never sized from the machine's CPU count
VECTOR_MAX_EDGES_DEFAULT = 1 << 24               # a scene with more crack edges gets no polygons (vectorize.py)
OUT_COMPRESS_CHOICES = ("none", "deflate")       # how the output rasters are written (datasets/geotiff_write.py)
OUT_PREDICTOR_CHOICES = ("auto", "off")
OUT_BIGTIFF_CHOICES = ("auto", "yes", "no")
OUT_LEVEL_DEFAULT, OUT_THREADS_DEFAULT, OUT_THREADS_MAX, OUT_TILE_FLAG = 6, 4, 16, 256
OUT_TILE_STRIPS = "strips"                       # out_tile: strips, said explicitly (None says so by default)
OUT_TILE_COG = 512                               # the tile side --out_cog chooses unless --out_tile gives one


def check_weights(weights) -> str:
    if weights not in WEIGHT_CHOICES:
        raise ValueError(f"weights must be one of {list(WEIGHT_CHOICES)}, got {weights!r}")
    return weights


def check_blend(blend) -> str:
    if blend not in BLEND_KINDS:
        raise ValueError(f"blend must be one of {list(BLEND_KINDS)}, got {blend!r}")
    return blend


def check_write_probs(write_probs) -> Optional[str]:
    if write_probs is not None and write_probs not in PROB_FORMATS:
        raise ValueError(f"write_probs must be one of {list(PROB_FORMATS)} or None, got {write_probs!r}")
    return write_probs


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


def check_nodata(nodata) -> Union[None, str, float]:
    """--nodata: None (off), "auto" (the input's GDAL_NODATA tag, else 0) or a finite number (also as a string)."""
    if nodata is None or nodata == "auto":
        return nodata
    try:
        value = float(nodata)
    except (TypeError, ValueError):
        raise ValueError(f"infer: nodata must be 'auto' or a finite number, got {nodata!r}") from None
    if isinstance(nodata, bool) or value != value or value in (float("inf"), float("-inf")):
        raise ValueError(f"infer: nodata must be 'auto' or a finite number, got {nodata!r}")
    return value


def scene_nodata(nodata: Union[str, float], tags: dict) -> float:
    """The value a scene's mask is taken with: the option's number, or under "auto" the scene's GDAL_NODATA tag (42113)
    when it parses as a finite float, else 0."""
    if nodata != "auto":
        return float(nodata)
    tag = tags.get(42113) if tags else None
    if isinstance(tag, bytes):
        tag = tag.decode("ascii", "replace")
    try:
        value = float(str(tag).strip().strip("\x00").strip()) if tag is not None else 0.0
    except ValueError:
        return 0.0
    return value if value == value and value not in (float("inf"), float("-inf")) else 0.0


def check_decode(decode, decode_threads) -> Tuple[str, int]:
    """--decode auto|host|device and --decode_threads 1..16 (the segment decoders' thread pool)."""
    if decode not in DECODE_CHOICES:
        raise ValueError(f"infer: decode must be one of {list(DECODE_CHOICES)}, got {decode!r}")
    if isinstance(decode_threads, bool) or not isinstance(decode_threads, (int, float)) or \
            int(decode_threads) != decode_threads or not 1 <= int(decode_threads) <= DECODE_THREADS_MAX:
        raise ValueError(f"infer: decode_threads must be an integer in 1..{DECODE_THREADS_MAX}, got {decode_threads!r}")
    return decode, int(decode_threads)


def check_vectors(write_vectors, vector_values, vector_connectivity, vector_max_edges, sieve, nodata_out) -> Optional[dict]:
    """--write_vectors and its options -> None (off) or the four vector fields.  vector_values: the class-map values that
    get polygons, default every written class value except 0 and nodata_out, which is [255]; vector_connectivity: 4 or 8,
    default the sieve's when the run sieves, else 4; vector_max_edges: default 2^24."""
    given = [name for name, v in (("--vector_values", vector_values), ("--vector_connectivity", vector_connectivity),
                                  ("--vector_max_edges", vector_max_edges)) if v is not None]
    if not write_vectors:
        if given:
            raise ValueError(f"infer: {', '.join(given)} need{'s' if len(given) == 1 else ''} --write_vectors")
        return None
    values = [255] if vector_values is None else list(vector_values)
    for v in values:
        if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or not 0 <= int(v) <= 255:
            raise ValueError(f"infer: vector_values must be integers in 0..255, got {v!r}")
    if vector_connectivity is None:
        vector_connectivity = sieve[1] if sieve is not None else 4
    if vector_connectivity not in (4, 8):
        raise ValueError(f"infer: vector_connectivity must be 4 or 8, got {vector_connectivity!r}")
    if vector_max_edges is None:
        vector_max_edges = VECTOR_MAX_EDGES_DEFAULT
    if isinstance(vector_max_edges, bool) or int(vector_max_edges) != vector_max_edges or int(vector_max_edges) < 0:
        raise ValueError(f"infer: vector_max_edges must be an integer >= 0, got {vector_max_edges!r}")
    return dict(write_vectors=True, vector_values=tuple(sorted({int(v) for v in values})),
                vector_connectivity=int(vector_connectivity), vector_max_edges=int(vector_max_edges))


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float)) and int(v) == v


def check_output(out_compress, out_level, out_predictor, out_tile, out_bigtiff, out_threads) -> Optional[dict]:
    """The six output-format options -> None (every one at its default: the rasters are written as they always were) or
    the six fields.  out_compress: "none" or "deflate"; out_level: zlib's 1..9, needs deflate; out_predictor: "auto" (under
    deflate 2 for the uint8 rasters and 3 for fp32, else 1) or "off"; out_tile: None (strips) or the tile side, a multiple
    of 16; out_bigtiff: "auto" (BigTIFF only where classic TIFF cannot hold the file), "yes" or "no"; out_threads: the
    deflate thread pool, 1..16."""
    if out_compress not in OUT_COMPRESS_CHOICES:
        raise ValueError(f"infer: out_compress must be one of {list(OUT_COMPRESS_CHOICES)}, got {out_compress!r}")
    if not _is_int(out_level) or not 1 <= int(out_level) <= 9:
        raise ValueError(f"infer: out_level must be an integer in 1..9, got {out_level!r}")
    if out_compress != "deflate" and int(out_level) != OUT_LEVEL_DEFAULT:
        raise ValueError("infer: --out_level needs --out_compress deflate")
    if out_predictor not in OUT_PREDICTOR_CHOICES:
        raise ValueError(f"infer: out_predictor must be one of {list(OUT_PREDICTOR_CHOICES)}, got {out_predictor!r}")
    if out_tile is not None and (not _is_int(out_tile) or int(out_tile) < 16 or int(out_tile) % 16):
        raise ValueError(f"infer: out_tile must be a multiple of 16 that is at least 16, got {out_tile!r}")
    if out_bigtiff not in OUT_BIGTIFF_CHOICES:
        raise ValueError(f"infer: out_bigtiff must be one of {list(OUT_BIGTIFF_CHOICES)}, got {out_bigtiff!r}")
    if not _is_int(out_threads) or not 1 <= int(out_threads) <= OUT_THREADS_MAX:
        raise ValueError(f"infer: out_threads must be an integer in 1..{OUT_THREADS_MAX}, got {out_threads!r}")
    fields = dict(out_compress=out_compress, out_level=int(out_level), out_predictor=out_predictor,
                  out_tile=None if out_tile is None else int(out_tile), out_bigtiff=out_bigtiff, out_threads=int(out_threads))
    if fields == _OUTPUT_DEFAULTS:
        return None
    return fields


_OUTPUT_DEFAULTS = dict(out_compress="none", out_level=OUT_LEVEL_DEFAULT, out_predictor="auto", out_tile=None,
                        out_bigtiff="auto", out_threads=OUT_THREADS_DEFAULT)


def check_overviews(out_overviews, out_cog, out_tile):
    """--out_overviews auto|N and the preset --out_cog -> (the two pyramid fields or None when neither is given, out_tile
    as check_output takes it).  out_overviews: None (no overview images), "auto" (levels until the smallest fits one tile,
    or 256 pixels for strips: overviews.auto_levels) or an integer >= 0 (also as a string; clamped per scene to the levels
    down to 1 x 1).  out_cog: tiles of 512 unless out_tile gives the side, overviews "auto" unless given; it excludes an
    explicit strip layout (out_tile "strips")."""
    if out_overviews is not None and out_overviews != "auto":
        try:
            n = int(out_overviews) if isinstance(out_overviews, str) else out_overviews
        except ValueError:
            n = None
        if n is None or not _is_int(n) or int(n) < 0:
            raise ValueError(f"infer: out_overviews must be 'auto' or an integer >= 0, got {out_overviews!r}")
        out_overviews = int(n)
    strips = isinstance(out_tile, str) and out_tile == OUT_TILE_STRIPS
    if strips:
        out_tile = None
    if out_cog:
        if strips:
            raise ValueError("infer: --out_cog writes tiles; it excludes --out_tile strips")
        if out_tile is None:
            out_tile = OUT_TILE_COG
        if out_overviews is None:
            out_overviews = "auto"
    if out_overviews is None:
        return None, out_tile
    return dict(out_overviews=out_overviews, out_cog=bool(out_cog)), out_tile


@dataclasses.dataclass(frozen=True)
class InferOptions:
    """size / scale: the output grid (grid_size); None, None: the raster's own.  stride and batch_size None: the
    default_stride of the crop and the config's batch size, set by resolve().  tta: None, a tta.VIEW_SETS name or a
    tuple of view codes; codes: its checked codes, set by resolve().  sieve: None or (min pixels, connectivity,
    passes).  threshold: None (the argmax) or (class, threshold, source), threshold_rule's dict as a tuple.
    A run without --nodata is this value, field for field what it always was; its four nodata attributes are the class
    constants below (off).  A run with --nodata is a NodataInferOptions, which appends them as fields.  Likewise decode
    ("auto": a file the strict TIFF reader takes goes the way it always went, every other file is unpacked on the
    device) and decode_threads: class constants here, fields of DecodeInferOptions / NodataDecodeInferOptions when either
    differs from its default.  And write_vectors with vector_values, vector_connectivity and vector_max_edges: off here,
    fields of the Vector* classes under --write_vectors.  And the six out_* options of the output format: the defaults
    here (the rasters go through write_strip_tiff, byte for byte as always), fields of output_options_class(...) when any
    is set; packed_output says which.  And out_overviews / out_cog, the overview images behind every written raster: off
    here, fields of overview_options_class(...) -- the Output* class of the run with the two appended -- when either is
    given; such a run is a packed-output run."""
    size: Optional[Tuple[int, int]] = None
    scale: Optional[float] = None
    stride: Optional[int] = None
    batch_size: Optional[int] = None
    tta: Union[None, str, Tuple[int, ...]] = None
    weights: str = "auto"
    blend: str = "uniform"
    write_probs: Optional[str] = None
    write_margin: bool = False
    sieve: Optional[Tuple[int, int, int]] = None
    threshold: Optional[Tuple[int, float, str]] = None
    keep_probabilities: bool = False
    n_workers: int = 0
    device: str = "cuda:0"
    codes: Optional[Tuple[int, ...]] = None
    nodata = None                        # not fields here: see NodataInferOptions
    nodata_out = NODATA_OUT_DEFAULT
    skip_empty = True
    write_valid = False
    decode = "auto"                      # not fields here: see DecodeInferOptions
    decode_threads = DECODE_THREADS_DEFAULT
    write_vectors = False                # not fields here: see vector_options_class
    vector_values = (255,)
    vector_connectivity = 4
    vector_max_edges = VECTOR_MAX_EDGES_DEFAULT
    out_compress = "none"                # not fields here: see output_options_class
    out_level = OUT_LEVEL_DEFAULT
    out_predictor = "auto"
    out_tile = None
    out_bigtiff = "auto"
    out_threads = OUT_THREADS_DEFAULT
    out_overviews = None                 # not fields here: see overview_options_class
    out_cog = False
    packed_output = False                # True on the Output* classes: the rasters are packed on the device and go
    #                                      through geotiff_write.write_raster

    @classmethod
    def make(cls, *, size=None, scale=None, stride=None, batch_size=None, tta=None, n_workers=0, device="cuda:0",
             keep_probabilities=False, weights="auto", blend="uniform", write_probs=None, write_margin=False, sieve=None,
             sieve_connectivity=4, sieve_passes=1, water_threshold=None, threshold_class=None,
             calibration=None, nodata=None, nodata_out=NODATA_OUT_DEFAULT, skip_empty=True,
             write_valid=False, decode="auto", decode_threads=DECODE_THREADS_DEFAULT, write_vectors=False,
             vector_values=None, vector_connectivity=None, vector_max_edges=None, out_compress="none",
             out_level=OUT_LEVEL_DEFAULT, out_predictor="auto", out_tile=None, out_bigtiff="auto",
             out_threads=OUT_THREADS_DEFAULT, out_overviews=None, out_cog=False) -> "InferOptions":
        """The options checked, in the order infer() always checked them: weights, blend, write_probs, the decision
        rule (threshold_rule), the sieve (postprocess.check_sieve_options), an explicit stride, the grid, nodata, decode,
        vectors, the overviews (which can choose the tile side), the output format."""
        from .postprocess import check_sieve_options
        check_weights(weights)
        check_blend(blend)
        check_write_probs(write_probs)
        rule = threshold_rule(water_threshold, threshold_class, calibration)
        if sieve is not None:
            check_sieve_options(sieve, sieve_connectivity, sieve_passes)
            sieve = (int(sieve), int(sieve_connectivity), int(sieve_passes))
        if stride is not None and int(stride) < 1:
            raise ValueError(f"infer: stride must be >= 1, got {int(stride)}")
        if size is not None or scale is not None:
            grid_size((1 << 20, 1 << 20), size, scale)
        nodata = check_nodata(nodata)
        if isinstance(nodata_out, bool) or int(nodata_out) != nodata_out or not 1 <= int(nodata_out) <= 254:
            raise ValueError(f"infer: nodata_out must be an integer in 1..254, got {nodata_out!r}")
        if nodata is None and (int(nodata_out) != NODATA_OUT_DEFAULT or not skip_empty or write_valid):
            raise ValueError("infer: --nodata_out, --keep_empty_crops and --write_valid need --nodata")
        extra = {}
        if nodata is not None:
            cls, extra = NodataInferOptions, dict(nodata=nodata, nodata_out=int(nodata_out), skip_empty=bool(skip_empty),
                                                  write_valid=bool(write_valid))
        decode, decode_threads = check_decode(decode, decode_threads)
        if (decode, decode_threads) != ("auto", DECODE_THREADS_DEFAULT):
            cls = NodataDecodeInferOptions if nodata is not None else DecodeInferOptions
            extra.update(decode=decode, decode_threads=decode_threads)
        vectors = check_vectors(write_vectors, vector_values, vector_connectivity, vector_max_edges, sieve, nodata_out)
        if vectors is not None:
            cls = vector_options_class(cls)
            extra.update(vectors)
        pyramid, out_tile = check_overviews(out_overviews, out_cog, out_tile)
        output = check_output(out_compress, out_level, out_predictor, out_tile, out_bigtiff, out_threads)
        if output is not None or pyramid is not None:        # a run with overviews is a packed-output run
            cls = output_options_class(cls)
            extra.update(output or _OUTPUT_DEFAULTS)
        if pyramid is not None:
            cls = overview_options_class(cls)
            extra.update(pyramid)
        return cls(size=None if size is None else (int(size[0]), int(size[1])), scale=scale,
                   stride=None if stride is None else int(stride), batch_size=int(batch_size) if batch_size else None,
                   tta=tta if tta is None or isinstance(tta, str) else tuple(int(c) for c in tta), weights=weights,
                   blend=blend, write_probs=write_probs, write_margin=bool(write_margin), sieve=sieve,
                   threshold=None if rule is None else (rule["class"], rule["threshold"], rule["source"]),
                   keep_probabilities=bool(keep_probabilities), n_workers=int(n_workers), device=str(device),
                   **extra)

    @classmethod
    def from_args(cls, args) -> "InferOptions":
        """The options an infer command line gave (infer.build_parser); keep_probabilities has no flag."""
        return cls.make(**{k: getattr(args, k) for k in KEYWORDS if k != "keep_probabilities"})

    def resolve(self, crop_height: int, crop_width: int, batch_size: Optional[int] = None) -> "InferOptions":
        """The options for a model of crop_height x crop_width crops whose config has batch_size: stride and batch_size
        filled in where they were left open, codes = tta.view_codes of tta (the d4 set needs square crops)."""
        from .tta import view_codes
        ch, cw = int(crop_height), int(crop_width)
        codes = view_codes(self.tta, ch, cw) if self.tta is not None else None
        return dataclasses.replace(self, stride=default_stride(ch, cw, self.blend, self.stride),
                                   batch_size=int(self.batch_size or batch_size), codes=codes)

    def check_classes(self, n_classes: int) -> None:
        """The threshold's class against the served model's class count."""
        if self.threshold is not None and self.threshold[0] >= n_classes:
            raise ValueError(f"infer: threshold class {self.threshold[0]} not in 0..{n_classes - 1}")

    def grid(self, src_hw: Tuple[int, int]) -> Tuple[int, int]:
        return grid_size(src_hw, self.size, self.scale)

    @property
    def n_views(self) -> int:
        return len(self.codes) if self.codes is not None else 1

    @property
    def rule(self) -> Optional[dict]:
        """threshold as threshold_rule returns it, the summary's "threshold"."""
        return None if self.threshold is None else dict(zip(("class", "threshold", "source"), self.threshold))

    @property
    def sieve_options(self) -> Optional[dict]:
        """sieve under the names of the summary's "sieve"."""
        return None if self.sieve is None else dict(zip(("min_pixels", "connectivity", "passes"), self.sieve))

    def predictor_for(self, dtype) -> int:
        """The TIFF predictor of an output raster of this sample type: under out_predictor "auto" with deflate 2 for
        integers and 3 for floats, else 1."""
        if self.out_compress != "deflate" or self.out_predictor == "off":
            return 1
        import numpy as np
        return 3 if np.dtype(dtype).kind == "f" else 2

    def output_format(self, bigtiff, overviews=None, cog=None) -> dict:
        """The records' and the summary's "output_format"; bigtiff: whether the file, or any file of the run, is BigTIFF.
        A run with overviews also records "overviews", the overview images written per file (the summary: the most any
        scene got), and "cog": the preset was asked for and geotiff.cog_report of every written file is empty."""
        fmt = {"compress": self.out_compress, "level": self.out_level if self.out_compress == "deflate" else None,
               "predictor": self.out_predictor, "tile": self.out_tile, "bigtiff": bigtiff, "threads": self.out_threads}
        if self.out_overviews is not None:
            fmt.update(overviews=overviews, cog=bool(cog))
        return fmt

    def overview_levels(self, hw: Tuple[int, int]) -> int:
        """The overview images a raster of hw gets: 0 without out_overviews; under "auto" the levels until the smallest
        fits one tile (256 pixels for strips); else the count asked for, clamped to the levels down to 1 x 1."""
        if self.out_overviews is None:
            return 0
        from .datasets.overviews import STRIP_SIDE, auto_levels, max_levels
        if self.out_overviews == "auto":
            return auto_levels(hw[0], hw[1], self.out_tile or STRIP_SIDE)
        return min(self.out_overviews, max_levels(hw[0], hw[1]))


@dataclasses.dataclass(frozen=True)
class NodataInferOptions(InferOptions):
    """InferOptions of a run with --nodata: the four nodata options appended after codes.  nodata: "auto" or a finite
    float (scene_nodata gives a scene's value); nodata_out: the class map's value where the input holds no data, in
    1..254; skip_empty: crops without a valid pixel are not forwarded; write_valid: also write <image>_valid.tif.
    InferOptions.make builds it when nodata is given; resolve() keeps it."""
    nodata: Union[None, str, float] = None
    nodata_out: int = NODATA_OUT_DEFAULT
    skip_empty: bool = True
    write_valid: bool = False


@dataclasses.dataclass(frozen=True)
class DecodeInferOptions(InferOptions):
    """InferOptions of a run whose --decode or --decode_threads is not the default, appended after codes.  decode: "auto",
    "host" (datasets/geotiff.py's numpy statement for every file) or "device" (every file through fu_tiff_unpack);
    decode_threads: the segment decoders' thread pool, 1..16."""
    decode: str = "auto"
    decode_threads: int = DECODE_THREADS_DEFAULT


@dataclasses.dataclass(frozen=True)
class NodataDecodeInferOptions(NodataInferOptions):
    """Both: the nodata fields, then the decode fields."""
    decode: str = "auto"
    decode_threads: int = DECODE_THREADS_DEFAULT


def vector_options_class(base):
    """The options class of a run with --write_vectors: `base` (any of the four above) with the four vector fields appended.
    write_vectors: True; vector_values: the class-map values that get polygons, sorted; vector_connectivity: 4 or 8;
    vector_max_edges: a scene with more crack edges gets no polygons."""
    return _VECTOR_CLASSES[base]


def _vector_class(base):
    cls = dataclasses.make_dataclass(
        "Vector" + base.__name__, [("write_vectors", bool, False), ("vector_values", Tuple[int, ...], (255,)),
                                   ("vector_connectivity", int, 4), ("vector_max_edges", int, VECTOR_MAX_EDGES_DEFAULT)],
        bases=(base,), frozen=True)
    cls.__module__ = __name__
    cls.__doc__ = f"{base.__name__} of a run with --write_vectors: the four vector fields appended (vector_options_class)."
    return cls


VectorInferOptions = _vector_class(InferOptions)
VectorNodataInferOptions = _vector_class(NodataInferOptions)
VectorDecodeInferOptions = _vector_class(DecodeInferOptions)
VectorNodataDecodeInferOptions = _vector_class(NodataDecodeInferOptions)
_VECTOR_CLASSES = {InferOptions: VectorInferOptions, NodataInferOptions: VectorNodataInferOptions,
                   DecodeInferOptions: VectorDecodeInferOptions, NodataDecodeInferOptions: VectorNodataDecodeInferOptions}


def output_options_class(base):
    """The options class of a run with an out_* option set: `base` (any of the eight above) with the six output-format
    fields appended.  out_compress: "none" or "deflate"; out_level: 1..9; out_predictor: "auto" or "off"; out_tile: None
    or the tile side; out_bigtiff: "auto", "yes" or "no"; out_threads: 1..16."""
    return _OUTPUT_CLASSES[base]


def _output_class(base):
    cls = dataclasses.make_dataclass(
        "Output" + base.__name__, [("out_compress", str, "none"), ("out_level", int, OUT_LEVEL_DEFAULT),
                                   ("out_predictor", str, "auto"), ("out_tile", Optional[int], None),
                                   ("out_bigtiff", str, "auto"), ("out_threads", int, OUT_THREADS_DEFAULT)],
        bases=(base,), namespace={"packed_output": True}, frozen=True)
    cls.__module__ = __name__
    cls.__doc__ = f"{base.__name__} of a run with an out_* option set: the six fields appended (output_options_class)."
    globals()[cls.__name__] = cls
    return cls


_OUTPUT_CLASSES = {base: _output_class(base) for base in (InferOptions, NodataInferOptions, DecodeInferOptions,
                                                          NodataDecodeInferOptions) + tuple(_VECTOR_CLASSES.values())}


def overview_options_class(base):
    """The options class of a run with --out_overviews or --out_cog: `base` (any of the Output* classes) with the two
    pyramid fields appended.  out_overviews: "auto" or the number of overview images; out_cog: the preset was asked for,
    and the records say whether the written files follow the cloud-optimised layout."""
    return _OVERVIEW_CLASSES[base]


def _overview_class(base):
    cls = dataclasses.make_dataclass(
        "Overview" + base.__name__, [("out_overviews", Union[str, int], "auto"), ("out_cog", bool, False)], bases=(base,),
        frozen=True)
    cls.__module__ = __name__
    cls.__doc__ = f"{base.__name__} of a run with overviews: the two pyramid fields appended (overview_options_class)."
    globals()[cls.__name__] = cls
    return cls


_OVERVIEW_CLASSES = {base: _overview_class(base) for base in _OUTPUT_CLASSES.values()}
