"""CPU: datasets/geotiff_write.py -- the byte layout in front of the entropy coder (pack_host against its inverse
geotiff.unpack_host and against answers written out by hand), the container (write_raster read back through geotiff.py:
compression, tiles, BigTIFF, the auto switch, thread-count independence, size), the out_* options of infer, and the default
route of write_scene, which stays write_strip_tiff byte for byte."""
import dataclasses
import itertools
import os

import numpy as np
import pytest

from floodplanet_code_amd.datasets import geotiff as G
from floodplanet_code_amd.datasets import geotiff_write as GW
from floodplanet_code_amd.datasets.synthetic import write_strip_tiff
from floodplanet_code_amd.datasets.tiff import TiffError
from floodplanet_code_amd.infer_options import KEYWORDS, InferOptions

SIZES = [(1, 1), (5, 3), (16, 16), (17, 33), (40, 70)]
DTYPES = ["u1", "u2", "i4", "f4"]
SOURCES = ["khw", "hwk", "padded"]
# NaNs with payloads (quiet and signalling, both signs), -0.0, the infinities, the largest and smallest denormal, and values
# whose neighbouring bytes wrap under the byte-wise difference
SPECIAL_F32 = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff80ffff, 0x80000000, 0x7f800000, 0xff800000, 0x007fffff,
                        0x00000001, 0x80000001, 0x00ff00ff, 0xff00ff00], dtype=np.uint32)


def segment_choices(H):
    """(tiled, seg_h, seg_w or None for the image's width)"""
    return [(1, 16, 16), (1, 32, 16)] + [(0, r, None) for r in (1, 7, 16, H + 5)]


def predictors(dtype):
    return (1, 3) if dtype == "f4" else (1, 2)


def make_array(dtype, k, H, W, source="khw", seed=0):
    """Random bits of the type as [k, H, W] ([H, W] for k = 1) over the memory order `source`: contiguous [k, H, W], a
    transposed view of a contiguous [H, W, k], or a view of rows padded by 5 samples.  float32 starts with SPECIAL_F32."""
    dt = np.dtype(dtype)
    g = np.random.default_rng(seed + 1000 * H + 10 * W + k)
    bits = g.integers(0, 1 << (8 * dt.itemsize), size=(k, H, W), dtype=np.uint64).astype(np.dtype(f"u{dt.itemsize}"))
    if dtype == "f4":
        flat = bits.reshape(-1)
        n = min(flat.size, SPECIAL_F32.size)
        flat[:n] = SPECIAL_F32[:n]
    a = bits.view(dt)
    if source == "hwk":
        a = np.ascontiguousarray(a.transpose(1, 2, 0)).transpose(2, 0, 1)
    elif source == "padded":
        wide = np.zeros((k, H, W + 5), dtype=dt)
        wide[:, :, :W] = a
        a = wide[:, :, :W]
    else:
        a = np.ascontiguousarray(a)
    return a if k > 1 else a[0]


def make_layout(dtype, k, H, W, seg, predictor):
    L = GW.raster_layout(dtype, H, W, k, predictor=predictor)
    tiled, seg_h, seg_w = seg
    L.update(tiled=tiled, seg_h=seg_h, seg_w=W if seg_w is None else seg_w)
    return L


def grid(dtype):
    """Every case of the round-trip grid for one sample type: (k, H, W, seg, predictor, source)."""
    for (H, W), k, p, source in itertools.product(SIZES, (1, 3), predictors(dtype), SOURCES):
        for seg in segment_choices(H):
            yield k, H, W, seg, p, source


def bits(a):
    return np.ascontiguousarray(a).view(np.dtype(f"u{a.dtype.itemsize}"))


# --------------------------------------------------------------------------------------------------------- the statement
@pytest.mark.parametrize("dtype", DTYPES)
def test_unpack_of_pack_is_the_array_bit_for_bit(dtype):
    n = 0
    for k, H, W, seg, p, source in grid(dtype):
        a = make_array(dtype, k, H, W, source)
        L = make_layout(dtype, k, H, W, seg, p)
        packed = GW.pack_host(a, L)
        assert packed.dtype == np.uint8 and packed.shape == (GW.check_pack_layout(L),)
        back = G.unpack_host(packed, L)
        assert back.shape == a.shape and back.dtype == a.dtype, (k, H, W, seg, p, source)
        assert np.array_equal(bits(back), bits(a)), (k, H, W, seg, p, source)
        n += 1
    assert n == len(SIZES) * 2 * 2 * len(SOURCES) * 6


def test_the_sources_pack_to_the_same_bytes():
    for dtype in DTYPES:
        L = make_layout(dtype, 3, 17, 33, (1, 16, 16), predictors(dtype)[1])
        want = GW.pack_host(make_array(dtype, 3, 17, 33, "khw"), L)
        for source in SOURCES[1:]:
            assert np.array_equal(GW.pack_host(make_array(dtype, 3, 17, 33, source), L), want)


def test_known_answer_uint8_row_under_predictor_2():
    a = np.array([[10, 13, 250, 3]], dtype=np.uint8)
    L = GW.raster_layout("u1", 1, 4, predictor=2)
    assert GW.pack_host(a, L).tolist() == [10, 3, 237, 9]                 # 250 - 13, and 3 - 250 modulo 256


def test_known_answer_float32_row_under_predictor_3_carries_across_the_planes():
    a = np.array([[0x11223344, 0x55667788]], dtype=np.uint32).view(np.float32)
    L = GW.raster_layout("f4", 1, 2, predictor=3)
    # byte planes, most significant first: 11 55 | 22 66 | 33 77 | 44 88; each byte minus the one in front of it, also
    # where a plane starts: 0x22 - 0x55 = 0xcd, 0x33 - 0x66 = 0xcd, 0x44 - 0x77 = 0xcd
    assert GW.pack_host(a, L).tolist() == [0x11, 0x44, 0xcd, 0x44, 0xcd, 0x44, 0xcd, 0x44]


def test_known_answer_edge_tile_is_padded_by_replication():
    a = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=np.uint8)
    L = GW.raster_layout("u1", 3, 3, tile=16)
    tile = GW.pack_host(a, L).reshape(16, 16)
    want = np.empty((16, 16), dtype=np.uint8)
    want[:3, :3] = a
    want[:3, 3:] = a[:, 2:3]                                              # the last column, repeated
    want[3:, :3] = a[2:3, :]                                              # the last row, repeated
    want[3:, 3:] = 9                                                      # the corner
    assert np.array_equal(tile, want)
    L2 = dict(L, predictor=2)                                             # padded before the predictor: runs of zeros
    d = GW.pack_host(a, L2).reshape(16, 16)
    assert d[0].tolist() == [1, 1, 1] + [0] * 13 and d[5].tolist() == [7, 1, 1] + [0] * 13


def test_unsupported_layouts_are_rejected():
    a = np.zeros((3, 4, 4), dtype=np.uint8)
    good = GW.raster_layout("u1", 4, 4, 3)
    for change, msg in ((dict(planar=0), "chunky"), (dict(big_endian=1), "big-endian"), (dict(predictor=3), "predictor 3"),
                        (dict(tiled=1, seg_w=24, seg_h=16), "multiples of 16"), (dict(seg_w=3), "as wide as"),
                        (dict(bytes_per_sample=8), "bad layout"), (dict(samples=17), "samples")):
        with pytest.raises(ValueError, match=msg):
            GW.pack_host(a, dict(good, **change))
    with pytest.raises(ValueError, match="predictor 2"):
        GW.pack_host(np.zeros((4, 4), dtype=np.float32), GW.raster_layout("f4", 4, 4, predictor=2))
    with pytest.raises(ValueError, match="layout describes"):
        GW.pack_host(np.zeros((4, 4), dtype=np.uint16), GW.raster_layout("u1", 4, 4))


# ------------------------------------------------------------------------------------------------------------- the files
GEO = [(33550, 12, [10.0, 10.0, 0.0]), (33922, 12, [0.0, 0.0, 0.0, 500000.0, 4000000.0, 0.0]),
       (34735, 3, [1, 1, 0, 1, 1024, 0, 1, 1]), (34737, 2, "WGS 84 / UTM zone 33N|"), (42113, 2, "127")]
GEO_READ = {33550: (10.0, 10.0, 0.0), 33922: (0.0, 0.0, 0.0, 500000.0, 4000000.0, 0.0),
            34735: (1, 1, 0, 1, 1024, 0, 1, 1), 34737: "WGS 84 / UTM zone 33N|", 42113: "127"}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("big", ["auto", "yes"], ids=["classic", "bigtiff"])
@pytest.mark.parametrize("tile", [None, 16], ids=["strips", "tiles"])
@pytest.mark.parametrize("compress", ["none", "deflate"])
def test_files_read_back_with_their_tags_and_header(compress, tile, big, dtype, tmp_path):
    path = str(tmp_path / "r.tif")
    for k in (1, 3):
        a = make_array(dtype, k, 40, 70)
        predictor = predictors(dtype)[1] if compress == "deflate" else 1
        L = GW.raster_layout(dtype, 40, 70, k, tile=tile, rows_per_strip=7, predictor=predictor)
        res = GW.write_raster(path, a, L, compress=compress, bigtiff=big, extra_tags=GEO)
        assert res["bigtiff"] == (big == "yes") and res["size"] == os.path.getsize(path)
        back = G.read_raster(path)
        assert back.shape == a.shape and back.dtype == a.dtype and np.array_equal(bits(back), bits(a))
        assert G.raster_geotiff_tags(path) == GEO_READ
        info = G.raster_info(path)
        assert info["compression"] == (8 if compress == "deflate" else 1) and info["predictor"] == predictor
        assert info["tiled"] == (tile is not None) and info["bigtiff"] == (big == "yes")
        assert (info["seg_h"], info["seg_w"]) == ((16, 16) if tile else (7, 70)) and info["samples"] == k
        assert info["planar"] == (2 if k > 1 else 1) and info["byteorder"] == "<"
        assert G.strict_reader_accepts(path) == (compress == "none" and tile is None and big == "auto")
        # the packed bytes are taken as they are
        res2 = GW.write_raster(str(tmp_path / "p.tif"), GW.pack_host(a, L), L, compress=compress, bigtiff=big,
                               extra_tags=GEO)
        assert res2 == res and open(path, "rb").read() == open(tmp_path / "p.tif", "rb").read()


def test_uncompressed_classic_strips_are_write_strip_tiff_byte_for_byte(tmp_path):
    a = make_array("f4", 3, 40, 70)
    write_strip_tiff(str(tmp_path / "a.tif"), a, extra_tags=GEO)
    GW.write_raster(str(tmp_path / "b.tif"), a, GW.raster_layout("f4", 40, 70, 3), extra_tags=GEO)
    assert open(tmp_path / "a.tif", "rb").read() == open(tmp_path / "b.tif", "rb").read()


def test_bigtiff_auto_switches_at_the_classic_limit(tmp_path):
    small, large = np.zeros((8, 8), dtype=np.uint8), make_array("u1", 1, 40, 70)
    for a, want in ((small, False), (large, True)):
        path = str(tmp_path / "x.tif")
        L = GW.raster_layout("u1", *a.shape)
        res = GW.write_raster(path, a, L, bigtiff="auto", classic_limit=1000)
        assert res["bigtiff"] == want == G.raster_info(path)["bigtiff"] and (os.path.getsize(path) > 1000) == want
        assert np.array_equal(G.read_raster(path), a)
    L = GW.raster_layout("u1", 40, 70)
    exact = GW.write_raster(str(tmp_path / "e.tif"), large, L)["size"]           # <= the limit is still classic
    assert not GW.write_raster(str(tmp_path / "e.tif"), large, L, classic_limit=exact)["bigtiff"]
    assert GW.write_raster(str(tmp_path / "e.tif"), large, L, classic_limit=exact - 1)["bigtiff"]
    with pytest.raises(TiffError, match=str(exact)):
        GW.write_raster(str(tmp_path / "n.tif"), large, L, bigtiff="no", classic_limit=1000)
    assert not GW.write_raster(str(tmp_path / "n.tif"), large, L, bigtiff="no")["bigtiff"]


def test_thread_count_does_not_change_the_file(tmp_path):
    a = make_array("f4", 3, 40, 70)
    L = GW.raster_layout("f4", 40, 70, 3, tile=16, predictor=3)
    blobs = []
    for threads in (1, 4):
        GW.write_raster(str(tmp_path / f"t{threads}.tif"), a, L, compress="deflate", level=9, threads=threads)
        blobs.append(open(tmp_path / f"t{threads}.tif", "rb").read())
    assert blobs[0] == blobs[1]
    for bad in (0, 17, 2.5, True):
        with pytest.raises(ValueError, match="threads"):
            GW.write_raster(str(tmp_path / "bad.tif"), a, L, threads=bad)
    for kw in (dict(compress="lzw"), dict(level=0), dict(level=10), dict(bigtiff="maybe")):
        with pytest.raises(ValueError):
            GW.write_raster(str(tmp_path / "bad.tif"), a, L, **kw)
    assert not os.path.exists(tmp_path / "bad.tif")
    with pytest.raises(ValueError, match="extra tag"):
        GW.write_raster(str(tmp_path / "bad.tif"), a, L, extra_tags=[(256, 3, [1])])


def test_a_constant_map_compresses_to_a_fraction(tmp_path):
    a = np.full((256, 256), 255, dtype=np.uint8)
    write_strip_tiff(str(tmp_path / "plain.tif"), a)
    for tile in (None, 64):
        L = GW.raster_layout("u1", 256, 256, tile=tile, predictor=2)
        GW.write_raster(str(tmp_path / "z.tif"), a, L, compress="deflate")
        assert os.path.getsize(tmp_path / "z.tif") * 10 < os.path.getsize(tmp_path / "plain.tif")
        assert np.array_equal(G.read_raster(str(tmp_path / "z.tif")), a)


# ----------------------------------------------------------------------------------------------------------- the options
OUT_KEYWORDS = ("out_compress", "out_level", "out_predictor", "out_tile", "out_bigtiff", "out_threads")


def test_default_options_are_the_plain_value():
    o = InferOptions.make()
    assert o == InferOptions() and type(o) is InferOptions and len(dataclasses.fields(o)) == 15
    assert set(OUT_KEYWORDS) <= set(KEYWORDS)
    assert (o.out_compress, o.out_level, o.out_predictor, o.out_tile, o.out_bigtiff, o.out_threads) == \
        ("none", 6, "auto", None, "auto", 4) and not o.packed_output
    same = InferOptions.make(out_compress="none", out_level=6, out_predictor="auto", out_tile=None, out_bigtiff="auto",
                             out_threads=4)
    assert type(same) is InferOptions and same == o


@pytest.mark.parametrize("other", [dict(), dict(nodata="auto"), dict(decode="device"), dict(write_vectors=True),
                                   dict(nodata=0, decode_threads=2, write_vectors=True)])
def test_an_out_option_derives_from_the_class_the_other_options_chose(other):
    base = InferOptions.make(**other)
    for kw in (dict(out_compress="deflate"), dict(out_tile=32), dict(out_bigtiff="yes"), dict(out_threads=2),
               dict(out_predictor="off"), dict(out_compress="deflate", out_level=9)):
        o = InferOptions.make(**other, **kw)
        assert type(o) is not type(base) and isinstance(o, type(base)) and type(o).__mro__[1] is type(base)
        assert o.packed_output and all(getattr(o, k) == v for k, v in kw.items())
        assert [f.name for f in dataclasses.fields(o)] == [f.name for f in dataclasses.fields(base)] + list(OUT_KEYWORDS)
        assert all(getattr(o, f.name) == getattr(base, f.name) for f in dataclasses.fields(base))
        assert type(o.resolve(64, 64, 4)) is type(o) and o.resolve(64, 64, 4).out_tile == o.out_tile
    o = InferOptions.make(out_compress="deflate", **other)
    assert (o.predictor_for(np.uint8), o.predictor_for(np.float32)) == (2, 3)
    assert InferOptions.make(out_compress="deflate", out_predictor="off").predictor_for(np.float32) == 1
    assert InferOptions.make(out_tile=16).predictor_for(np.uint8) == 1          # no deflate: no predictor


@pytest.mark.parametrize("kw", [dict(out_compress="lzw"), dict(out_level=3), dict(out_compress="deflate", out_level=0),
                                dict(out_compress="deflate", out_level=10), dict(out_compress="deflate", out_level=2.5),
                                dict(out_predictor="2"), dict(out_tile=24), dict(out_tile=0), dict(out_tile=8),
                                dict(out_tile=-16), dict(out_tile=True), dict(out_bigtiff="maybe"), dict(out_threads=0),
                                dict(out_threads=17), dict(out_threads=1.5)], ids=str)
def test_bad_out_options_raise_before_anything_else_runs(kw, tmp_path):
    from floodplanet_code_amd import infer as I
    with pytest.raises(ValueError, match="out_"):
        InferOptions.make(**kw)
    with pytest.raises(ValueError, match="out_"):                                # before the checkpoint or a scene is opened
        I.infer(str(tmp_path / "no" / "checkpoints" / "such.ckpt"), [str(tmp_path / "none.tif")], str(tmp_path / "out"),
                **kw)
    assert not os.path.exists(tmp_path / "out")


def test_command_line_and_keywords_build_the_same_options():
    from floodplanet_code_amd.infer import build_parser
    head = ["x.ckpt", "in", "--out_dir", "o"]
    cases = [([], dict()), (["--out_compress", "deflate", "--out_level", "9", "--out_threads", "8"],
                            dict(out_compress="deflate", out_level=9, out_threads=8)),
             (["--out_tile"], dict(out_tile=256)), (["--out_tile", "512", "--out_bigtiff", "yes"],
                                                    dict(out_tile=512, out_bigtiff="yes")),
             (["--out_compress", "deflate", "--out_predictor", "off", "--nodata", "auto", "--write_vectors"],
              dict(out_compress="deflate", out_predictor="off", nodata="auto", write_vectors=True))]
    for argv, kw in cases:
        got = InferOptions.from_args(build_parser().parse_args(head + argv))
        assert got == InferOptions.make(**kw) and type(got) is type(InferOptions.make(**kw))
    with pytest.raises(ValueError, match="out_tile"):
        InferOptions.from_args(build_parser().parse_args(head + ["--out_tile", "100"]))


# ----------------------------------------------------------------------------------------------------------- write_scene
def _scene_arrays(H, W, k=3, seed=5):
    g = np.random.default_rng(seed)
    return {"counts": np.array([H * W - 7, 4, 3], dtype=np.int64), "n_valid": np.array([H * W - 5], dtype=np.int64),
            "class": g.choice(np.array([0, 127, 255], dtype=np.uint8), size=(H, W)),
            "probs": g.integers(0, 256, (k, H, W), dtype=np.uint8), "margin": g.integers(0, 256, (H, W), dtype=np.uint8),
            "valid": g.integers(0, 2, (H, W), dtype=np.uint8), "canvas": g.random((H, W, k), dtype=np.float32)}


SCENE_TAGS = {33550: (10.0, 10.0, 0.0), 33922: (0.0, 0.0, 0.0, 500000.0, 4000000.0, 0.0)}


def test_write_scene_with_default_options_is_write_strip_tiff_byte_for_byte(tmp_path):
    from floodplanet_code_amd import infer as I
    H, W = 37, 52
    arrays = _scene_arrays(H, W)
    scene = {"hw": (H, W), "src_hw": (H, W), "tags": SCENE_TAGS, "n": 1, "nodata": 0.0, "skipped": 0}
    tags = I.geo_tags_for_grid(SCENE_TAGS, (H, W), (H, W))
    for probs in ("u8", "f32"):
        options = InferOptions.make(write_probs=probs, write_margin=True, nodata="auto", write_valid=True).resolve(64, 64, 2)
        out = str(tmp_path / probs / "img.tif")
        rec = I.write_scene(arrays, scene, options, "in.tif", out)
        assert "output_format" not in rec
        want = {"output": (arrays["class"], tags + [(42113, 2, "127")]), "margin": (arrays["margin"], tags),
                "valid": (arrays["valid"], tags),
                "probabilities": (arrays["probs"] if probs == "u8"
                                  else np.ascontiguousarray(arrays["canvas"].transpose(2, 0, 1)), tags)}
        for key, (array, extra) in want.items():
            write_strip_tiff(str(tmp_path / "want.tif"), array, extra_tags=extra)
            assert open(rec[key], "rb").read() == open(tmp_path / "want.tif", "rb").read(), (probs, key)
    assert "output_format" not in I.run_summary([rec], 1, 1.0, 1, options, "raw")


def test_default_route_switches_to_bigtiff_where_classic_cannot_hold_the_file(tmp_path, monkeypatch):
    """The limit is 2^32 - 1; lowered to 1000 bytes here, the class map (37 x 52) and the canvas no longer fit."""
    from floodplanet_code_amd import infer as I
    monkeypatch.setattr(GW, "CLASSIC_LIMIT", 1000)
    H, W = 37, 52
    arrays = _scene_arrays(H, W)
    scene = {"hw": (H, W), "src_hw": (H, W), "tags": SCENE_TAGS, "n": 1}
    options = InferOptions.make(write_probs="f32").resolve(64, 64, 2)
    rec = I.write_scene(arrays, scene, options, "in.tif", str(tmp_path / "big" / "img.tif"))
    for key, want in (("output", arrays["class"]), ("probabilities", arrays["canvas"].transpose(2, 0, 1))):
        info = G.raster_info(rec[key])
        assert info["bigtiff"] and not info["tiled"] and info["rows_per_strip"] == 16 and info["compression"] == 1
        assert np.array_equal(bits(G.read_raster(rec[key])), bits(want))
        assert G.raster_geotiff_tags(rec[key])[33550] == (10.0, 10.0, 0.0)
    assert rec["output_format"]["bigtiff"] == {"class": True, "probabilities": True}
    assert rec["output_format"]["compress"] == "none" and rec["output_format"]["tile"] is None
    assert I.run_summary([rec], 1, 1.0, 1, options, "raw")["output_format"]["bigtiff"] is True


def test_write_scene_with_out_options_writes_the_packed_bytes(tmp_path):
    """Host only: what finalize_scene reads from the device is stood in for by pack_host, as empty_scene_arrays does."""
    from floodplanet_code_amd import infer as I
    H, W = 37, 52
    raw = _scene_arrays(H, W)
    scene = {"hw": (H, W), "src_hw": (H, W), "tags": SCENE_TAGS, "n": 1, "nodata": 0.0, "skipped": 0}
    kw = dict(write_margin=True, nodata="auto", write_valid=True)
    for probs, out_kw in (("u8", dict(out_compress="deflate", out_tile=16)), ("f32", dict(out_compress="deflate")),
                          ("f32", dict(out_tile=32, out_bigtiff="yes"))):
        options = InferOptions.make(write_probs=probs, **kw, **out_kw).resolve(64, 64, 2)
        arrays = {k: raw[k] for k in ("counts", "n_valid")}
        for name in I.PACKED_RASTERS:
            a = raw[name].transpose(2, 0, 1) if name == "canvas" else raw[name]
            arrays["packed_" + name] = GW.pack_host(a, I.output_layout(options, a.dtype, a.shape))
        out = str(tmp_path / f"{probs}{len(out_kw)}{options.out_tile}" / "img.tif")
        rec = I.write_scene(arrays, scene, options, "in.tif", out)
        plain = I.write_scene(raw, scene, InferOptions.make(write_probs=probs, **kw).resolve(64, 64, 2), "in.tif",
                              str(tmp_path / "plain" / "img.tif"))
        big = options.out_bigtiff == "yes"
        for key in ("output", "probabilities", "margin", "valid"):
            assert np.array_equal(bits(G.read_raster(rec[key])), bits(G.read_raster(plain[key]))), key
            assert G.raster_geotiff_tags(rec[key]) == G.raster_geotiff_tags(plain[key]), key
            info = G.raster_info(rec[key])
            assert info["bigtiff"] == big and info["tiled"] == (options.out_tile is not None)
            assert info["compression"] == (8 if options.out_compress == "deflate" else 1)
            want_p = 1 if options.out_compress == "none" else 3 if info["dtype"] == "float32" else 2
            assert info["predictor"] == want_p, key
        assert G.raster_geotiff_tags(rec["output"])[42113] == "127"
        fmt = rec["output_format"]
        assert fmt == {"compress": options.out_compress, "level": 6 if options.out_compress == "deflate" else None,
                       "predictor": "auto", "tile": options.out_tile, "threads": 4,
                       "bigtiff": {k: big for k in ("class", "valid", "probabilities", "margin")}}
        assert I.run_summary([rec], 1, 1.0, 1, options, "raw")["output_format"] == dict(fmt, bigtiff=big)


def test_empty_scene_arrays_are_packed_on_the_host(tmp_path):
    from floodplanet_code_amd import infer as I
    options = InferOptions.make(nodata="auto", write_valid=True, write_probs="f32", write_margin=True, write_vectors=True,
                                out_compress="deflate", out_tile=16).resolve(64, 64, 2)
    scene = {"hw": (21, 40), "src_hw": (21, 40), "tags": {}, "n": 0, "nodata": 0.0, "skipped": 2}
    arrays = I.empty_scene_arrays(scene, 3, options)
    assert {"packed_class", "packed_margin", "packed_valid", "packed_canvas", "class"} <= set(arrays)
    assert not {"margin", "valid", "canvas"} & set(arrays)                       # only the class map rides along, for the rings
    rec = I.write_scene(arrays, scene, options, "in.tif", str(tmp_path / "e" / "img.tif"))
    assert (G.read_raster(rec["output"]) == 127).all() and G.read_raster(rec["output"]).shape == (21, 40)
    prob = G.read_raster(rec["probabilities"])
    assert prob.shape == (3, 21, 40) and prob.dtype == np.float32 and not prob.any()
    assert not G.read_raster(rec["valid"]).any() and rec["vectors"]["polygons"] == 0
