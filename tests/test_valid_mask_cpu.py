"""CPU: nodata in scene inference -- the three host statements of datasets/valid_mask.py on hand-made cases, the nodata
options of InferOptions and their flags, a SceneQueue that meets a scene without a box, and write_scene's GDAL_NODATA tag."""
import dataclasses
import hashlib
import os

import numpy as np
import pytest

from floodplanet_code_amd import infer as I
from floodplanet_code_amd.datasets.resize import lanczos4_axis_window
from floodplanet_code_amd.datasets.tiff import read_geotiff_tags, read_tiff
from floodplanet_code_amd.datasets.valid_mask import (axis_tables, box_valid_counts_host, grid_valid_host,
                                                      source_valid_host)
from floodplanet_code_amd.infer_options import KEYWORDS, InferOptions, NodataInferOptions, scene_nodata


def fill_cases(C, h, w, nodata, seed=0):
    """A raster [C, h, w] with every kind of fill the rule names, and the mask the rule gives it, built by hand: a fill
    corner, a single fill pixel, NaN / Inf in one band, a pixel where only some bands equal nodata (valid when C > 1)."""
    g = np.random.default_rng(seed)
    a = (g.random((C, h, w), dtype=np.float32) * 70 - 50).astype(np.float32)
    a[a == 0] = 1.0
    fill = np.float32(0 if nodata is None else nodata)
    want = np.ones((h, w), dtype=np.uint8)
    a[:, :h // 3, : w // 4] = fill                      # a fill corner
    a[:, h // 2, w // 2] = fill                         # a single fill pixel
    if nodata is not None:
        want[:h // 3, : w // 4] = 0
        want[h // 2, w // 2] = 0
    a[C - 1, h - 2, 1] = np.nan                         # not finite in one band
    a[0, h - 1, w - 1] = np.inf
    a[C // 2, 0, w - 1] = -np.inf
    want[h - 2, 1] = want[h - 1, w - 1] = want[0, w - 1] = 0
    a[0, h - 3, w - 3] = fill                           # only some bands equal nodata: valid -- unless it is the only band
    if C == 1 and nodata is not None:
        want[h - 3, w - 3] = 0
    return a, want


@pytest.mark.parametrize("nodata", [0, -9999, None])
@pytest.mark.parametrize("C", [1, 2, 7])
def test_source_valid_on_hand_made_cases(C, nodata):
    a, want = fill_cases(C, 12, 17, nodata)
    got = source_valid_host(a, nodata)
    assert got.dtype == np.uint8 and got.shape == (12, 17)
    np.testing.assert_array_equal(got, want)
    if nodata is not None:                                   # another value is not fill, the non-finite pixels still are
        assert source_valid_host(a, 5).sum() == 12 * 17 - 3
    with pytest.raises(ValueError, match="finite"):
        source_valid_host(a, float("nan"))


def test_source_valid_compares_in_fp32():
    a = np.full((1, 1, 2), np.float32(0.1), dtype=np.float32)
    np.testing.assert_array_equal(source_valid_host(a, 0.1), [[0, 0]])        # 0.1 rounds to the same fp32
    np.testing.assert_array_equal(source_valid_host(a, 0.1000001), [[1, 1]])


def _tables(src, dst):
    iy, wy, _ = lanczos4_axis_window(src[0], dst[0], 0, dst[0], dst[0])
    ix, wx, _ = lanczos4_axis_window(src[1], dst[1], 0, dst[1], dst[1])
    return iy, wy, ix, wx


def test_grid_valid_identity_tables_give_the_source_mask_back():
    a, want = fill_cases(2, 37, 52, 0)
    src = source_valid_host(a, 0)
    np.testing.assert_array_equal(grid_valid_host(src, *_tables((37, 52), (37, 52))), want)
    for t, u in zip(axis_tables((37, 52), (37, 52)), _tables((37, 52), (37, 52))):
        np.testing.assert_array_equal(t, u)


@pytest.mark.parametrize("dst", [(74, 104), (22, 31)], ids=["2x up", "0.6x down"])
def test_grid_valid_pixel_never_has_fill_among_its_taps(dst):
    a, _ = fill_cases(2, 37, 52, 0)
    src = source_valid_host(a, 0)
    iy, wy, ix, wx = _tables((37, 52), dst)
    got = grid_valid_host(src, iy, wy, ix, wx)
    assert got.shape == dst and got.dtype == np.uint8 and 0 < got.sum() < got.size
    for Y in range(dst[0]):                                  # the rule recomputed from the tables, pixel by pixel
        ys = iy[Y][wy[Y] != 0]
        for X in range(dst[1]):
            xs = ix[X][wx[X] != 0]
            assert got[Y, X] == int(src[np.ix_(ys, xs)].all()), (Y, X)
    full = np.ones((37, 52), dtype=np.uint8)                 # a scene with no fill is all valid
    assert grid_valid_host(full, iy, wy, ix, wx).all()
    assert not grid_valid_host(np.zeros_like(full), iy, wy, ix, wx).any()


def test_box_valid_counts_host():
    g = np.random.default_rng(3)
    m = (g.random((100, 150)) < 0.6).astype(np.uint8)
    boxes = I.crop_boxes(100, 150, 64, 64, 32) + [(5, 7, 6, 8), (0, 0, 100, 150), (3, 33, 50, 80)]
    got = box_valid_counts_host(m, boxes)
    assert got.dtype == np.int64 and got.shape == (len(boxes),)
    assert got.tolist() == [int(m[a:c, b:d].sum()) for a, b, c, d in boxes]
    assert got[-2] == m.sum() and got[-3] == m[5, 7]
    for bad in ([], [(0, 0, 101, 10)], [(4, 4, 4, 9)], [(-1, 0, 3, 3)]):
        with pytest.raises(ValueError):
            box_valid_counts_host(m, bad)


# ------------------------------------------------------------------------------------------------------------ options
def test_nodata_options_and_their_errors():
    d = InferOptions.make()
    assert d == InferOptions() and type(d) is InferOptions and len(dataclasses.fields(d)) == 15   # today's value
    assert (d.nodata, d.nodata_out, d.skip_empty, d.write_valid) == (None, 127, True, False)
    assert InferOptions((8, 8), None, 32, 4, None, "raw", "hann", "u8", True, None, None, False, 0, "cuda:0").stride == 32
    assert set(KEYWORDS) >= {"nodata", "nodata_out", "skip_empty", "write_valid"}
    o = InferOptions.make(nodata="auto")
    assert isinstance(o, InferOptions) and (o.nodata, o.nodata_out, o.skip_empty, o.write_valid) == ("auto", 127, True, False)
    assert [f.name for f in dataclasses.fields(o)][15:] == ["nodata", "nodata_out", "skip_empty", "write_valid"]
    o = InferOptions.make(nodata="-9999", nodata_out=1, skip_empty=False, write_valid=True, stride=16)
    assert o == NodataInferOptions(stride=16, nodata=-9999.0, nodata_out=1, skip_empty=False, write_valid=True)
    assert o.resolve(64, 64, 4).nodata == -9999.0 and o.resolve(64, 64, 4).batch_size == 4
    assert InferOptions.make(nodata=0).nodata == 0.0 and InferOptions.make(nodata=0) != d
    for kw in (dict(nodata_out=3), dict(skip_empty=False), dict(write_valid=True)):
        with pytest.raises(ValueError, match="need --nodata"):
            InferOptions.make(**kw)
    for bad in ("fill", float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="nodata must be 'auto' or a finite number"):
            InferOptions.make(nodata=bad)
    for bad in (0, 255, 300, -1, 1.5):
        with pytest.raises(ValueError, match=r"nodata_out must be an integer in 1\.\.254"):
            InferOptions.make(nodata=0, nodata_out=bad)


def test_flags_map_to_the_same_value():
    base = ["m.ckpt", "in", "--out_dir", "out"]
    args = I.build_parser().parse_args(base)
    assert InferOptions.from_args(args) == InferOptions.make()
    args = I.build_parser().parse_args(base + ["--nodata", "auto"])
    assert InferOptions.from_args(args) == InferOptions.make(nodata="auto")
    args = I.build_parser().parse_args(base + ["--nodata", "-9999", "--nodata_out", "200", "--keep_empty_crops",
                                               "--write_valid", "--sieve", "4"])
    assert InferOptions.from_args(args) == InferOptions.make(nodata=-9999, nodata_out=200, skip_empty=False,
                                                             write_valid=True, sieve=4)
    with pytest.raises(ValueError, match="need --nodata"):
        InferOptions.from_args(I.build_parser().parse_args(base + ["--write_valid"]))


def test_scene_nodata_reads_the_tag_under_auto():
    assert scene_nodata(-5.0, {42113: "7"}) == -5.0
    assert scene_nodata("auto", {42113: "-9999"}) == -9999.0 and scene_nodata("auto", {42113: " 3.5\x00"}) == 3.5
    for tags in ({}, {42113: "nan"}, {42113: "none"}, {42113: "inf"}, {42113: ""}):
        assert scene_nodata("auto", tags) == 0.0


# -------------------------------------------------------------------------------------------------------------- queue
@pytest.mark.parametrize("empty", [{2}, {0}, {5}, {1, 2, 3}, set(range(6))], ids=str)
def test_scene_queue_hands_out_a_scene_without_boxes_once_and_in_order(empty):
    n_boxes = [3, 5, 2, 4, 1, 6]
    uploads = []

    def upload(i):
        uploads.append(i)
        return i, f"scene{i}", [] if i in empty else [(i, j) for j in range(n_boxes[i])]

    q = I.SceneQueue(range(6), upload, 4)
    handed, seen = [], []
    for batch in q.batches():
        assert 1 <= len(batch) <= 4 and not any(i in empty for i, _ in batch)
        seen += batch
        handed += q.stitched(batch)
    handed += q.stitched(())
    assert [i for i, _ in handed] == list(range(6)) and [s for _, s in handed] == [f"scene{i}" for i in range(6)]
    assert seen == [(i, (i, j)) for i in range(6) if i not in empty for j in range(n_boxes[i])]
    assert uploads == list(range(6)) and not q.resident and q.stitched(()) == []
    assert q.max_resident <= 3                               # what it is without an empty scene: they hold no device memory
    plain = I.SceneQueue(range(6), lambda i: (i, i, [(i, j) for j in range(n_boxes[i])]), 4)
    for batch in plain.batches():
        plain.stitched(batch)
    assert plain.max_resident == 3 and plain.stitched(()) == []


# -------------------------------------------------------------------------------------------------------------- files
GEO = {33550: (10.0, 10.0, 0.0), 33922: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0), 34735: (1, 1, 0, 1, 1025, 0, 1, 1),
       42113: "-9999"}


def _arrays(H, W):
    """Fixed arrays from integer arithmetic alone, so the digests below depend on no random generator."""
    y, x = np.mgrid[:H, :W]
    cls = (((3 * y + 5 * x) % 7 < 3) * 255).astype(np.uint8)
    return {"class": cls, "counts": np.array([7, 8, 9], dtype=np.int64), "margin": ((y * x + 11 * y) % 256).astype(np.uint8),
            "probs": np.stack([((k + 1) * y + 13 * x) % 256 for k in range(3)]).astype(np.uint8),
            "valid": ((y + 2 * x) % 5 != 0).astype(np.uint8), "n_valid": np.array([24], dtype=np.int64)}


def test_write_scene_tags_the_class_map_only_under_nodata(tmp_path):
    scene = {"tags": GEO, "src_hw": (20, 30), "hw": (40, 60), "n": 3, "nodata": -9999.0, "skipped": 2}
    kw = dict(write_probs="u8", write_margin=True)
    out = str(tmp_path / "a" / "x.tif")
    rec = I.write_scene(_arrays(40, 60), scene, InferOptions.make(**kw), "in.tif", out)
    assert 42113 not in read_geotiff_tags(out) and "valid_pixels" not in rec and "nodata" not in rec
    assert not os.path.exists(I.side_output_path(out, "valid"))
    out2 = str(tmp_path / "b" / "x.tif")
    rec2 = I.write_scene(_arrays(40, 60), scene, InferOptions.make(nodata="auto", nodata_out=99, write_valid=True, **kw),
                         "in.tif", out2)
    tags = read_geotiff_tags(out2)
    assert tags[42113].rstrip("\x00") == "99" and tags[33550] == read_geotiff_tags(out)[33550]
    for kind in ("prob", "margin", "valid"):                 # 0 is a value there: no nodata tag
        assert 42113 not in read_geotiff_tags(I.side_output_path(out2, kind))
    np.testing.assert_array_equal(read_tiff(rec2["valid"]), _arrays(40, 60)["valid"])
    np.testing.assert_array_equal(read_tiff(out2), read_tiff(out))
    assert (rec2["valid_pixels"], rec2["skipped_crops"], rec2["nodata"], rec2["crops"]) == (24, 2, -9999.0, 3)
    assert set(rec2) - set(rec) == {"valid_pixels", "skipped_crops", "nodata", "valid"}
    assert all(rec2[k] == rec[k] for k in ("input", "source_size", "grid_size", "crops", "class_pixels"))


def test_write_scene_without_the_options_writes_the_files_it_always_wrote(tmp_path):
    """The three files of a fixed array, byte for byte: digests taken with the code as it was before the nodata options."""
    scene = {"tags": GEO, "src_hw": (20, 30), "hw": (40, 60), "n": 3}
    out = str(tmp_path / "x.tif")
    I.write_scene(_arrays(40, 60), scene, InferOptions.make(write_probs="u8", write_margin=True), "in.tif", out)
    digests = {kind: hashlib.sha256(open(p, "rb").read()).hexdigest()
               for kind, p in (("class", out), ("prob", I.side_output_path(out, "prob")),
                               ("margin", I.side_output_path(out, "margin")))}
    assert digests == PARENT_DIGESTS


def test_empty_scene_arrays():
    scene = {"hw": (5, 7), "n": 0}
    o = InferOptions.make(nodata=0, nodata_out=9, write_probs="u8", write_margin=True, write_valid=True, sieve=4,
                          keep_probabilities=True)
    a = I.finalize_scene(None, "0", [0, 255, 255], o, scene)           # no stitcher, no canvas
    assert (a["class"] == 9).all() and a["class"].shape == (5, 7) and a["class"].dtype == np.uint8
    assert a["counts"].tolist() == [0, 0, 0] and a["n_valid"].tolist() == [0] and a["sieve"].tolist() == [0, 0]
    assert a["probs"].shape == (3, 5, 7) and not a["probs"].any() and not a["margin"].any() and not a["valid"].any()
    assert a["kept"].shape == (5, 7, 3) and a["kept"].dtype == np.float32 and not a["kept"].any()


PARENT_DIGESTS = {"class": "aadfa90f58d12c695d2ea290c025bb71280962215b654785810180cfe9cec9c8",
                  "prob": "7271484ef2e7611125e8b5ff142645a8e7fdfbd97b8417ca7e8950ecba33bf58",
                  "margin": "ab871a3f798c6d690f24d511b43a9acffdbb7b9671b3f69561ae6989631e763d"}
