"""Host-side data path: tile grid against vectors produced by the reference's own function,
TIFF decoding against synthetic files and the bundled rasters' golden checksums, the dataset's item contract."""
import gzip
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from tools.tiff_writer import make_floodplanet_tree, write_tiff   # noqa: E402

from floodplanet_code_amd.datasets import (CropParams, FloodplanetTiles, TiffError, collate_tiles,   # noqa: E402
                                           generate_image_slice_object, get_crop_slices, read_tiff, resize_image,
                                           resize_lanczos4, resize_nearest, tiff_info, tiff_size)

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_crop_slices_match_the_reference_function_on_1120_cases():
    cases = json.load(open(os.path.join(GOLD, "tiles_golden.json")))
    assert len(cases) == 1120
    kinds = set()
    for c in cases:
        a = c["args"]
        step = tuple(a["step"]) if isinstance(a["step"], list) else a["step"]
        args = (a["height"], a["width"], a["crop_height"], a["crop_width"], step, a["mode"])
        if "raises" in c:
            exc = {"ValueError": ValueError, "TypeError": TypeError, "NotImplementedError": NotImplementedError}[c["raises"]]
            with pytest.raises(exc):
                get_crop_slices(*args)
            kinds.add(c["raises"])
            continue
        got = get_crop_slices(*args)
        if "slices" in c:
            assert got == c["slices"], a
        else:
            assert len(got) == c["n"] and got[:5] == c["head"] and got[-5:] == c["tail"], a
            assert hashlib.sha256(json.dumps(got).encode()).hexdigest() == c["sha"], a
    assert kinds == {"ValueError", "TypeError", "NotImplementedError"}


def test_crop_params_and_slice_object():
    cp = CropParams(256, 768, 256, 200, 1024, 968, 256, 256)
    assert (cp.hE, cp.wE, cp.og_height, cp.max_crop_width) == (512, 968, 1024, 256)
    assert "H0: 256" in str(cp)
    s = generate_image_slice_object(256)
    assert (s.height, s.width, s.stride, s.scale) == (256, 256, 256, 1)
    assert generate_image_slice_object(64, 96, 32, 2)[:] == (64, 96, 2, 32)


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16", "float32", "float64", "uint32"])
@pytest.mark.parametrize("byteorder", ["<", ">"])
@pytest.mark.parametrize("planar", [1, 2])
def test_tiff_round_trip(tmp_path, dtype, byteorder, planar):
    g = np.random.default_rng(1)
    for shape, rps in [((37, 23), 5), ((3, 37, 23), 8), ((7, 16, 16), 100), ((2, 1, 9), 1)]:
        a = (g.random(shape) * 200 - 20).astype(dtype)
        p = str(tmp_path / f"a_{len(shape)}_{rps}.tif")
        write_tiff(p, a, planar=planar, rows_per_strip=rps, byteorder=byteorder)
        got = read_tiff(p)
        want = a if (a.ndim == 2 or planar == 2) else np.transpose(a, (1, 2, 0))     # chunky -> [H, W, bands]
        assert got.dtype == np.dtype(dtype) and got.dtype.isnative and got.flags.c_contiguous
        assert got.shape == want.shape and np.array_equal(got, want)
        assert tiff_size(p) == (shape[-2], shape[-1])
        info = tiff_info(p)
        assert info["dtype"] == dtype and info["samples"] == (1 if len(shape) == 2 else shape[0])


def test_tiff_reader_rejects_what_it_does_not_decode(tmp_path):
    a = np.arange(64, dtype=np.uint8).reshape(8, 8)
    p = str(tmp_path / "x.tif")
    write_tiff(p, a, compression=5)
    with pytest.raises(TiffError, match="compress"):
        read_tiff(p)
    write_tiff(p, a, magic=43)
    with pytest.raises(TiffError, match="BigTIFF"):
        read_tiff(p)
    write_tiff(p, a, extra_tags=[(322, 3, [16]), (324, 4, [8])])
    raw = bytearray(open(p, "rb").read())
    open(p, "wb").write(raw[: len(raw) - 10])                       # truncated strip data
    with pytest.raises(TiffError):
        read_tiff(p)
    open(p, "wb").write(b"PK\x03\x04 not a tiff")
    with pytest.raises(TiffError, match="not a TIFF"):
        read_tiff(p)
    open(p, "wb").write(b"II")
    with pytest.raises(TiffError):
        read_tiff(p)


def test_bundled_rasters_decode_to_their_golden_checksums(tmp_path):
    """rasters_golden.json: shape, dtype and checksum of the dataset's 115 rasters.  They come in five TIFF layouts (planar,
    uncompressed: 7-band float32 L8 with 15 or 18 rows per strip, 2-band float32 S1 with 5 or 6, 1-band uint8 labels with
    8); tests/golden/rasters/ holds one raster of each layout, gzipped, under its path in the dataset."""
    gold = json.load(open(os.path.join(GOLD, "rasters_golden.json")))
    assert len(gold) == 115
    bundled = os.path.join(GOLD, "rasters")
    rels = sorted(os.path.relpath(os.path.join(d, f), bundled)[:-3] for d, _, fs in os.walk(bundled) for f in fs)
    layouts = set()
    for rel in rels:
        want = gold[rel]
        path = str(tmp_path / os.path.basename(rel))
        with gzip.open(os.path.join(bundled, rel + ".gz"), "rb") as src, open(path, "wb") as dst:
            dst.write(src.read())
        info = tiff_info(path)
        layouts.add((info["dtype"], info["samples"], info["rows_per_strip"], info["planar"]))
        a = read_tiff(path)
        a3 = a[None] if a.ndim == 2 else a
        assert list(a3.shape) == want["shape"] and a3.dtype.name == want["dtype"], rel
        assert hashlib.sha256(np.ascontiguousarray(a3.astype(a3.dtype.newbyteorder("<"))).tobytes()).hexdigest() == \
            want["sha256"], rel
    assert layouts == {("float32", 7, 15, 2), ("float32", 7, 18, 2), ("float32", 2, 5, 2), ("float32", 2, 6, 2),
                       ("uint8", 1, 8, 1)}, layouts


def test_resampling_conventions():
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert resize_image(a, 3, 4) is a                                   # same size: untouched (utils_image.py:37-38)
    assert np.array_equal(resize_nearest(a, 6, 8), a[np.arange(6) // 2][:, np.arange(8) // 2])
    assert np.array_equal(resize_nearest(np.arange(5)[None], 1, 2), np.array([[0, 2]]))      # floor(dst * 5 / 2)
    c = np.full((2, 9, 11), 3.5, np.float32)
    assert np.abs(resize_lanczos4(c, 31, 17) - 3.5).max() < 1e-5        # weights sum to one, borders replicate
    r = resize_lanczos4(np.random.default_rng(0).random((5, 6)).astype(np.float32), 10, 12)
    assert r.shape == (10, 12) and r.dtype == np.float32
    # an impulse far from the border reproduces the separable 8-tap kernel
    z = np.zeros((33, 33), np.float32)
    z[16, 16] = 1
    up = resize_lanczos4(z, 66, 66)
    assert abs(up.sum() - 4.0) < 2e-2 and up.max() == up[32:34, 32:34].max()
    with pytest.raises(NotImplementedError):
        resize_image(np.zeros((1, 2, 3, 4)), 2, 2)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("fp"))
    return root, make_floodplanet_tree(root)


def test_lanczos_tile_tables_reproduce_the_crop_of_the_whole_raster():
    """Round 4: the device resampling path ships per tile a window of the source raster + two 8-tap tables
    (datasets.resize.lanczos4_axis_window).  Lanczos is local, so the tile computed from them must equal the crop of the whole
    raster's resample -- bit for bit (same taps, same order) -- for interior tiles, tiles cut at the raster's edge (zero rows
    beyond it), single rows, upsampling and downsampling; equal sizes give the identity (the reference's resize is a no-op)."""
    from floodplanet_code_amd.datasets.resize import lanczos4_axis_window, resize_lanczos4, resize_lanczos4_tile
    g = np.random.default_rng(0)
    for (hs, ws, hd, wd) in [(37, 41, 128, 96), (120, 90, 50, 64), (33, 33, 33, 70)]:
        a = g.standard_normal((2, hs, ws)).astype(np.float32)
        full = resize_lanczos4(a, hd, wd) if (hs, ws) != (hd, wd) else a
        for (h0, hE, w0, wE, TH, TW) in [(0, 32, 0, 32, 32, 32), (hd - 20, hd, wd - 9, wd, 32, 32), (5, 6, 7, 9, 8, 8),
                                         (0, min(hd, 48), 0, min(wd, 48), 48, 48)]:
            iy, wy, (y0, y1) = lanczos4_axis_window(hs, hd, h0, hE, TH)
            ix, wx, (x0, x1) = lanczos4_axis_window(ws, wd, w0, wE, TW)
            assert iy.dtype == np.int32 and wy.dtype == np.float32 and iy.min() >= 0 and iy.max() < y1 - y0
            t = resize_lanczos4_tile(a[:, y0:y1, x0:x1], iy, wy, ix, wx)
            np.testing.assert_array_equal(t[:, :hE - h0, :wE - w0], full[:, h0:hE, w0:wE])
            assert not t[:, hE - h0:].any() and not t[:, :, wE - w0:].any()
    with pytest.raises(ValueError):
        lanczos4_axis_window(10, 20, 5, 30, 32)


def test_window_items_equal_raw_items(tree):
    """FloodplanetTiles.window_item (device resampling) carries what raw_item (host resampling) computes: resampling the window
    with its tables and applying the sensor scaling on the host gives raw_item's crop bit for bit, same padded target."""
    from floodplanet_code_amd.datasets.resize import resize_lanczos4_tile
    root, _ = tree
    ds = FloodplanetTiles(root, "all", generate_image_slice_object(40, 40, 40), eval_region=["RegA"], sensor="S1", ignore_index=0)
    assert len(ds) > 4
    for i in range(len(ds)):
        w, r = ds.window_item(i), ds.raw_item(i)
        t = resize_lanczos4_tile(w["window"].numpy(), w["iy"].numpy(), w["wy"].numpy(), w["ix"].numpy(), w["wx"].numpy())
        t = np.nan_to_num(np.clip((t + 50) / 100, 0, 1)).astype(np.float32)
        h, wd = r["raw"].shape[-2:]
        assert w["valid_hw"] == (h, wd) and w["scale_mode"] == 1
        np.testing.assert_array_equal(t[:, :h, :wd], r["raw"].numpy())
        assert torch.equal(w["target"], r["target"])


def test_dataset_items_follow_the_reference_contract(tree):
    root, made = tree
    sp = generate_image_slice_object(64, 64, 64)
    ds = FloodplanetTiles(root, "train", sp, eval_region=["RegC"], sensor="S1", ignore_index=0, output_metadata=True)
    assert ds.n_channels == {"ms_image": 2} and ds.n_classes == 3
    assert len(ds.skipped_without_label) == 2                            # the orphans of RegA / RegB
    # 96x96 labels, 64x64 tiles, mode "exact": 1 full + 2 edge strips + 1 corner per image, 2 regions x 2 images
    assert len(ds) == 4 * 4
    seen_edge = False
    for i in range(len(ds)):
        it = ds[i]
        cp, reg, name = it["metadata"]["crop_params"], it["metadata"]["region_name"], None
        assert reg in ("RegA", "RegB")
        assert it["image"].shape == (2, 64, 64) and it["image"].dtype == torch.float32
        assert it["target"].shape == (64, 64) and it["target"].dtype == torch.int64
        assert it["mean"].shape == (2, 1, 1) and (it["mean"] == 0).all() and (it["std"] == 1).all()
        assert 0.0 <= it["image"].min() and it["image"].max() <= 1.0 and torch.isfinite(it["image"]).all()
        name = os.path.splitext(os.path.basename(it["metadata"]["image_path"]))[0]
        lab = made[(reg, name)]["label"][cp.h0:cp.hE, cp.w0:cp.wE]
        want = np.where(lab == 2, 1, 0)                                   # 0 (no data) -> ignore_index 0, 1 -> 0, 2 -> 1
        t = it["target"].numpy()
        assert np.array_equal(t[:lab.shape[0], :lab.shape[1]], want)
        if lab.shape != (64, 64):
            seen_edge = True
            assert (t[lab.shape[0]:, :] == 0).all() and (t[:, lab.shape[1]:] == 0).all()       # ignore padding
            assert (it["image"][:, lab.shape[0]:, :] == 0).all() and (it["image"][:, :, lab.shape[1]:] == 0).all()
    assert seen_edge
    # S1 scaling on an un-resampled read: clip((x + 50) / 100, 0, 1), NaN -> 0 (floodplanet.py:347-348)
    ds_same = FloodplanetTiles(root, "all", generate_image_slice_object(96, 96, 96), eval_region=["RegA"], sensor="S1",
                               ignore_index=0, output_metadata=True)
    it = ds_same[0]
    assert it["image"].shape == (2, 96, 96)
    b = collate_tiles([ds[0], ds[1]])
    assert b["image"].shape == (2, 2, 64, 64) and b["target"].shape == (2, 64, 64) and b["mean"].shape == (2, 2, 1, 1)
    assert len(b["metadata"]) == 2


def test_dataset_scaling_is_exact_when_no_resampling_is_needed(tmp_path):
    root = str(tmp_path)
    made = make_floodplanet_tree(root, regions=("Solo",), images_per_region=1, label_size=40, s1_size=40, l8_size=40)
    (reg, name), arrs = next(iter(made.items()))
    sp = generate_image_slice_object(40, 40, 40)
    s1 = FloodplanetTiles(root, "all", sp, eval_region=["Solo"], sensor="S1", ignore_index=2)[0]
    want = np.nan_to_num(np.clip((arrs["S1"] + 50) / 100, 0, 1))
    assert np.array_equal(s1["image"].numpy(), want.astype(np.float32))
    assert np.array_equal(s1["target"].numpy(), np.where(arrs["label"] == 2, 1, np.where(arrs["label"] == 0, 2, 0)))
    l8 = FloodplanetTiles(root, "all", sp, eval_region=["Solo"], sensor="L8", ignore_index=0, norm_mode="local")[0]
    x = (np.clip(arrs["L8"], 0, 18607.72) / 18607.72).astype(np.float32)
    flat = x.reshape(7, -1)
    assert np.allclose(l8["image"].numpy(), (x - flat.mean(1)[:, None, None]) / flat.std(1)[:, None, None], atol=1e-6)
    assert np.allclose(l8["mean"][:, 0, 0], flat.mean(1)) and np.allclose(l8["std"][:, 0, 0], flat.std(1))


def test_dataset_splits_and_errors(tree):
    root, _ = tree
    sp = generate_image_slice_object(64, 64, 64)
    tr = FloodplanetTiles(root, "train", sp, eval_region="RegC", sensor="L8", ignore_index=0)
    va = FloodplanetTiles(root, "valid", sp, eval_region="RegC", sensor="L8", ignore_index=0)
    assert {e["region_name"] for e in tr.dataset} == {"RegA", "RegB"} and {e["region_name"] for e in va.dataset} == {"RegC"}
    assert tr.n_channels == {"ms_image": 7}
    a = FloodplanetTiles(root, "train", sp, sensor="L8", ignore_index=0, seed_num=0, train_split_pct=0.5)
    b = FloodplanetTiles(root, "train", sp, sensor="L8", ignore_index=0, seed_num=0, train_split_pct=0.5)
    v = FloodplanetTiles(root, "valid", sp, sensor="L8", ignore_index=0, seed_num=0, train_split_pct=0.5)
    assert [e["image_path"] for e in a.dataset] == [e["image_path"] for e in b.dataset]          # seeded split
    assert not ({e["image_path"] for e in a.dataset} & {e["image_path"] for e in v.dataset})
    assert len({e["image_path"] for e in a.dataset} | {e["image_path"] for e in v.dataset}) == 6
    with pytest.raises(ValueError, match="Eval region"):
        FloodplanetTiles(root, "train", sp, eval_region=["Nowhere"], sensor="L8")
    with pytest.raises(ValueError, match="No images found"):
        FloodplanetTiles(root, "all", sp, eval_region=["RegA"], sensor="PS")
    with pytest.raises(NotImplementedError, match="DEM"):
        FloodplanetTiles(root, "all", sp, eval_region=["RegA"], sensor="S1", dem=True)
    with pytest.raises(ValueError, match="Train split pct"):
        FloodplanetTiles(root, "train", sp, sensor="S1", train_split_pct=1.5)
    with pytest.raises(NotImplementedError):
        FloodplanetTiles(root, "train", sp, sensor="S1", channels="RGB")


# ---------------------------------------------------------------------------------------------------------------------
# the item dicts against the reference's own crop grid / normalize / buffer functions (oracle/make_loader_golden.py)
def loader_golden():
    z = np.load(os.path.join(GOLD, "loader_golden.npz"))
    return json.loads(bytes(z["meta"]).decode()), z


def loader_tree(tmp_path, meta):
    root = str(tmp_path / "loader_tree")
    t = dict(meta["tree"])
    t["regions"] = tuple(t["regions"])
    make_floodplanet_tree(root, **t)
    return root


def item_key(md):
    cp = md["crop_params"]
    name = os.path.splitext(os.path.basename(md["image_path"]))[0]
    return f"{md['region_name']}/{name}/{cp.h0}_{cp.w0}"


@pytest.mark.parametrize("norm_mode", [None, "local"])
def test_host_assembled_items_equal_the_reference_functions_fixture(tmp_path, norm_mode):
    """Every crop of a synthetic tree (image raster at the label raster's size: no resampling takes part): TIFF reader ->
    crop grid -> S1 scaling -> normalize -> edge buffer, against arrays produced by the reference's own get_crop_slices /
    _crop_image / normalize / _add_buffer_to_image.  Same float32 operations -> bit-exact, 'local' statistics included."""
    from floodplanet_code_amd.datasets import FloodplanetTiles, generate_image_slice_object
    meta, z = loader_golden()
    root = loader_tree(tmp_path, meta)
    sp = generate_image_slice_object(meta["crop"]["height"], meta["crop"]["width"], meta["crop"]["stride"])
    ds = FloodplanetTiles(root, "all", sp, eval_region=["RegA"], sensor="S1", ignore_index=meta["ignore_index"],
                          norm_mode=norm_mode, output_metadata=True)
    assert len(ds) == len(meta["items"])
    seen = set()
    for i in range(len(ds)):
        it = ds[i]
        k = item_key(it["metadata"])
        seen.add(k)
        np.testing.assert_array_equal(it["image"].numpy(), z[f"{k}/{norm_mode}/image"], err_msg=k)
        np.testing.assert_array_equal(it["target"].numpy(), z[f"{k}/target"], err_msg=k)
        np.testing.assert_array_equal(np.asarray(it["mean"]).reshape(-1), z[f"{k}/{norm_mode}/mean"], err_msg=k)
        np.testing.assert_array_equal(np.asarray(it["std"]).reshape(-1), z[f"{k}/{norm_mode}/std"], err_msg=k)
    assert seen == {f"{i['region']}/{i['name']}/{i['h0']}_{i['w0']}" for i in meta["items"]}
