"""CPU: the host statement of the band statistics against the fixture produced by the reference's own
compute_dataset_normalization_parameters (tests/tools/make_normstats_golden.py), the parameter file, and norm_mode
'global' carried from the parameters to the data set items and to infer's up-front checks."""
import glob
import gzip
import os
import pickle
import shutil

import numpy as np
import pytest

from conftest import GOLDEN
from floodplanet_code_amd.datasets import FloodplanetTiles, generate_image_slice_object
from floodplanet_code_amd.datasets import stats as S


def fixture():
    z = np.load(os.path.join(GOLDEN, "loader_normstats_golden.npz"))
    q = np.float32(int(z["q"]))
    srcs = [z[k].astype(np.float32) / q for k in ("image_q", "dem_q", "slope_q")]
    return z, srcs, (z["valid_h"], z["valid_w"])


def test_host_statistics_equal_numpy_fp64_and_the_reference():
    z, srcs, valid = fixture()
    assert srcs[0].shape == (12, 3, 64, 64) and (valid[0] < 64).any() and (valid[1] < 64).any()
    got = S.band_stats_host(srcs, valid, mask="nonzero")
    assert (got["count"] == int(z["f64_count"])).all() and (got["n_nonfinite"] == 0).all()
    n_crop = int((valid[0].astype(np.int64) * valid[1]).sum())
    assert 0 < n_crop - int(z["f64_count"]) <= 40                           # the no-data pixels inside the crops
    np.testing.assert_allclose(got["mean"], z["f64_mean"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["std"], z["f64_std"], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(got["min"], z["f64_min"])
    np.testing.assert_array_equal(got["max"], z["f64_max"])
    assert (z["f64_std"] >= 0.1 * z["f64_mean"]).all()                      # the accuracy bounds' premise
    np.testing.assert_allclose(got["mean"], z["ref_mean"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(got["std"], z["ref_std"], rtol=1e-6, atol=0)
    assert got["hist"].shape == (5, 4096) and (got["hist"].sum(axis=1) == got["count"]).all()


def test_the_first_sources_mask_applies_to_every_source():
    z, srcs, valid = fixture()
    image, dem, slope = srcs
    assert (dem[0, 0, :, 63] != 0).all() and valid[1][5] == 40 and (dem[5, 0, :, 40:] != 0).all()
    three = S.band_stats_host([image, dem, slope], valid, mask="nonzero", return_pixels=True)
    alone = S.band_stats_host([dem], valid, mask="nonzero")                # dem's own mask: every pixel of the crops
    assert three["count"][3] == int(z["f64_count"]) < alone["count"][0]
    m = image.sum(axis=1) != 0
    np.testing.assert_array_equal(three["pixels"][3], dem[:, 0][m])
    # without valid sizes the image's zero padding does the same job, as in the reference's padded items
    np.testing.assert_array_equal(S.band_stats_host([image, dem, slope], None)["count"], three["count"])
    every = S.band_stats_host([image, dem, slope], valid, mask=None)
    assert (every["count"] == int((valid[0].astype(np.int64) * valid[1]).sum())).all()


def test_non_finite_pixels_are_left_out_and_counted():
    _, srcs, valid = fixture()
    image, dem = srcs[0].copy(), srcs[1].copy()
    clean = S.band_stats_host([image, dem], valid)
    image[0, 1, 3, 4] = np.nan
    dem[2, 0, 5, 6] = np.inf
    image[5, 0, 0, 50] = np.nan                                            # outside the valid crop: not even counted
    got = S.band_stats_host([image, dem], valid)
    assert (got["n_nonfinite"] == 2).all() and (got["count"] == clean["count"] - 2).all()
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["std"]).all()


def test_percentiles_from_the_histogram_are_within_one_bin():
    _, srcs, valid = fixture()
    got = S.band_stats_host(srcs, valid, return_pixels=True)
    for q in (5, 50, 95):
        est = S.percentile_from_hist(got["hist"], q, 0.0, 1.0)
        want = np.percentile(got["pixels"].astype(np.float64), q, axis=1)
        assert np.abs(est - want).max() <= 1.0 / 4096, q


def test_parameter_file_round_trip_and_merge(tmp_path):
    path = str(tmp_path / "sub" / "dataset_norm_params.p")
    a = {"S1": {"mean": np.array([0.4, 0.5]), "std": np.array([0.1, 0.2])}}
    S.save_norm_params(path, "floodplanet", a)
    back = S.load_norm_params(path, "floodplanet")
    assert back["S1"]["mean"].dtype == np.float64 and np.array_equal(back["S1"]["std"], a["S1"]["std"])
    S.save_norm_params(path, "other_set", {"PS": {"mean": [0.1] * 4, "std": [0.3] * 4}})
    S.save_norm_params(path, "floodplanet", {"S1": {"mean": np.array([0.6, 0.7]), "std": np.array([0.3, 0.4])}})
    raw = pickle.load(open(path, "rb"))                                     # the reference's layout, plain pickle
    assert set(raw) == {"floodplanet", "other_set"} and list(raw["other_set"]["PS"]["mean"]) == [0.1] * 4
    assert np.array_equal(raw["floodplanet"]["S1"]["mean"], [0.6, 0.7])
    ref_path = str(tmp_path / "ref.p")                                      # a file as the reference writes it
    pickle.dump({"floodplanet": {"S1": {"mean": np.asarray([0.5, 0.25]), "std": np.asarray([0.2, 0.1])},
                                 "dem": {"mean": np.float32([1.0]), "std": np.float32([2.0])}}}, open(ref_path, "wb"))
    got = S.load_norm_params(ref_path, "floodplanet")
    assert set(got) == {"S1", "dem"} and np.array_equal(got["S1"]["mean"], [0.5, 0.25])
    assert S.load_norm_params(raw, "other_set") is raw["other_set"]
    with pytest.raises(KeyError):
        S.load_norm_params(ref_path, "sen1floods11")


def _bundled_tree(tmp_path):
    for gz in glob.glob(os.path.join(GOLDEN, "rasters", "**", "*.tif.gz"), recursive=True):
        dst = tmp_path / os.path.relpath(gz, os.path.join(GOLDEN, "rasters"))[:-3]
        dst.parent.mkdir(parents=True, exist_ok=True)
        with gzip.open(gz) as src, open(dst, "wb") as fh:
            shutil.copyfileobj(src, fh)
    return str(tmp_path)


def test_global_items_are_the_reference_arithmetic_bit_for_bit(tmp_path):
    root = _bundled_tree(tmp_path)
    sp = generate_image_slice_object(300, 300, 300)
    kw = dict(eval_region=["Bangladesh"], sensor="L8", ignore_index=0)
    plain = FloodplanetTiles(root, "all", sp, norm_mode=None, **kw)
    mean = np.linspace(0.05, 0.4, 7)
    std = np.linspace(0.03, 0.2, 7)
    params = {"floodplanet": {"L8": {"mean": mean, "std": std}, "dem": {"mean": np.ones(1), "std": np.ones(1)}}}
    path = str(tmp_path / "p.p")
    pickle.dump(params, open(path, "wb"))
    assert len(plain) >= 4
    for given in (params, path):
        ds = FloodplanetTiles(root, "all", sp, norm_mode="global", norm_params=given, **kw)
        edge = False
        for i in range(len(plain)):
            cp = plain.dataset[i]["crop_params"]
            h, w = cp.hE - cp.h0, cp.wE - cp.w0
            edge |= h < 300 or w < 300
            want = plain[i]["image"].numpy().copy()
            crop = want[:, :h, :w].copy()
            crop -= mean[:, None, None]                                   # base_dataset.py:109-110 on the fp32 image
            crop /= std[:, None, None]
            want[:] = 0
            want[:, :h, :w] = crop
            it = ds[i]
            assert it["image"].dtype == plain[i]["image"].dtype
            np.testing.assert_array_equal(it["image"].numpy().view(np.int32), want.view(np.int32))
            np.testing.assert_array_equal(it["image"].numpy()[:, :h, :w],
                                          ((plain[i]["image"].numpy()[:, :h, :w].astype(np.float64) - mean[:, None, None])
                                           .astype(np.float32).astype(np.float64) / std[:, None, None]).astype(np.float32))
            assert it["mean"].shape == (7, 1, 1) and np.array_equal(it["mean"][:, 0, 0], mean)
            assert np.array_equal(it["std"][:, 0, 0], std) and it["mean"].dtype == np.float64
            np.testing.assert_array_equal(it["target"].numpy(), plain[i]["target"].numpy())
        assert edge
    # the cached raster is not normalised in place: a second read gives the same item
    np.testing.assert_array_equal(ds[0]["image"].numpy(), ds[0]["image"].numpy())
    with pytest.raises(ValueError, match="7"):
        FloodplanetTiles(root, "all", sp, norm_mode="global",
                         norm_params={"floodplanet": {"L8": {"mean": np.zeros(4), "std": np.ones(4)}}}, **kw)
    with pytest.raises(KeyError):
        FloodplanetTiles(root, "all", sp, norm_mode="global", norm_params={"floodplanet": {"S1": params["floodplanet"]["L8"]}},
                         **kw)
    with pytest.raises(NotImplementedError, match="parameter file"):
        FloodplanetTiles(root, "all", sp, norm_mode="global", **kw)
    with pytest.raises(NotImplementedError, match="not implemented"):
        FloodplanetTiles(root, "all", sp, norm_mode="zscore", norm_params=params, **kw)


def test_infer_accepts_global_with_parameters_up_front(tmp_path):
    from floodplanet_code_amd import infer as I
    cfg = dict(crop_height=64, crop_width=64, batch_size=4, norm_mode="global",
               dataset=dict(name="floodplanet", channels="ALL", sensor="S1", dataset_kwargs=None),
               model=dict(name="ms_model", model_kwargs=dict(base_channels=8)))
    params = {"floodplanet": {"S1": {"mean": np.array([0.4, 0.5]), "std": np.array([0.1, 0.2])}}}
    (tmp_path / "scene.tif").write_bytes(b"")
    with pytest.raises(NotImplementedError, match="norm_mode"):
        I.infer(str(tmp_path / "missing.ckpt"), [str(tmp_path)], str(tmp_path / "out"), cfg=cfg)
    with pytest.raises(FileNotFoundError, match="missing.ckpt"):          # past the checks: fails on the checkpoint
        I.infer(str(tmp_path / "missing.ckpt"), [str(tmp_path)], str(tmp_path / "out"), cfg=cfg, norm_params=params)
    with pytest.raises(ValueError, match="2 channels"):
        I.infer(str(tmp_path / "missing.ckpt"), [str(tmp_path)], str(tmp_path / "out"), cfg=cfg,
                norm_params={"floodplanet": {"S1": {"mean": np.zeros(3), "std": np.ones(3)}}})
    cfg["dataset"]["dataset_kwargs"] = dict(dem=True)
    with pytest.raises(NotImplementedError, match="ms_image"):
        I.infer(str(tmp_path / "missing.ckpt"), [str(tmp_path)], str(tmp_path / "out"), cfg=cfg, norm_params=params)
    assert I.build_parser().parse_args(["c.ckpt", "x.tif", "--out_dir", "o", "--norm_params", "p.p"]).norm_params == "p.p"


def test_device_path_has_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.BandStats(3, "cpu")
