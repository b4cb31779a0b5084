"""GPU: fu_band_stats through the C ABI against the numpy statement of its contract (datasets.stats.band_stats_host) and
the reference's fixture; streaming and bit-reproducibility; percentiles; rejected calls; and norm_mode 'global' end to
end (parameters computed on the device -> TileLoader's device assembly -> predict / infer)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from floodplanet_code_amd import _lib
from floodplanet_code_amd.datasets import stats as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
sys.path.insert(0, os.path.dirname(__file__))


def fixture():
    z = np.load(os.path.join(GOLDEN, "loader_normstats_golden.npz"))
    q = np.float32(int(z["q"]))
    srcs = [z[k].astype(np.float32) / q for k in ("image_q", "dem_q", "slope_q")]
    return z, srcs, (z["valid_h"], z["valid_w"])


def _dev(srcs):
    return [torch.from_numpy(np.ascontiguousarray(s)).to(DEV) for s in srcs]


def _compare(st, want, tag=""):
    """Integers exact, mean / std to 1e-9 relative (fp64 sums of <= 2^26 terms in [0, 1]; var = E[x^2] - mean^2 amplifies
    rounding by E[x^2] / var <= 101 for std >= 0.1 mean)."""
    got = st.result()
    torch.cuda.synchronize()
    print(tag, "mean rel", np.abs(got["mean"] / want["mean"] - 1).max(), "std rel", np.abs(got["std"] / want["std"] - 1).max())
    np.testing.assert_array_equal(got["count"], want["count"], err_msg=tag)
    np.testing.assert_array_equal(got["n_nonfinite"], want["n_nonfinite"], err_msg=tag)
    np.testing.assert_array_equal(got["min"], want["min"], err_msg=tag)
    np.testing.assert_array_equal(got["max"], want["max"], err_msg=tag)
    if st.hist is not None:
        np.testing.assert_array_equal(st.histogram(), want["hist"], err_msg=tag)
    np.testing.assert_allclose(got["mean"], want["mean"], rtol=1e-9, atol=0, err_msg=tag)
    np.testing.assert_allclose(got["std"], want["std"], rtol=1e-9, atol=0, err_msg=tag)
    return got


def test_fixture_statistics_equal_host_and_reference():
    z, srcs, valid = fixture()
    st = S.BandStats(5, DEV, mask="nonzero").update(_dev(srcs), valid)
    got = _compare(st, S.band_stats_host(srcs, valid, mask="nonzero"), "fixture")
    assert got["count"][0] == int(z["f64_count"])
    np.testing.assert_allclose(got["mean"], z["ref_mean"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(got["std"], z["ref_std"], rtol=1e-6, atol=0)
    # the image alone, padded items without valid sizes (what the reference's data set hands over)
    st1 = S.BandStats(3, DEV, mask="nonzero").update(_dev(srcs[:1]))
    np.testing.assert_allclose(st1.result()["mean"], z["ref_mean"][:3], rtol=1e-6, atol=0)
    np.testing.assert_allclose(st1.result()["std"], z["ref_std"][:3], rtol=1e-6, atol=0)


def _random_batch(g, B, chans, H, W, bad=True):
    srcs = []
    for k, c in enumerate(chans):
        x = (0.1 + 0.8 * g.random((B, c, H, W))).astype(np.float32)
        if k == 1:
            x = (x ** 2).astype(np.float32)
        srcs.append(x)
    holes = g.random((B, H, W)) < 0.03
    srcs[0][np.broadcast_to(holes[:, None], srcs[0].shape)] = 0.0          # no-data pixels of the first source
    srcs[-1][0, 0, 0, 0], srcs[-1][B - 1, 0, H - 1, W - 1] = -0.25, 1.5     # beyond the histogram's range: edge bins
    if bad:
        srcs[0][0, 0, 1, 2] = np.nan
        srcs[-1][B - 1, -1, 2, 1] = np.inf
        srcs[-1][B // 2, 0, H // 2, W // 2] = -np.inf
    vh = g.integers(1, H + 1, size=B).astype(np.int32)
    vw = g.integers(1, W + 1, size=B).astype(np.int32)
    vh[0], vw[0], vh[-1], vw[-1] = H, W, H, W
    return srcs, (vh, vw)


@pytest.mark.parametrize("mask", [None, "nonzero"])
@pytest.mark.parametrize("B,chans,H,W", [(3, (2,), 37, 45), (5, (4, 1), 37, 45), (4, (3, 1, 1), 64, 64), (2, (8,), 40, 100),
                                         (3, (10, 2, 4), 33, 36), (6, (9,), 128, 128)])
def test_random_batches_equal_host(mask, B, chans, H, W):
    g = np.random.default_rng(B * 1000 + H + len(chans))
    srcs, valid = _random_batch(g, B, chans, H, W)
    for use_valid in (True, False):
        for bins in (4096, 300, None):
            v = valid if use_valid else None
            st = S.BandStats(sum(chans), DEV, bins=bins, mask=mask).update(_dev(srcs), v)
            want = S.band_stats_host(srcs, v, bins=bins, mask=mask)
            assert want["n_nonfinite"][0] >= 2
            _compare(st, want, f"{mask} {chans} {H}x{W} valid={use_valid} bins={bins}")


def test_unaligned_sources_take_the_scalar_path_with_the_same_result():
    g = np.random.default_rng(5)
    srcs, valid = _random_batch(g, 3, (3, 2), 32, 64)
    flat = [torch.zeros(s.size + 1, device=DEV) for s in srcs]
    views = []
    for f, s in zip(flat, srcs):
        f[1:] = torch.from_numpy(s).to(DEV).view(-1)
        views.append(f[1:].view(*s.shape))
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views)
    a = S.BandStats(5, DEV).update(views, valid)
    b = S.BandStats(5, DEV).update(_dev(srcs), valid)
    want = S.band_stats_host(srcs, valid)
    _compare(a, want, "unaligned")
    _compare(b, want, "aligned")


def test_streaming_and_bit_reproducibility():
    _, srcs, valid = fixture()
    dev = _dev(srcs)
    want = S.band_stats_host(srcs, valid)

    def run(chunks):
        st = S.BandStats(5, DEV)
        for a, b in chunks:
            st.update([d[a:b] for d in dev], (valid[0][a:b], valid[1][a:b]))
        return st

    one, three = run([(0, 12)]), run([(0, 4), (4, 8), (8, 12)])
    _compare(one, want, "one call")
    _compare(three, want, "three calls")
    for k in ("count", "min", "max", "n_nonfinite"):
        np.testing.assert_array_equal(one.result()[k], three.result()[k])
    np.testing.assert_array_equal(one.histogram(), three.histogram())
    for chunks in ([(0, 12)], [(0, 4), (4, 8), (8, 12)], [(0, 5), (5, 12), (0, 12)]):
        assert run(chunks).state_bytes() == run(chunks).state_bytes(), chunks          # bit-identical accumulators
    # a larger batch that fills every workgroup of the grid, twice
    g = np.random.default_rng(11)
    big = [torch.from_numpy(g.random((16, 8, 256, 256), dtype=np.float32)).to(DEV)]
    a = S.BandStats(8, DEV).update(big).update(big).state_bytes()
    b = S.BandStats(8, DEV).update(big).update(big).state_bytes()
    assert a == b


def test_percentiles_and_non_finite_pixels():
    g = np.random.default_rng(3)
    srcs, valid = _random_batch(g, 6, (3, 1), 96, 80)
    want = S.band_stats_host(srcs, valid, return_pixels=True)
    st = S.BandStats(4, DEV).update(_dev(srcs), valid)
    assert (st.result()["n_nonfinite"] == want["n_nonfinite"]).all() and want["n_nonfinite"][0] >= 2
    assert np.isfinite(st.result()["mean"]).all()
    pix = np.clip(want["pixels"].astype(np.float64), 0.0, 1.0)
    for q in (5, 50, 95):
        got = st.percentile(q)
        ref = np.percentile(pix, q, axis=1)
        print("q", q, "max |diff| in bins", np.abs(got - ref).max() * 4096)
        assert np.abs(got - ref).max() <= 1.0 / 4096, q
    with pytest.raises(RuntimeError, match="without a histogram"):
        S.BandStats(4, DEV, bins=None).percentile(50)


def test_bad_arguments_are_rejected_and_nothing_is_touched():
    lib = _lib.load()
    x = torch.rand(2, 3, 16, 16, device=DEV)
    st = S.BandStats(3, DEV, bins=64)
    st.update([x])
    torch.cuda.synchronize()
    before = st.state_bytes()
    stream = torch.cuda.current_stream().cuda_stream
    ws, wsn = st._workspace.data_ptr(), st._workspace.numel()

    def call(srcs=(x,), chans=(3,), n_src=None, B=2, H=16, W=16, mask=1, acc=None, ws=ws, wsn=wsn, **fields):
        arr = (C.c_void_p * 8)(*[s.data_ptr() if s is not None else None for s in srcs])
        chs = (C.c_int32 * 8)(*chans)
        a = acc if acc is not None else _lib.FuBandAccum.from_buffer_copy(st._acc)
        for k, v in fields.items():
            setattr(a, k, v)
        return lib.fu_band_stats(arr, chs, len(srcs) if n_src is None else n_src, B, H, W, None, None, mask,
                                 C.byref(a), ws, wsn, stream)

    assert call() == _lib.FU_OK
    torch.cuda.synchronize()
    after_one = st.state_bytes()
    assert after_one != before
    cases = [(dict(B=0), "B = 0"), (dict(H=0), "H = 0"), (dict(W=-3), "W = -3"), (dict(n_src=0), "sources"),
             (dict(n_src=9), "sources"), (dict(srcs=(None,)), "bad source"), (dict(chans=(0,)), "bad source"),
             (dict(srcs=(x, x, x, x, x, x), chans=(3,) * 6), "18 channels"), (dict(mask=2), "mask_mode"),
             (dict(n_bins=0), "n_bins"), (dict(n_bins=1 << 20), "n_bins"), (dict(hi=0.0), "lo < hi"),
             (dict(lo=2.0), "lo < hi"), (dict(hi=float("nan")), "lo < hi"), (dict(count=None), "missing accumulators"),
             (dict(sumsq=None), "missing accumulators"), (dict(vmax=None), "missing accumulators"),
             (dict(ws=None), "workspace"), (dict(wsn=1024), "workspace"), (dict(ws=ws + 4), "workspace")]
    for kw, msg in cases:
        assert call(**kw) == _lib.FU_ERR_INVALID, kw
        assert msg.encode() in lib.fu_last_error(), (kw, lib.fu_last_error())
    assert lib.fu_band_stats(None, None, 1, 2, 16, 16, None, None, 0, None, ws, wsn, stream) == _lib.FU_ERR_INVALID
    torch.cuda.synchronize()
    assert st.state_bytes() == after_one                                    # nothing ran
    with pytest.raises(ValueError, match="channels"):
        st.update([x, x])
    assert lib.fu_band_stats_workspace_bytes(3, 64) <= wsn and lib.fu_band_stats_workspace_bytes(0, 64) == 0


# ------------------------------------------------------------------------------------------------------------ end to end
def _tree(tmp_path, **kw):
    from tools.tiff_writer import make_floodplanet_tree
    root = str(tmp_path)
    make_floodplanet_tree(root, regions=("RegA", "RegB"), images_per_region=2, **kw)
    return root


@pytest.mark.parametrize("device_resize", [False, True])
def test_compute_norm_params_equals_host_over_the_whole_data_set(tmp_path, device_resize):
    from floodplanet_code_amd.datasets import FloodplanetTiles, generate_image_slice_object
    root = _tree(tmp_path, label_size=90, s1_size=37)
    ds = FloodplanetTiles(root, "all", generate_image_slice_object(32, 32, 32), eval_region=["RegA"], sensor="S1",
                          ignore_index=0)
    params, st = S.compute_norm_params(ds, DEV, batch_size=5, device_resize=device_resize, return_stats=True)
    raws = [ds.raw_item(i)["raw"].numpy() for i in range(len(ds))]
    tot = None
    for r in raws:                                                          # item by item: the crops differ in size
        h = S.band_stats_host([r[None]], None, mask="nonzero")
        tot = h if tot is None else {k: (np.minimum(tot[k], h[k]) if k == "min" else np.maximum(tot[k], h[k]) if k == "max"
                                         else tot[k] + h[k]) for k in ("count", "sum", "sumsq", "min", "max", "hist")}
    mean, std = S.finalize(tot["count"], tot["sum"], tot["sumsq"])
    got = st.result()
    assert set(params) == {"S1"} and params["S1"]["mean"].dtype == np.float64 and params["S1"]["mean"].shape == (2,)
    # (with device_resize the tiles are resampled on the device, bit for bit the host's: the integers stay exact)
    np.testing.assert_array_equal(got["count"], tot["count"])
    np.testing.assert_array_equal(st.histogram(), tot["hist"])
    np.testing.assert_allclose(params["S1"]["mean"], mean, rtol=1e-9, atol=0)
    np.testing.assert_allclose(params["S1"]["std"], std, rtol=1e-9, atol=0)
    np.testing.assert_array_equal(got["min"], tot["min"])
    np.testing.assert_array_equal(got["max"], tot["max"])


def test_tileloader_global_equals_host_items_with_fp32_parameters(tmp_path):
    from floodplanet_code_amd.datasets import FloodplanetTiles, TileLoader, generate_image_slice_object
    root = _tree(tmp_path, label_size=90, s1_size=37)
    sp = generate_image_slice_object(32, 32, 24)
    kw = dict(eval_region=["RegA", "RegB"], sensor="S1", ignore_index=0, output_metadata=True)
    params = {"floodplanet": S.compute_norm_params(FloodplanetTiles(root, "all", sp, **kw), DEV)}
    ds = FloodplanetTiles(root, "all", sp, norm_mode="global", norm_params=params, **kw)
    m32 = params["floodplanet"]["S1"]["mean"].astype(np.float32)[:, None, None]
    s32 = params["floodplanet"]["S1"]["std"].astype(np.float32)[:, None, None]
    for resize in (False, True):
        n = 0
        for batch in TileLoader(ds, 7, DEV, device_assembly=True, device_resize=resize):
            for b, md in enumerate(batch["metadata"]):
                i = [k for k, ex in enumerate(ds.dataset) if ex["image_path"] == md["image_path"]
                     and ex["crop_params"].h0 == md["crop_params"].h0 and ex["crop_params"].w0 == md["crop_params"].w0][0]
                raw = ds.raw_item(i)["raw"].numpy()
                want = np.zeros((2, 32, 32), np.float32)
                want[:, :raw.shape[1], :raw.shape[2]] = (raw - m32) / s32   # two float32 operations, as the kernel's
                np.testing.assert_array_equal(batch["image"][b].cpu().numpy(), want)
                np.testing.assert_array_equal(batch["mean"][b].cpu().numpy(), m32)
                np.testing.assert_array_equal(batch["std"][b].cpu().numpy(), s32)
                np.testing.assert_allclose(batch["image"][b].cpu().numpy(), ds[i]["image"].numpy(), rtol=0, atol=1e-5)
                n += 1
        assert n == len(ds)


def test_infer_with_global_norm_equals_predict_bit_for_bit(tmp_path):
    """As tests/test_gpu_infer.py's test_infer_canvases_equal_predict_bit_for_bit, in norm_mode 'global'."""
    from floodplanet_code_amd import infer as I
    from floodplanet_code_amd import predict as P
    from floodplanet_code_amd.datasets import FloodplanetTiles, generate_image_slice_object
    from floodplanet_code_amd.fit import SyntheticTiles, fit_model
    root = _tree(tmp_path / "tree", label_size=100, s1_size=40)
    exp = str(tmp_path / "exp")
    ch = {"ms_image": 2}
    cfg = dict(lr=2e-3, n_epochs=1, batch_size=2, save_topk_models=1, ignore_index=0, crop_height=64, crop_width=64,
               crop_stride=32, eval_region=["RegA", "RegB"], n_workers=0,
               model=dict(name="ms_model", model_kwargs=dict(optimizer_name="adam", base_channels=8, precision="fp32")))
    ckpt = fit_model(cfg, SyntheticTiles(3, 2, ch, 64, 64, DEV, seed=1), SyntheticTiles(1, 2, ch, 64, 64, DEV, seed=2),
                     ch, 3, exp_dir=exp, device=DEV)
    ds = FloodplanetTiles(root, "all", generate_image_slice_object(64, 64, 64), eval_region=["RegA", "RegB"], sensor="S1",
                          ignore_index=0)
    path = str(tmp_path / "dataset_norm_params.p")
    S.save_norm_params(path, "floodplanet", S.compute_norm_params(ds, DEV, device_resize=True))
    cfg = P.resolve_cfg(exp, ckpt)
    cfg["norm_mode"] = "global"
    with pytest.raises(NotImplementedError):
        P.predict(cfg, exp, ckpt, "floodplanet", predict_images=True, data_root=root, batch_size=9, device=DEV)
    cfg["norm_params"] = path
    pred = P.predict(cfg, exp, ckpt, "floodplanet", predict_images=True, eval_dataset_split="test", n_workers=0,
                     data_root=root, batch_size=9, device=DEV)["probabilities"]
    plain = P.predict(dict(cfg, norm_mode=None), exp, ckpt, "floodplanet", predict_images=True, eval_dataset_split="test",
                      n_workers=0, data_root=root, batch_size=9, device=DEV)["probabilities"]
    paths = sorted(os.path.join(root, "CSDAP_complete", key.split("/")[0], "S1", key.split("/")[1] + ".tif") for key in pred)
    del cfg["norm_params"]
    out = I.infer(ckpt, paths, str(tmp_path / "out"), cfg=cfg, size=(100, 100), stride=32, batch_size=9,
                  keep_probabilities=True, norm_params=path)
    assert out["n_scenes"] == len(pred) == 4
    for rec in out["scenes"]:
        region = os.path.basename(os.path.dirname(os.path.dirname(rec["input"])))
        name = os.path.splitext(os.path.basename(rec["input"]))[0]
        np.testing.assert_array_equal(out["probabilities"][rec["output"]], pred[f"{region}/{name}"])
        assert not np.array_equal(pred[f"{region}/{name}"], plain[f"{region}/{name}"])      # the mode changes the input
