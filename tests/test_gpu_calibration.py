"""GPU: the probability histogram kernels against calibration.prob_histogram_host (integer counts: exact equality
everywhere), fu_eval_prob_hist against fu_prob_hist on fu_merge_views' single-view probabilities (the identity
include/floodunet.h names as the logits path's oracle), added-to semantics, rejected calls, fu_stitch_finalize_maps_ex
against fu_stitch_finalize_maps and an elementwise torch statement, and predict --calibrate / infer --calibration end to
end on a synthetic tree.

One histogram copy needs (k * k + 2) * n_bins * 4 bytes of LDS and FU_PROB_HIST_LDS_BYTES = 163840 are reserved: of the
grid k in {2, 3, 8} x n_bins in {2, 256, 1024} only (8, 1024) -- 270336 bytes -- is over the limit, and that case asserts
the rejection the header states instead of counts."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd import calibration as K
from floodplanet_code_amd.unet import HipUNet
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IGNORE = 255
LDS_BYTES = 163840
sys.path.insert(0, os.path.dirname(__file__))


def _net(C=2, base=8, seed=3):
    net = HipUNet(C, 3, base_channels=base)
    net.load_state_dict(O.make_state(C, 3, base, True, seed=seed))
    return net.to(DEV).eval()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _case(n, k, n_bins, seed):
    """probs [n, k] and targets [n]: uniform random rows, rows exactly on bin edges, 0, 1 and NaN; targets over
    [-1, k] (both ends out of range) and the ignore value."""
    g = np.random.default_rng(seed)
    p = g.random((n, k), dtype=np.float32)
    kind = g.integers(0, 8, size=n)
    edges = (g.integers(0, n_bins + 1, size=(n, k)) / n_bins).astype(np.float32)
    p[kind == 0] = edges[kind == 0]
    p[kind == 1] = 0.0
    p[kind == 2] = 1.0
    p[(kind == 3) & (g.random(n) < 0.3), 0] = np.nan
    t = g.integers(-1, k + 1, size=n).astype(np.int64)
    t[g.random(n) < 0.1] = IGNORE
    return p, t


def _device_hist(p, t, k, n_bins, offset=0, want=(True, True), fill=0):
    """fu_prob_hist on a device copy of p whose pointer is `offset` floats past an allocation boundary."""
    lib = _lib.load()
    buf = torch.zeros(p.size + offset, dtype=torch.float32, device=DEV)
    buf[offset:] = torch.from_numpy(p).reshape(-1).to(DEV)
    pd = buf[offset:]
    assert pd.data_ptr() % 16 == (4 * offset) % 16
    td = torch.from_numpy(t).to(DEV)
    hist = torch.full((k, k, n_bins), fill, dtype=torch.int64, device=DEV)
    top = torch.full((2, n_bins), fill, dtype=torch.int64, device=DEV)
    rc = lib.fu_prob_hist(pd.data_ptr(), td.data_ptr(), t.shape[0], k, IGNORE, n_bins, hist.data_ptr() if want[0] else None,
                          top.data_ptr() if want[1] else None, _stream())
    torch.cuda.synchronize()
    return rc, hist.cpu().numpy(), top.cpu().numpy()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n_pixels", [1, 255, 4099])
@pytest.mark.parametrize("n_bins", [2, 256, 1024])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_prob_hist_equals_host_specification(k, n_bins, n_pixels, offset):
    p, t = _case(n_pixels, k, n_bins, seed=1000 * k + n_bins + n_pixels)
    rc, hist, top = _device_hist(p, t, k, n_bins, offset, fill=0)
    if (k * k + 2) * n_bins * 4 > LDS_BYTES:             # the stated limit: rejected, nothing launched
        assert (k, n_bins) == (8, 1024)
        assert rc == _lib.FU_ERR_INVALID and b"LDS" in _lib.load().fu_last_error()
        assert not hist.any() and not top.any()
        return
    assert rc == _lib.FU_OK, _lib.load().fu_last_error()
    want_hist, want_top = K.prob_histogram_host(p, t, IGNORE, n_bins)
    np.testing.assert_array_equal(hist, want_hist)
    np.testing.assert_array_equal(top, want_top)
    if n_pixels > 1:
        assert 0 < want_top.sum() < n_pixels


TWO_TURNS = 256 * 4096 + 4099                            # the grid is capped at 256 blocks of 1024 threads x 4 pixels


@pytest.mark.parametrize("k,n_bins,n_pixels,value", [(3, 256, TWO_TURNS, 1.0), (3, 256, 70001, 0.0), (2, 1024, 4099, 0.3),
                                                     (8, 256, 5000, 0.999)])
def test_saturated_input_counts_every_pixel_in_one_bin(k, n_bins, n_pixels, value):
    """Every pixel the same probabilities and the same target: every lane of every wave meets in one bin per histogram
    row (the pre-aggregation path); TWO_TURNS pixels send some blocks round their loop a second time."""
    p = np.full((n_pixels, k), value, dtype=np.float32)
    t = np.full(n_pixels, k - 1, dtype=np.int64)
    rc, hist, top = _device_hist(p, t, k, n_bins)
    assert rc == _lib.FU_OK
    b = int(K.prob_bins(np.float32(value), n_bins))
    want = np.zeros_like(hist)
    want[:, k - 1, b] = n_pixels
    np.testing.assert_array_equal(hist, want)
    want_top = np.zeros_like(top)
    want_top[int(k == 1), b] = n_pixels                  # all equal: class 0 wins the argmax, the target is k - 1
    np.testing.assert_array_equal(top, want_top)
    if n_pixels < 100000:                                # the host statement agrees (skipped where it would take seconds)
        h2, t2 = K.prob_histogram_host(p, t, IGNORE, n_bins)
        np.testing.assert_array_equal(hist, h2)
        np.testing.assert_array_equal(top, t2)


def test_two_dominant_bins_and_an_outlier_per_wave():
    """Waves that hold two large groups and a few strays: several election rounds, then the plain adds."""
    n, k, n_bins = 9000, 3, 256
    g = np.random.default_rng(5)
    p = np.tile(np.array([[0.98, 0.01, 0.01]], np.float32), (n, 1))
    p[(np.arange(n) // 37) % 2 == 1] = [0.02, 0.97, 0.01]
    stray = g.random(n) < 0.05
    p[stray] = g.random((int(stray.sum()), k), dtype=np.float32)
    t = ((np.arange(n) // 37) % 2).astype(np.int64)
    t[g.random(n) < 0.02] = IGNORE
    rc, hist, top = _device_hist(p, t, k, n_bins)
    assert rc == _lib.FU_OK
    want_hist, want_top = K.prob_histogram_host(p, t, IGNORE, n_bins)
    np.testing.assert_array_equal(hist, want_hist)
    np.testing.assert_array_equal(top, want_top)


@pytest.mark.parametrize("shape", [(32, 32), (48, 80)])
def test_logits_entry_equals_probs_entry_on_single_view_probabilities(shape):
    H, W = shape
    B, n_bins = 3, 256
    net = _net()
    g = torch.Generator().manual_seed(H + W)
    x = (torch.rand(B, 2, H, W, generator=g) * 4 - 2).to(DEV)
    target = torch.randint(-1, 4, (B, H, W), generator=g).to(DEV)
    target[0, :3] = IGNORE
    with torch.no_grad():
        net.forward_views(x, [0])
        probs, _ = net.merge_views()                     # one view of code 0: e[c] * inv, rounded once
        h_probs, t_probs = net.prob_histogram(target, IGNORE, n_bins, probs=probs)
        h_views, t_views = net.prob_histogram(target, IGNORE, n_bins)             # the resident logits of the views forward
        net(x)
        h_logits, t_logits = net.prob_histogram(target, IGNORE, n_bins)           # ... and of a plain forward
    torch.cuda.synchronize()
    assert h_probs.shape == (3, 3, n_bins) and t_probs.shape == (2, n_bins) and h_probs.dtype == torch.int64
    for h, t in ((h_views, t_views), (h_logits, t_logits)):
        assert torch.equal(h, h_probs) and torch.equal(t, t_probs)
    want_hist, want_top = K.prob_histogram_host(probs.cpu().numpy(), target.cpu().numpy(), IGNORE, n_bins)
    np.testing.assert_array_equal(h_probs.cpu().numpy(), want_hist)
    np.testing.assert_array_equal(t_probs.cpu().numpy(), want_top)
    n_valid = int(((target != IGNORE) & (target >= 0) & (target < 3)).sum())
    assert int(t_probs.sum()) == n_valid and 0 < n_valid < B * H * W
    with pytest.raises(ValueError):
        net.prob_histogram(target[:, :-1], IGNORE, n_bins)
    with pytest.raises(ValueError):
        net.prob_histogram(target, IGNORE, 100)
    with pytest.raises(ValueError):
        net.prob_histogram(target, IGNORE, n_bins, probs=probs[..., :2])


def test_outputs_are_added_to_and_each_is_optional():
    k, n_bins, n = 3, 64, 3001
    p, t = _case(n, k, n_bins, seed=9)
    want_hist, want_top = K.prob_histogram_host(p, t, IGNORE, n_bins)
    lib = _lib.load()
    pd, td = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
    hist = torch.full((k, k, n_bins), 5, dtype=torch.int64, device=DEV)
    top = torch.full((2, n_bins), 7, dtype=torch.int64, device=DEV)
    for _ in range(2):
        _lib.check(lib.fu_prob_hist(pd.data_ptr(), td.data_ptr(), n, k, IGNORE, n_bins, hist.data_ptr(), top.data_ptr(), _stream()))
    _lib.check(lib.fu_prob_hist(pd.data_ptr(), td.data_ptr(), n, k, IGNORE, n_bins, hist.data_ptr(), None, _stream()))
    _lib.check(lib.fu_prob_hist(pd.data_ptr(), td.data_ptr(), n, k, IGNORE, n_bins, None, top.data_ptr(), _stream()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hist.cpu().numpy(), 5 + 3 * want_hist)
    np.testing.assert_array_equal(top.cpu().numpy(), 7 + 3 * want_top)


def test_rejected_calls_return_an_error_and_leave_the_outputs_untouched():
    lib = _lib.load()
    n = 500
    p9 = torch.rand(n, 9, device=DEV)
    td = torch.zeros(n, dtype=torch.int64, device=DEV)
    hist = torch.full((9 * 9 * 1024,), 7, dtype=torch.int64, device=DEV)
    top = torch.full((2 * 2048,), 7, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()

    def call(k=3, n_bins=256, n_pixels=n, h=hist.data_ptr(), t=top.data_ptr(), probs=p9.data_ptr(), target=td.data_ptr()):
        return lib.fu_prob_hist(probs, target, n_pixels, k, IGNORE, n_bins, h, t, _stream())

    for kw, msg in ((dict(n_bins=100), b"power of two"), (dict(n_bins=0), b"power of two"), (dict(n_bins=1), b"power of two"),
                    (dict(n_bins=2048), b"power of two"), (dict(k=9), b"n_classes"), (dict(k=0), b"n_classes"),
                    (dict(h=None, t=None), b"nothing to write"), (dict(n_pixels=0), b"n_pixels"),
                    (dict(k=8, n_bins=1024), b"LDS"), (dict(probs=None), b"null"), (dict(target=None), b"null"),
                    (dict(probs=p9.data_ptr() + 2), b"misaligned")):
        assert call(**kw) == _lib.FU_ERR_INVALID, kw
        err = lib.fu_last_error()
        assert b"fu_prob_hist" in err and msg in err, (kw, err)
    net = HipUNet(2, 3, base_channels=8).to(DEV).eval()
    net._get_ctx(torch.device(DEV), 1, 32, 32)           # a context that has run no forward yet
    t32 = torch.zeros(1, 32, 32, dtype=torch.int64, device=DEV)
    assert lib.fu_eval_prob_hist(net._ctx, t32.data_ptr(), IGNORE, 256, hist.data_ptr(), top.data_ptr(), _stream()) \
        == _lib.FU_ERR_INVALID
    assert b"no forward pass yet" in lib.fu_last_error()
    with pytest.raises(RuntimeError, match="no forward"):
        net.prob_histogram(t32, IGNORE)
    with torch.no_grad():
        net(torch.zeros(1, 2, 32, 32, device=DEV))
    for kw in (dict(n_bins=48), dict(n_bins=2048), dict(h=None, t=None)):
        a = dict(n_bins=256, h=hist.data_ptr(), t=top.data_ptr())
        a.update(kw)
        assert lib.fu_eval_prob_hist(net._ctx, t32.data_ptr(), IGNORE, a["n_bins"], a["h"], a["t"], _stream()) == _lib.FU_ERR_INVALID
        assert b"fu_eval_prob_hist" in lib.fu_last_error()
    torch.cuda.synchronize()
    assert bool((hist == 7).all()) and bool((top == 7).all())
    assert call() == _lib.FU_OK                           # and an accepted call does run
    torch.cuda.synchronize()
    assert int((top - 7).sum()) == n


# ------------------------------------------------------------------------------------------------------------ finalisation
def _canvas(H, W, k, thr, cls, seed):
    """Raw sums and weights with uncovered pixels, values exactly at the threshold and ties among the other classes."""
    g = np.random.default_rng(seed)
    weight = g.integers(0, 4, size=(H, W)).astype(np.float32)          # 0: uncovered
    v = g.random((H, W, k), dtype=np.float32)
    v /= v.sum(-1, keepdims=True)
    v[2, :, cls] = thr                                   # exactly at the threshold (weight 1 below keeps it exact)
    v[3, :, cls] = np.nextafter(np.float32(thr), np.float32(0))
    weight[2:4] = 1.0
    others = [c for c in range(k) if c != cls]
    v[4:6, :, others] = 0.25                             # ties among the others: the first of them wins
    v[4, :, cls], v[5, :, cls] = 0.1, 0.9
    v[6, :, :] = 0.2                                     # everything tied, below the threshold
    canvas = (v * weight[..., None]).astype(np.float32)
    return canvas, weight


def _finalize(canvas, weight, k, eps, values, thr, ex=True):
    lib = _lib.load()
    H, W = weight.shape
    cv, wt = torch.from_numpy(canvas).to(DEV), torch.from_numpy(weight).to(DEV)
    out = {"cls": torch.full((H, W), 9, dtype=torch.uint8, device=DEV), "prob": torch.full((k, H, W), 9, dtype=torch.uint8, device=DEV),
           "margin": torch.full((H, W), 9, dtype=torch.uint8, device=DEV), "counts": torch.full((k,), 3, dtype=torch.int64, device=DEV)}
    cval = None if values is None else (ctypes.c_uint8 * k)(*values)
    args = (cv.data_ptr(), wt.data_ptr(), k, H, W, eps, 1, cval, out["cls"].data_ptr(), out["prob"].data_ptr(),
            out["margin"].data_ptr(), out["counts"].data_ptr())
    if ex:
        rc = lib.fu_stitch_finalize_maps_ex(*args, thr, _stream())
    else:
        rc = lib.fu_stitch_finalize_maps(*args, _stream())
    torch.cuda.synchronize()
    out["canvas"] = cv
    return rc, out


@pytest.mark.parametrize("values", [None, [0, 255, 255]])
@pytest.mark.parametrize("eps", [1e-5, 0.0])
def test_finalize_maps_ex_without_a_threshold_is_finalize_maps(eps, values):
    canvas, weight = _canvas(17, 23, 3, 0.375, 1, seed=1)
    rc0, a = _finalize(canvas, weight, 3, eps, values, None, ex=False)
    rc1, b = _finalize(canvas, weight, 3, eps, values, None, ex=True)
    assert rc0 == rc1 == _lib.FU_OK
    for name in ("cls", "prob", "margin", "counts"):
        assert torch.equal(a[name], b[name]), name
    assert torch.equal(a["canvas"].view(torch.int32), b["canvas"].view(torch.int32))
    assert not bool((a["cls"] == 9).any())


@pytest.mark.parametrize("values", [None, [0, 255, 128]])
@pytest.mark.parametrize("eps", [1e-5, 0.0])
@pytest.mark.parametrize("cls,thr", [(1, 0.375), (0, 0.5), (2, 0.0), (1, 1.0)])
def test_finalize_maps_ex_applies_the_threshold_rule(cls, thr, eps, values):
    H, W, k = 17, 23, 3
    canvas, weight = _canvas(H, W, k, thr, cls, seed=cls + 2)
    rc, base = _finalize(canvas, weight, k, eps, values, None)
    rc2, got = _finalize(canvas, weight, k, eps, values, _lib.FuClassThreshold(cls, thr))
    assert rc == rc2 == _lib.FU_OK
    v = base["canvas"]                                   # the normalised values, as the kernel compares them
    assert torch.equal(got["canvas"].view(torch.int32), v.view(torch.int32))
    covered = (torch.from_numpy(weight).to(DEV) + np.float32(eps)) > 0
    masked = v.clone()
    masked[..., cls] = -float("inf")
    is_max = masked == masked.max(-1, keepdim=True).values
    other = torch.full((H, W), k, dtype=torch.int64, device=DEV)
    for c in reversed(range(k)):                         # the first maximum over the classes other than cls
        other = torch.where(is_max[..., c], torch.full_like(other, c), other)
    assert bool((is_max.sum(-1) > 1).any()) and int(other.max()) < k and not bool((other == cls).any())
    decided = torch.where(v[..., cls] >= np.float32(thr), torch.full_like(other, cls), other)
    decided = torch.where(covered, decided, torch.zeros_like(decided))
    lut = torch.tensor(values if values is not None else list(range(k)), dtype=torch.uint8, device=DEV)
    assert torch.equal(got["cls"], lut[decided])
    want_counts = 3 + torch.bincount(decided[covered], minlength=k)
    assert torch.equal(got["counts"], want_counts)
    assert torch.equal(got["prob"], base["prob"]) and torch.equal(got["margin"], base["margin"])
    if eps == 0.0:
        assert 0 < int(covered.sum()) < H * W
    if 0.0 < thr < 1.0:
        assert not torch.equal(got["cls"], base["cls"])
        if eps == 0.0:                                   # weight 1, eps 0: the planted values reach the comparison as they are
            assert bool((v[2, :, cls] == np.float32(thr)).all()) and bool((decided[2] == cls).all())   # >=: T itself passes
            assert bool((v[3, :, cls] < np.float32(thr)).all()) and bool((decided[3] != cls).all())


def test_finalize_maps_ex_rejects_bad_thresholds_and_launches_nothing():
    canvas, weight = _canvas(17, 23, 3, 0.5, 1, seed=7)
    for k, thr in ((3, _lib.FuClassThreshold(3, 0.5)), (3, _lib.FuClassThreshold(-1, 0.5)), (3, _lib.FuClassThreshold(1, 1.5)),
                   (3, _lib.FuClassThreshold(1, -0.01)), (3, _lib.FuClassThreshold(1, float("nan"))),
                   (3, _lib.FuClassThreshold(1, float("inf"))), (1, _lib.FuClassThreshold(0, 0.5))):
        cvs = canvas if k == 3 else canvas[..., :1].copy()
        rc, out = _finalize(cvs, weight, k, 1e-5, None, thr)
        assert rc == _lib.FU_ERR_INVALID and b"fu_stitch_finalize_maps_ex" in _lib.load().fu_last_error()
        assert bool((out["cls"] == 9).all()) and bool((out["counts"] == 3).all()) and bool((out["prob"] == 9).all())
        np.testing.assert_array_equal(out["canvas"].cpu().numpy(), cvs)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """As test_gpu_predict's fixture: a one-epoch checkpoint of a 2-channel S1 model and a labelled tree."""
    from tools.tiff_writer import make_floodplanet_tree
    from floodplanet_code_amd.fit import SyntheticTiles, fit_model
    root = str(tmp_path_factory.mktemp("tree"))
    make_floodplanet_tree(root, regions=("RegA", "RegB"), images_per_region=2, label_size=100, s1_size=40)
    exp = str(tmp_path_factory.mktemp("exp"))
    ch = {"ms_image": 2}
    cfg = dict(lr=2e-3, n_epochs=1, batch_size=2, save_topk_models=1, ignore_index=0, crop_height=64, crop_width=64,
               crop_stride=32, eval_region=["RegA", "RegB"], n_workers=0,
               model=dict(name="ms_model", model_kwargs=dict(optimizer_name="adam", base_channels=8, precision="fp32")))
    ckpt = fit_model(cfg, SyntheticTiles(3, 2, ch, 64, 64, DEV, seed=1), SyntheticTiles(1, 2, ch, 64, 64, DEV, seed=2),
                     ch, 3, exp_dir=exp, device=DEV)
    return root, exp, ckpt


def _crop_probabilities(root, ckpt, cfg, bs, tta):
    """Per-crop probabilities [N, H, W, k] and targets on the host, from an independent model instance walking the same
    batches: the device's single-view (or merged) probabilities, read back."""
    from floodplanet_code_amd.datasets import FloodplanetTiles, TileLoader, generate_image_slice_object
    from floodplanet_code_amd.models import WaterSegmentationModel
    ds = FloodplanetTiles(root, "test", generate_image_slice_object(64, 64, 32), eval_region=["RegA", "RegB"], sensor="S1",
                          ignore_index=0, seed_num=0, output_metadata=True)
    m = WaterSegmentationModel.load_from_checkpoint(ckpt, in_channels=ds.n_channels, n_classes=3, lr=cfg["lr"],
                                                    base_channels=8, precision="fp32").to(DEV)
    m._set_model_to_eval()
    probs, targets = [], []
    with torch.no_grad():
        for batch in TileLoader(ds, bs, DEV, shuffle=False, ignore_index=0, device_assembly=True, device_resize=True):
            m.model.forward_views(m._gather_sources(batch), [0] if tta is None else tta)
            p, _ = m.model.merge_views()
            probs.append(p.cpu().numpy())
            targets.append(batch["target"].cpu().numpy())
    return np.concatenate(probs), np.concatenate(targets), m._loss_ignore


def _host_point(p, t, ignore, cls, thr):
    valid = (t != ignore) & (t >= 0) & (t < p.shape[-1])
    d, pos = (p[..., cls] >= np.float32(thr)) | (thr == 0), t == cls
    return {"tp": int((d & pos & valid).sum()), "fp": int((d & ~pos & valid).sum()), "fn": int((~d & pos & valid).sum())}


@pytest.mark.parametrize("tta", [None, "flips"])
def test_predict_calibrate_writes_the_sweep_of_the_crop_probabilities(trained, tta):
    from floodplanet_code_amd import predict as P
    root, exp, ckpt = trained
    cfg = P.resolve_cfg(exp, ckpt)
    kw = dict(predict_images=False, eval_dataset_split="test", n_workers=0, data_root=root, batch_size=5, device=DEV, tta=tta)
    plain = P.predict(cfg, exp, ckpt, "floodplanet", **kw)
    d = plain["pred_dir"]
    cal_path = os.path.join(d, "calibration.json")
    if os.path.exists(cal_path):                         # the other parametrisation's: this run must not write one
        os.remove(cal_path)
        plain = P.predict(cfg, exp, ckpt, "floodplanet", **kw)
    assert not os.path.exists(cal_path) and "best_threshold" not in plain
    shared = ("metrics.json", "ranked_images_F1-score.txt", "ranked_images_mIoU.txt", "ranked_regions_F1-Score.txt",
              "ranked_regions_iou.txt")
    before = {f: open(os.path.join(d, f), "rb").read() for f in shared}
    out = P.predict(cfg, exp, ckpt, "floodplanet", calibrate=1, **kw)
    assert out["pred_dir"] == d and out["metrics"] == plain["metrics"]
    assert {f: open(os.path.join(d, f), "rb").read() for f in shared} == before       # metrics.json is unchanged
    rep = json.load(open(cal_path))
    assert rep["class"] == 1 and rep["n_bins"] == 256 and out["best_threshold"] == rep["best_threshold"]
    assert out["best_f1"] == rep["best_f1"] and rep.get("tta") == tta

    from floodplanet_code_amd.tta import view_codes
    p, t, ignore = _crop_probabilities(root, ckpt, cfg, 5, None if tta is None else view_codes(tta, 64, 64))
    assert p.shape[0] > 5 and p.shape[0] % 5 != 0        # the last batch is partial
    want_hist, want_top = K.prob_histogram_host(p, t, ignore, 256)
    np.testing.assert_array_equal(np.array(rep["hist"]), want_hist)
    np.testing.assert_array_equal(np.array(rep["top"]), want_top)
    for key, thr in (("at_half", 0.5), ("at_best", rep["best_threshold"])):
        assert rep[key]["threshold"] == thr
        assert {m: rep[key][m] for m in ("tp", "fp", "fn")} == _host_point(p, t, ignore, 1, thr), key
    valid = (t != ignore) & (t >= 0) & (t < 3)
    am = p.argmax(-1)                                    # numpy takes the first maximum, as the kernels do
    assert {m: rep["argmax"][m] for m in ("tp", "fp", "fn")} == {
        "tp": int((valid & (am == 1) & (t == 1)).sum()), "fp": int((valid & (am == 1) & (t != 1)).sum()),
        "fn": int((valid & (am != 1) & (t == 1)).sum())}
    assert rep["argmax"]["n_pixels"] == int(valid.sum())
    assert rep["n_pixels"] == rep["at_half"]["tp"] + rep["at_half"]["fp"] + rep["at_half"]["fn"] + rep["at_half"]["tn"] > 0
    with pytest.raises(ValueError):
        P.predict(cfg, exp, ckpt, "floodplanet", calibrate=1, calibrate_bins=100, **kw)
    with pytest.raises(ValueError):
        P.predict(cfg, exp, ckpt, "floodplanet", calibrate=3, **kw)


def test_infer_applies_the_calibrated_threshold_and_is_unchanged_without_it(trained, tmp_path):
    from floodplanet_code_amd import infer as I
    from floodplanet_code_amd import predict as P
    from floodplanet_code_amd.datasets.tiff import read_tiff
    root, exp, ckpt = trained
    cfg = P.resolve_cfg(exp, ckpt)
    paths = [os.path.join(root, "CSDAP_complete")]
    kw = dict(cfg=cfg, size=(100, 100), stride=32, batch_size=9, write_probs="f32", write_margin=True)

    def files(out_dir):
        found = {}
        for d, _, names in os.walk(out_dir):
            for f in names:
                if f.endswith(".tif"):
                    found[os.path.relpath(os.path.join(d, f), out_dir)] = open(os.path.join(d, f), "rb").read()
        return found

    scene_paths = sorted(p for p in I.find_inputs(paths) if os.sep + "S1" + os.sep in p)
    a = I.infer(ckpt, scene_paths, str(tmp_path / "a"), **kw)
    b = I.infer(ckpt, scene_paths, str(tmp_path / "b"), **kw)
    fa, fb = files(str(tmp_path / "a")), files(str(tmp_path / "b"))
    assert len(fa) == 3 * len(scene_paths) >= 12 and fa == fb and "threshold" not in a and "threshold" not in b
    assert [r["class_pixels"] for r in a["scenes"]] == [r["class_pixels"] for r in b["scenes"]]

    pred = P.predict(cfg, exp, ckpt, "floodplanet", predict_images=False, eval_dataset_split="test", n_workers=0,
                     data_root=root, batch_size=9, device=DEV, calibrate=1)
    written = os.path.join(pred["pred_dir"], "calibration.json")
    zero = tmp_path / "calibration.json"                 # and the end of the range: everything counted is water
    zero.write_text(json.dumps({"class": 1, "best_threshold": 0.0}))
    changed = 0
    for name, cal, thr in (("best", written, pred["best_threshold"]), ("zero", str(zero), 0.0)):
        out_dir = str(tmp_path / name)
        out = I.infer(ckpt, scene_paths, out_dir, calibration=cal, **kw)
        assert out["threshold"] == {"class": 1, "threshold": thr, "source": cal}
        assert json.load(open(os.path.join(out_dir, "summary.json")))["threshold"] == out["threshold"]
        ft = files(out_dir)
        for rec in out["scenes"]:
            for side in ("probabilities", "margin"):     # the probability and margin rasters do not change
                rel = os.path.relpath(rec[side], out_dir)
                assert ft[rel] == fa[rel], rel
            v = read_tiff(rec["probabilities"])          # [k, H, W] float32: what the kernel compared
            other = np.where(v[2] > v[0], 2, 0)          # first maximum over the classes other than 1
            decided = np.where(v[1] >= np.float32(thr), 1, other)
            np.testing.assert_array_equal(read_tiff(rec["output"]), (np.clip(decided, 0, 1) * 255).astype(np.uint8))
            assert rec["class_pixels"] == np.bincount(decided.ravel(), minlength=3).tolist()
            changed += int((decided != v.argmax(0)).sum())
    assert changed > 0
    same = I.infer(ckpt, scene_paths, str(tmp_path / "opt"), water_threshold=pred["best_threshold"], threshold_class=1, **kw)
    assert files(str(tmp_path / "opt")) == files(str(tmp_path / "best")) and same["threshold"]["source"] == "option"
    with pytest.raises(ValueError, match="not in 0..2"):
        I.infer(ckpt, scene_paths, str(tmp_path / "bad"), water_threshold=0.5, threshold_class=3, **kw)
