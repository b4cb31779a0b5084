"""CPU: the probability histogram's specification (calibration.prob_histogram_host), the threshold sweep against a
brute-force loop over the float32 probabilities (integer counts equal, not close), tie-breaking, the calibration error on
a hand example, the new C symbols and the command lines of predict --calibrate and infer --water_threshold /
--calibration."""
import json
import os
import re

import numpy as np
import pytest

from floodplanet_code_amd import _lib
from floodplanet_code_amd import calibration as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fu_eval_prob_hist", "fu_prob_hist", "fu_stitch_finalize_maps_ex")


def test_header_and_binding_declare_the_new_symbols_and_abi_stays_5():
    hdr = open(os.path.join(ROOT, "include", "floodunet.h")).read()
    assert int(re.search(r"#define\s+FU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    assert "fu_class_threshold" in hdr and "FU_PROB_HIST_LDS_BYTES" in hdr
    lib = _lib.load()                                    # every listed symbol resolves, or load() raises
    assert lib.fu_abi_version() == 5
    # argument checks that need no device: each names its entry point
    assert lib.fu_eval_prob_hist(None, None, 0, 256, None, None, None) == _lib.FU_ERR_INVALID
    assert b"fu_eval_prob_hist" in lib.fu_last_error()
    assert lib.fu_prob_hist(None, None, 1, 3, 0, 256, None, None, None) == _lib.FU_ERR_INVALID
    assert b"fu_prob_hist" in lib.fu_last_error()
    thr = _lib.FuClassThreshold(1, 0.5)
    assert lib.fu_stitch_finalize_maps_ex(None, None, 3, 2, 2, 1e-5, 1, None, None, None, None, None, thr, None) \
        == _lib.FU_ERR_INVALID
    assert b"fu_stitch_finalize_maps" in lib.fu_last_error()


def _random_case(n, k, seed, n_bins):
    g = np.random.default_rng(seed)
    p = g.random((n, k), dtype=np.float32)
    p /= p.sum(1, keepdims=True)
    edges = (g.integers(0, n_bins + 1, size=(n // 4, k)) / n_bins).astype(np.float32)     # exactly on j / n_bins
    p[: n // 4] = edges
    t = g.integers(-1, k + 1, size=n)                    # -1 and k: out of range
    t[g.random(n) < 0.1] = 255                           # the ignore value
    return p.astype(np.float32), t


@pytest.mark.parametrize("k,n_bins", [(2, 2), (3, 256), (8, 1024), (1, 16)])
def test_host_histogram_counts_every_valid_pixel_once_per_class(k, n_bins):
    p, t = _random_case(3000, k, seed=k + n_bins, n_bins=n_bins)
    hist, top = K.prob_histogram_host(p, t, 255, n_bins)
    n_valid = int(((t != 255) & (t >= 0) & (t < k)).sum())
    assert hist.shape == (k, k, n_bins) and top.shape == (2, n_bins) and hist.dtype == top.dtype == np.int64
    assert 0 < n_valid < len(t)
    for c in range(k):
        assert hist[c].sum() == n_valid
        np.testing.assert_array_equal(hist[c].sum(1), np.bincount(t[(t >= 0) & (t < k) & (t != 255)], minlength=k))
    assert top.sum() == n_valid
    am = p.argmax(1)                                     # numpy's argmax takes the first maximum too
    valid = (t != 255) & (t >= 0) & (t < k)
    assert top[1].sum() == int((am[valid] == t[valid]).sum())


def test_stated_bins_for_edges_zero_one_nan_and_negative():
    n_bins = 8
    vals = np.array([0.0, 1.0, np.nan, -0.25, -0.0, 0.125, 0.124999, 0.5, 0.875, 0.99999, 1.5, np.inf, -np.inf,
                     np.nextafter(np.float32(0.5), np.float32(0))], dtype=np.float32)
    want = [0, 7, 0, 0, 0, 1, 0, 4, 7, 7, 7, 7, 0, 3]
    np.testing.assert_array_equal(K.prob_bins(vals, n_bins), want)
    for j in range(n_bins):                              # j / n_bins sits in bin j: the threshold is a bin's lower edge
        assert K.prob_bins(np.float32(j / n_bins), n_bins) == j
    probs = np.stack([vals, vals], axis=1)               # two classes with the same value: class 0 wins the argmax
    hist, top = K.prob_histogram_host(probs, np.zeros(len(vals), np.int64), -100, n_bins)
    np.testing.assert_array_equal(hist[0, 0], np.bincount(want, minlength=n_bins))
    np.testing.assert_array_equal(hist[1, 0], hist[0, 0])
    assert hist[:, 1].sum() == 0
    # a NaN never wins the argmax: NaN / -inf rows keep class 0 with "probability" -inf -> bin 0, counted as a hit for t = 0
    np.testing.assert_array_equal(top[1], np.bincount(want, minlength=n_bins))
    assert top[0].sum() == 0
    for bad in (0, 1, 3, 100, 2048):
        with pytest.raises(ValueError, match="power of two"):
            K.prob_histogram_host(probs, np.zeros(len(vals), np.int64), -100, bad)


def _brute_force(p, t, cls, n_bins, ignore):
    """Threshold the float32 probabilities themselves at every j / n_bins."""
    k = p.shape[1]
    valid = (t != ignore) & (t >= 0) & (t < k)
    pc, pos = p[valid, cls], t[valid] == cls
    rows = []
    for j in range(n_bins):
        T = np.float32(j / n_bins)
        assert float(T) == j / n_bins                    # the threshold is a float32 number
        with np.errstate(invalid="ignore"):
            d = (pc >= T) if j > 0 else np.ones_like(pos)   # T = 0 declares every counted pixel (NaN and negatives too)
        rows.append((int((d & pos).sum()), int((d & ~pos).sum()), int((~d & pos).sum()), int((~d & ~pos).sum())))
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize("k,n_bins,cls", [(2, 2, 1), (3, 256, 1), (3, 64, 2), (8, 1024, 0)])
def test_sweep_equals_brute_force_thresholding_of_the_float32_probabilities(k, n_bins, cls):
    p, t = _random_case(5000, k, seed=11 * k + cls, n_bins=n_bins)
    p[7, :] = np.nan
    p[8, cls] = -0.5
    hist, _ = K.prob_histogram_host(p, t, 255, n_bins)
    cv = K.curves(hist, cls)
    bf = _brute_force(p, t, cls, n_bins, 255)
    for i, m in enumerate(("tp", "fp", "fn", "tn")):
        assert cv[m].dtype == np.int64
        np.testing.assert_array_equal(cv[m], bf[:, i], err_msg=m)
    np.testing.assert_array_equal(cv["thresholds"], np.arange(n_bins) / n_bins)
    tp, fp, fn = (bf[:, i].astype(np.float64) for i in range(3))
    f1 = np.divide(2 * tp, 2 * tp + fp + fn, out=np.zeros(n_bins), where=(2 * tp + fp + fn) > 0)
    iou = np.divide(tp, tp + fp + fn, out=np.zeros(n_bins), where=(tp + fp + fn) > 0)
    np.testing.assert_array_equal(cv["f1"], f1)
    np.testing.assert_array_equal(cv["iou"], iou)
    for metric, v in (("f1", f1), ("iou", iou)):
        best = max(range(n_bins), key=lambda j: (v[j], -abs(j / n_bins - 0.5), -j))
        assert K.best_threshold(hist, cls, metric) == (best / n_bins, v[best])
    prec = np.divide(tp, tp + fp, out=np.zeros(n_bins), where=(tp + fp) > 0)
    rec = np.divide(tp, tp + fn, out=np.zeros(n_bins), where=(tp + fn) > 0)
    ap, prev = 0.0, 0.0
    for j in range(n_bins - 1, -1, -1):
        ap += (rec[j] - prev) * prec[j]
        prev = rec[j]
    assert K.average_precision(hist, cls) == pytest.approx(ap, rel=1e-12, abs=0)
    assert rec[0] == 1.0 and 0.0 < K.average_precision(hist, cls) <= 1.0


def test_best_threshold_breaks_ties_towards_one_half_then_the_smaller():
    n_bins = 8
    hist = np.zeros((2, 2, n_bins), dtype=np.int64)
    hist[1, 1, 7] = 10                                   # every positive at p = 7/8.., every negative at p < 1/8:
    hist[1, 0, 0] = 10                                   # thresholds 1/8 .. 7/8 are all perfect
    cv = K.curves(hist, 1)
    np.testing.assert_array_equal(cv["f1"], [2 / 3] + [1.0] * 7)
    assert K.best_threshold(hist, 1, "f1") == (0.5, 1.0)
    assert K.best_threshold(hist, 1, "iou") == (0.5, 1.0)
    hist[1, 1, 7], hist[1, 1, 4] = 9, 1                  # a positive at 4/8: thresholds 5/8.. lose it -> 1/8 .. 4/8 tie
    assert K.best_threshold(hist, 1)[0] == 0.5
    hist[1, 1, 4], hist[1, 1, 3] = 0, 1                  # the positive at 3/8 instead: 1/8 .. 3/8 tie -> the nearest, 3/8
    assert K.best_threshold(hist, 1) == (0.375, 1.0)
    h3 = np.zeros((2, 2, n_bins), dtype=np.int64)        # equidistant tie: 3/8 and 5/8 -> the smaller
    h3[1, 1, 6], h3[1, 0, 1] = 4, 4                      # 4 positives high, 4 negatives low, 2 positives at 3/8 and
    h3[1, 1, 3], h3[1, 0, 4] = 2, 3                      # 3 negatives at 4/8.  3/8: tp 6 fp 3; 4/8: tp 4 fp 3 fn 2;
    cv = K.curves(h3, 1)                                 # 5/8: tp 4 fn 2 -> 12/15 == 8/10 > 8/13
    assert cv["f1"][3] == cv["f1"][5] == 0.8 > cv["f1"][4]
    assert K.best_threshold(h3, 1) == (0.375, 0.8)
    with pytest.raises(ValueError):
        K.best_threshold(h3, 1, "accuracy")
    with pytest.raises(ValueError):
        K.curves(h3, 2)


def test_expected_calibration_error_on_a_two_bin_example():
    top = np.array([[30, 10], [10, 50]], dtype=np.int64)  # bin 0 (confidence 0.25): 10 of 40 right; bin 1 (0.75): 50 of 60
    ece = K.expected_calibration_error(top, groups=2)
    assert ece == pytest.approx(0.4 * abs(10 / 40 - 0.25) + 0.6 * abs(50 / 60 - 0.75), abs=1e-15)
    assert K.expected_calibration_error(top, groups=1) == pytest.approx(abs(60 / 100 - (40 * 0.25 + 60 * 0.75) / 100), abs=1e-15)
    assert K.expected_calibration_error(np.zeros((2, 4), np.int64)) == 0.0
    perfect = np.array([[3, 1], [1, 3]], dtype=np.int64)  # accuracy equals the midpoint in both bins
    assert K.expected_calibration_error(perfect, groups=2) == 0.0
    with pytest.raises(ValueError):
        K.expected_calibration_error(np.zeros((3, 4), np.int64))


def test_report_is_json_ready_and_read_back(tmp_path):
    p, t = _random_case(2000, 3, seed=5, n_bins=64)
    hist, top = K.prob_histogram_host(p, t, 255, 64)
    valid = (t != 255) & (t >= 0) & (t < 3)
    conf = np.zeros((3, 3), np.int64)
    np.add.at(conf, (t[valid], p[valid].argmax(1)), 1)
    rep = K.report(hist, top, 1, confusion=conf)
    path = tmp_path / "calibration.json"
    path.write_text(json.dumps(rep))
    back = json.loads(path.read_text())
    assert back["class"] == 1 and back["n_bins"] == 64 and back["hist"] == hist.tolist() and back["top"] == top.tolist()
    cv = K.curves(hist, 1)
    j = int(round(back["best_threshold"] * 64))
    assert back["at_best"]["tp"] == cv["tp"][j] and back["at_half"]["fp"] == cv["fp"][32]
    assert back["best_f1"] == cv["f1"].max() and back["best_iou"] == cv["iou"].max()
    assert back["argmax"]["n_pixels"] == top.sum() == conf.sum() and back["argmax"]["accuracy"] == np.trace(conf) / conf.sum()
    am = p[valid].argmax(1)
    assert (back["argmax"]["tp"], back["argmax"]["fp"], back["argmax"]["fn"]) == (
        int(((am == 1) & (t[valid] == 1)).sum()), int(((am == 1) & (t[valid] != 1)).sum()), int(((am != 1) & (t[valid] == 1)).sum()))
    assert K.report(hist, None, 1)["argmax"] is None and K.report(hist, None, 1)["ece"] is None
    assert K.read_calibration(str(path)) == (1, back["best_threshold"])
    (tmp_path / "other.json").write_text("{}")
    with pytest.raises(ValueError, match="calibration.json"):
        K.read_calibration(str(tmp_path / "other.json"))


def test_command_lines_parse_and_contradictions_raise_before_device_work(tmp_path):
    from floodplanet_code_amd import infer as I
    from floodplanet_code_amd import predict as P
    a = P.build_parser().parse_args(["x.ckpt", "--data_root", "d"])
    assert a.calibrate is None and a.calibrate_bins == 256
    assert P.build_parser().parse_args(["x.ckpt", "--data_root", "d", "--calibrate"]).calibrate == 1
    a = P.build_parser().parse_args(["x.ckpt", "--data_root", "d", "--calibrate", "2", "--calibrate_bins", "64"])
    assert (a.calibrate, a.calibrate_bins) == (2, 64)
    with pytest.raises(ValueError, match="power of two"):    # before the (missing) checkpoint is opened
        P.main(["/nonexistent/checkpoints/x.ckpt", "--data_root", "d", "--calibrate", "--calibrate_bins", "100"])
    with pytest.raises(ValueError, match="negative"):
        P.main(["/nonexistent/checkpoints/x.ckpt", "--data_root", "d", "--calibrate", "-1"])

    base = ["x.ckpt", "scene.tif", "--out_dir", "o"]
    a = I.build_parser().parse_args(base)
    assert a.water_threshold is None and a.threshold_class is None and a.calibration is None
    a = I.build_parser().parse_args(base + ["--water_threshold", "0.35", "--threshold_class", "2"])
    assert (a.water_threshold, a.threshold_class) == (0.35, 2)
    assert I.build_parser().parse_args(base + ["--calibration", "c.json"]).calibration == "c.json"
    assert I.threshold_rule() is None
    assert I.threshold_rule(0.35) == {"class": 1, "threshold": 0.35, "source": "option"}
    assert I.threshold_rule(0.0, 2)["class"] == 2
    cal = tmp_path / "calibration.json"
    cal.write_text(json.dumps({"class": 1, "best_threshold": 0.4375}))
    assert I.threshold_rule(calibration=str(cal)) == {"class": 1, "threshold": 0.4375, "source": str(cal)}
    for kw in (dict(water_threshold=0.5, calibration=str(cal)), dict(threshold_class=1, calibration=str(cal)),
               dict(threshold_class=1), dict(water_threshold=1.5), dict(water_threshold=-0.1),
               dict(water_threshold=float("nan")), dict(water_threshold=0.5, threshold_class=-1)):
        with pytest.raises(ValueError):
            I.threshold_rule(**kw)
    missing = "/nonexistent/checkpoints/x.ckpt"
    with pytest.raises(ValueError, match="excludes"):        # main and infer() check before they open the checkpoint
        I.main([missing, "scene.tif", "--out_dir", "o", "--water_threshold", "0.5", "--calibration", str(cal)])
    with pytest.raises(ValueError, match="needs --water_threshold"):
        I.main([missing, "scene.tif", "--out_dir", "o", "--threshold_class", "1"])
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        I.infer(missing, ["scene.tif"], "o", water_threshold=2.0)
