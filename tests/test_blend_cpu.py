"""CPU: window-weighted blending's host side -- stitch.blend_window against the restated formulas, the seam property on the
numpy reference, the argument checks of fu_stitch_add_batch_windowed / fu_stitch_finalize_maps that need no context, and
infer's new options."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from floodplanet_code_amd import _lib
from floodplanet_code_amd import infer as I
from floodplanet_code_amd import stitch as S

sys.path.insert(0, os.path.dirname(__file__))
from tools import blend_ref as R  # noqa: E402

KINDS = ("uniform", "linear", "hann")


@pytest.mark.parametrize("n", [1, 2, 31, 32, 256, 512])
@pytest.mark.parametrize("kind", KINDS)
def test_blend_window_properties_and_restated_formula(kind, n):
    w = S.blend_window(kind, n)
    assert w.dtype == np.float32 and w.shape == (n,)
    np.testing.assert_array_equal(w, w[::-1])                 # symmetric
    assert float(w.min()) > 0 and float(w.max()) <= 1         # strictly positive: a covered pixel has a positive weight
    if kind == "linear":
        assert float(w.max()) == 1.0
    if kind == "uniform":
        assert bool((w == 1).all())
    want = R.window(kind, n)
    assert want.dtype == np.float32
    np.testing.assert_array_equal(w.view(np.uint32), want.view(np.uint32))      # bit for bit


def test_blend_window_hann_corner_is_a_normal_float():
    w = S.blend_window("hann", 512)
    assert 9.3e-6 < float(w.min()) < 9.5e-6
    corner = np.float32(w[0]) * np.float32(w[0])
    assert corner > np.finfo(np.float32).tiny                 # 8.9e-11: eps = 0 divides by a normal number


def test_blend_window_rejects_unknown_kinds():
    with pytest.raises(ValueError, match="cubic"):
        S.blend_window("cubic", 8)
    with pytest.raises(ValueError):
        S.blend_window("hann", 0)
    with pytest.raises(ValueError, match="blend"):
        S.GpuImageStitcher(None, "cpu", blend="cubic")


@pytest.mark.parametrize("kind,largest", [("uniform", 0.5), ("linear", 0.1), ("hann", 0.1)])
def test_seam_between_two_disagreeing_crops(kind, largest):
    """Two 32 x 32 crops at columns 0 and 16 that predict (1, 0, 0) and (0, 1, 0): equal weights step by 0.5 where the
    overlap ends; a window ramps (1 / 17 = 0.059 for the triangle, 0.098 for the raised cosine)."""
    probs = np.zeros((2, 32, 32, 3), np.float32)
    probs[0, ..., 0] = 1
    probs[1, ..., 1] = 1
    win = R.window(kind, 32)
    out, _, weight = R.stitch_blend_reference(probs, [(0, 0, 32, 32), (0, 16, 32, 48)], 32, 48, win, win)
    assert out.dtype == np.float32 and float(weight.min()) > 0
    jump = float(np.abs(np.diff(out[..., 1], axis=1)).max())
    if kind == "uniform":
        assert jump == 0.5
    else:
        assert jump <= largest
        assert jump == pytest.approx({"linear": 1 / 17, "hann": 0.098}[kind], abs=1e-3)
    np.testing.assert_allclose(out.sum(-1), 1.0, rtol=0, atol=1e-6)
    # one crop only: its own value, up to the rounding of w * (1 / w)
    np.testing.assert_allclose(out[:, :16, 0], 1.0, rtol=0, atol=2e-7)
    np.testing.assert_allclose(out[:, 32:, 1], 1.0, rtol=0, atol=2e-7)


def test_new_entries_reject_bad_arguments_without_context():
    lib = _lib.load()
    table = (_lib.FuStitchEntry * 1)()
    assert lib.fu_stitch_add_batch_windowed(None, 1, table, None, 0, None, None, None) == _lib.FU_ERR_INVALID
    assert b"fu_stitch_add_batch_windowed" in lib.fu_last_error()
    canvas = (ctypes.c_float * 12)()                           # host memory: a rejected call never touches it
    weight = (ctypes.c_float * 4)()
    cls = (ctypes.c_uint8 * 4)(7, 7, 7, 7)
    cv, wt, co = (ctypes.addressof(a) for a in (canvas, weight, cls))

    def call(canvas=cv, weight=wt, k=3, eps=1e-5, norm=0, class_out=co):
        return lib.fu_stitch_finalize_maps(canvas, weight, k, 2, 2, eps, norm, None, class_out, None, None, None, None)

    cases = {"no output": dict(class_out=None), "eps < 0": dict(eps=-1e-5), "eps nan": dict(eps=float("nan")),
             "eps inf": dict(eps=float("inf")), "0 classes": dict(k=0), "9 classes": dict(k=9),
             "null canvas": dict(canvas=None), "null weight": dict(weight=None)}
    for name, kw in cases.items():
        assert call(**kw) == _lib.FU_ERR_INVALID, name
        assert b"fu_stitch_finalize_maps" in lib.fu_last_error(), name
    assert list(cls) == [7, 7, 7, 7]
    hdr = open(os.path.join(ROOT, "include", "floodunet.h")).read()
    assert int(re.search(r"#define\s+FU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5 == lib.fu_abi_version()
    for name in ("fu_stitch_add_batch_windowed", "fu_stitch_finalize_maps"):
        assert name in hdr and name in _lib.SIGNATURES


def test_infer_cli_accepts_the_new_flags_and_the_stride_rule():
    ap = I.build_parser()
    a = ap.parse_args(["c.ckpt", "x.tif", "--out_dir", "o"])
    assert a.blend == "uniform" and a.write_probs is None and a.write_margin is False and a.stride is None
    a = ap.parse_args(["c.ckpt", "x.tif", "--out_dir", "o", "--blend", "hann", "--write_probs", "u8", "--write_margin"])
    assert a.blend == "hann" and a.write_probs == "u8" and a.write_margin is True
    assert ap.parse_args(["c.ckpt", "x.tif", "--out_dir", "o", "--write_probs", "f32"]).write_probs == "f32"
    for bad in (["--blend", "cubic"], ["--write_probs", "f16"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["c.ckpt", "x.tif", "--out_dir", "o"] + bad)
    assert I.default_stride(64, 48) == 48 and I.default_stride(64, 48, "uniform") == 48
    assert I.default_stride(64, 48, "linear") == 24 and I.default_stride(512, 512, "hann") == 256
    assert I.default_stride(64, 48, "hann", 40) == 40 and I.default_stride(64, 48, "uniform", 7) == 7
    assert I.side_output_path("/o/R_pred/a.b.tif", "prob") == "/o/R_pred/a.b_prob.tif"
    from floodplanet_code_amd import predict as P
    assert P.build_parser().parse_args(["c.ckpt", "--data_root", "d", "--blend", "linear"]).blend == "linear"


@pytest.mark.parametrize("kwargs,match", [(dict(blend="cubic"), "blend"), (dict(write_probs="f16"), "write_probs")])
def test_infer_rejects_unknown_values_before_gpu_work(kwargs, match, tmp_path, monkeypatch):
    import torch
    calls = []
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: calls.append("stream"))
    cfg = dict(crop_height=64, crop_width=64, batch_size=4, norm_mode=None,
               dataset=dict(name="floodplanet", channels="ALL", sensor="S1", dataset_kwargs=None),
               model=dict(name="ms_model", model_kwargs=dict(base_channels=8)))
    with pytest.raises(ValueError, match=match):
        I.infer(str(tmp_path / "missing.ckpt"), [str(tmp_path)], str(tmp_path / "out"), cfg=cfg, **kwargs)
    assert not calls and not (tmp_path / "out").exists()
