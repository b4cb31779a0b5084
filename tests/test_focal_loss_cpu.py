"""CPU: the host side of the focal cross entropy (fu_loss_ce_focal) -- the C ABI declarations, the fp64 specification
(tests/tools/focal_ref.py) against torch's cross entropy, its closed-form gradient and a hand-computed case, the model
constructors' checks and the fit command line.  No GPU."""
import math
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from floodplanet_code_amd import _lib, fit
from floodplanet_code_amd.models import build_model

sys.path.insert(0, os.path.dirname(__file__))
from tools import focal_ref as R  # noqa: E402

HEADER = os.path.join(ROOT, "include", "floodunet.h")
WEIGHTS = [2.5, 0.7, 1.3, 0.25, 3.0, 0.5]


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_the_entry_point_and_lib_binds_it():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(fu_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}
    assert int(re.search(r"#define\s+FU_ABI_VERSION\s+(\d+)", txt).group(1)) == 5      # additive: no version bump
    assert "fu_loss_ce_focal" in decl, "fu_loss_ce_focal is not declared in floodunet.h"
    args = [a.strip() for a in decl["fu_loss_ce_focal"].split(",")]
    assert len(args) == 10, args
    assert args[4] == "float focal_gamma"
    assert "fu_loss_ce_focal" in _lib.SIGNATURES, "fu_loss_ce_focal has no ctypes row in _lib.SIGNATURES"
    res, sig = _lib.SIGNATURES["fu_loss_ce_focal"]
    assert res is _lib._i and len(sig) == 10
    assert sig[4] is _lib._f                                    # focal_gamma travels as a C float
    assert sig == _lib.SIGNATURES["fu_loss_ce_weighted"][1]     # the weighted call's layout, gamma where eps was


# ------------------------------------------------------------------------------------------------ the specification
def _case(C, seed, B=2, H=9, W=11, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * scale)
    t = torch.randint(0, C, (B, H, W), generator=g)
    return z, t


@pytest.mark.parametrize("C", [2, 3, 6])
def test_reference_at_gamma_zero_is_torchs_weighted_cross_entropy(C):
    z, t = _case(C, seed=C)
    for ii in (0, C - 1, -100):
        for w in (None, WEIGHTS[:C]):
            w64 = None if w is None else torch.tensor(w, dtype=torch.float32).double()
            want = F.cross_entropy(z, t, weight=w64, ignore_index=ii)
            got = R.focal_loss(z, t, 0.0, w, ii)
            assert abs(got.item() - want.item()) <= 1e-12, (C, ii, w)
    assert R.focal_loss(z, torch.full_like(t, 1), 2.0, None, 1).item() == 0.0       # D == 0: loss 0, not torch's NaN


@pytest.mark.parametrize("C", [2, 3, 6])
def test_reference_autograd_gradient_equals_the_closed_form(C):
    worst = 0.0
    for gamma in (0.0, 0.5, 1.0, 2.0, 5.0):
        for ii, w in ((0, WEIGHTS[:C]), (-100, None)):
            for scale in (1.0, 8.0):
                z, t = _case(C, seed=10 + C, scale=scale)
                z.requires_grad_(True)
                R.focal_loss(z, t, gamma, w, ii).backward()
                want = R.focal_dlogits_closed_form(z, t, gamma, w, ii)
                d = (z.grad - want).abs().max().item()
                worst = max(worst, d)
                assert d <= 1e-12, (C, gamma, ii, scale, d)
                assert bool(want.abs().sum() > 0)
    print("worst |autograd - closed form| =", worst)


def test_reference_three_pixels_by_hand():
    """Two classes, z = (0, log 3) -> p = (1/4, 3/4).  Pixel 0: t = 1 (q = 3/4, u = 1/4); pixel 1: t = 0 (q = 1/4, u = 3/4);
    pixel 2 ignored.  w = (2, 1), gamma = 2:  loss = [1 * (1/4)^2 * log(4/3) + 2 * (3/4)^2 * log 4] / (1 + 2)."""
    z = torch.tensor([0.0, math.log(3.0)], dtype=torch.float64).view(1, 2, 1, 1).repeat(1, 1, 1, 3).clone()
    t = torch.tensor([[[1, 0, 7]]])
    want = (1 * (1 / 16) * math.log(4 / 3) + 2 * (9 / 16) * math.log(4)) / 3
    got = R.focal_loss(z, t, 2.0, [2.0, 1.0], 7)
    assert abs(got.item() - want) <= 1e-15
    # pixel 0: m = u^2 - 2 q u log q = 1/16 + (3/8) log(4/3);  dz = w (p - onehot) m / D
    m0 = 1 / 16 + (3 / 8) * math.log(4 / 3)
    m1 = 9 / 16 + 2 * (1 / 4) * (3 / 4) * math.log(4)
    g = R.focal_dlogits_closed_form(z, t, 2.0, [2.0, 1.0], 7)[0, :, 0, :]
    assert torch.allclose(g[:, 0], torch.tensor([0.25, -0.25], dtype=torch.float64) * m0 / 3, rtol=0, atol=1e-15)
    assert torch.allclose(g[:, 1], torch.tensor([-0.75, 0.75], dtype=torch.float64) * 2 * m1 / 3, rtol=0, atol=1e-15)
    assert not bool(g[:, 2].any())


# ------------------------------------------------------------------------------------------------ model constructor
@pytest.mark.parametrize("name", ["ms_model", "ef_model", "lf_model"])
def test_model_ctor_keeps_focal_gamma(name):
    m = build_model(name, {"ms_image": 2}, 3, 1e-3, 50, None, ignore_index=0, base_channels=8, focal_gamma=2.0,
                    class_weights=[0.0, 0.5, 2.0])
    assert m.focal_gamma == 2.0 and type(m.focal_gamma) is float
    assert isinstance(m.loss_func, torch.nn.CrossEntropyLoss)                # kept for API parity
    assert torch.equal(m.loss_func.weight, torch.tensor([0.0, 0.5, 2.0]))
    assert build_model(name, {"ms_image": 2}, 3, 1e-3, 50, None, ignore_index=0, base_channels=8).focal_gamma == 0.0
    m.set_loss_options([1, 2, 3], 0.0, 0.5)
    assert m.focal_gamma == 0.5 and m.class_weights == (1.0, 2.0, 3.0)
    m.set_loss_options([1, 2, 3], 0.25)                                     # the two-argument call: gamma back at 0
    assert m.focal_gamma == 0.0 and m.label_smoothing == 0.25
    with pytest.raises(ValueError):
        m.set_loss_options(None, 0.1, 2.0)


@pytest.mark.parametrize("bad", [dict(focal_gamma=-1), dict(focal_gamma=float("nan")), dict(focal_gamma=float("inf")),
                                 dict(focal_gamma=2, label_smoothing=0.1)])
@pytest.mark.parametrize("name", ["ms_model", "ef_model", "lf_model"])
def test_model_ctor_rejects_bad_focal_options(name, bad, monkeypatch):
    # before any GPU use: the library must not even be loaded for the check
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the GPU library was touched")))
    with pytest.raises(ValueError):
        build_model(name, {"ms_image": 2}, 3, 1e-3, 50, None, ignore_index=0, base_channels=8, **bad)


def test_hipunet_checks_focal_gamma_on_the_host(monkeypatch):
    from floodplanet_code_amd.unet import HipUNet, check_focal_gamma
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the GPU library was touched")))
    net = HipUNet(2, 3, base_channels=8)
    t = torch.zeros(1, 16, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match="kind='ce'"):
        net._loss_raw(t, 0, torch.device("cpu"), kind="bce_dice", focal_gamma=2)
    for kw in (dict(focal_gamma=-1), dict(focal_gamma=float("nan")), dict(focal_gamma=float("inf")),
               dict(focal_gamma=2, label_smoothing=0.1)):
        with pytest.raises(ValueError, match="focal_gamma"):
            net._loss_raw(t, 0, torch.device("cpu"), **kw)
    assert check_focal_gamma(0) == 0.0 and check_focal_gamma(2) == 2.0 and check_focal_gamma(0, 0.1) == 0.0
    assert type(check_focal_gamma(2)) is float


def test_trainer_checks_focal_gamma_on_the_host(monkeypatch):
    from floodplanet_code_amd.distributed import DataParallelTrainer
    from floodplanet_code_amd.unet import HipUNet
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the GPU library was touched")))
    net = HipUNet(2, 3, base_channels=8)
    assert DataParallelTrainer(net, lr=1e-3, focal_gamma=2).focal_gamma == 2.0
    for kw in (dict(focal_gamma=-1), dict(focal_gamma=float("nan")), dict(focal_gamma=2, label_smoothing=0.1)):
        with pytest.raises(ValueError):
            DataParallelTrainer(net, lr=1e-3, **kw)


# ------------------------------------------------------------------------------------------------ command line
def _args(*extra):
    return fit.build_parser().parse_args(["/data", "--exp_dir", "/exp", *extra])


def test_fit_command_line_parses_focal_gamma():
    kw = fit.cfg_from_args(_args("--focal_gamma", "2"))["model"]["model_kwargs"]
    assert kw["focal_gamma"] == 2.0 and type(kw["focal_gamma"]) is float
    assert "label_smoothing" not in kw and "class_weights" not in kw
    kw = fit.cfg_from_args(_args("--focal_gamma", "0.5", "--class_weights", "0", "1", "2.5"))["model"]["model_kwargs"]
    assert kw["focal_gamma"] == 0.5 and kw["class_weights"] == [0.0, 1.0, 2.5]
    for extra in ((), ("--focal_gamma", "0")):                               # absent: the config the command line always gave
        plain = fit.cfg_from_args(_args(*extra))
        assert plain["model"]["model_kwargs"] == dict(optimizer_name="adam", base_channels=64, precision="fp32")


def test_fit_command_line_rejects_bad_focal_options(capsys):
    for extra in (("--focal_gamma", "2", "--label_smoothing", "0.1"), ("--focal_gamma", "-1"), ("--focal_gamma", "nan"),
                  ("--focal_gamma", "inf")):
        with pytest.raises(ValueError):
            fit.cfg_from_args(_args(*extra))
        with pytest.raises(SystemExit):                                      # a usage error, before any data is read
            fit.main(["/nonexistent", "--exp_dir", "/nonexistent", *extra])
    capsys.readouterr()
