"""CPU: the host side of the region term (fu_loss_ce_region) -- the fp64 specification (tests/tools/region_ref.py) against
fp64 autograd of the definition, against the Dice ratio of BCE + Dice and at the all-ignored batch; the float32 restatement
against the bound the GPU tests use, with two comparator controls; the C ABI declarations; the host-side option checks of
HipUNet, the models and the trainer; the fit command line.  No GPU.

Worst ratio of the float32 restatement against region_ref.grad_bound (K = 16), printed by
test_float32_restatement_stays_within_a_quarter_of_the_bound:

    inputs                                       plain CE   weighted / smoothed CE   focal
    constructed (C in 2, 3, 4, 5, 8; 3 ignores)  0.029      0.064                    0.062
    big_case layouts (C = 3)                     0.020      0.027                    --

The controls on the (0.3, 0.7) case: alpha and beta swapped in the coefficients, and the sign of B_k flipped, both miss the
bound by orders of magnitude (ratios above 1e3)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from floodplanet_code_amd import _lib, fit
from floodplanet_code_amd.models import build_model

sys.path.insert(0, os.path.dirname(__file__))
from tools import loss_ref as L  # noqa: E402
from tools import region_ref as R  # noqa: E402

HEADER = os.path.join(ROOT, "include", "floodunet.h")
CLASSES = [2, 3, 4, 5, 8]
LAM = 0.7
CE_FORMS = [("ce", {}), ("weighted", {"eps": 0.1}), ("focal", {"gamma": 2.0})]


def _ignores(C):
    return [0, C - 1, -100]


# ------------------------------------------------------------------------------------------------ the specification
def _autograd(z32, t, ii, lam, alpha, beta, s):
    """lambda R and its gradient by fp64 autograd of the definition"""
    z = torch.from_numpy(z32).double().requires_grad_(True)
    C = z.shape[1]
    v = torch.from_numpy(L.valid_mask(t, ii, C))
    tt = torch.from_numpy(np.where(v.numpy(), t, 0))
    pv = torch.softmax(z, 1) * v[:, None]
    y = torch.nn.functional.one_hot(tt, C).double() * v[:, None]
    I, P, T = (pv * y).sum(0), pv.sum(0), y.sum(0)
    TI = (I + s) / (I + alpha * (P - I) + beta * (T - I) + s)
    inc = torch.from_numpy(R.included(C, ii))
    Rv = ((1 - TI) * inc).sum() / inc.sum()
    (lam * Rv).backward()
    return float(lam * Rv.detach()), z.grad.numpy(), TI.detach().numpy()


@pytest.mark.parametrize("C", CLASSES)
def test_closed_form_equals_fp64_autograd_of_the_definition(C):
    worst = 0.0
    for ii in _ignores(C):
        z, t = L.constructed_inputs(C, ii)
        for alpha, beta, s in R.PARAM_SETS + [(0.0, 1.0, 1.0), (1.0, 0.0, 1.0)]:
            want_l, want_g, want_ti = _autograd(z, t, ii, LAM, alpha, beta, s)
            for form, kw in CE_FORMS:
                kw = L.form_kwargs(form, kw, C, ii)
                ce = L.reference(form, z, t, ii, **kw)
                got = R.reference(form, z, t, ii, LAM, alpha, beta, s, **kw)
                dl = abs((got["loss"] - ce["loss"]) - want_l)
                dg = np.abs((got["grad"] - ce["grad"]) - want_g).max()
                worst = max(worst, dl, dg)
                assert dl <= 1e-12 and dg <= 1e-12, (C, ii, alpha, beta, s, form, dl, dg)
                assert abs(got["R"] * LAM - want_l) <= 1e-12
                inc = R.included(C, ii)
                assert np.abs(got["TI"][inc] - want_ti[inc]).max() <= 1e-12 and (got["TI"][~inc] == 1.0).all()
                assert got["n_valid"] == ce["n_valid"] and np.array_equal(got["confusion"], ce["confusion"])
            assert beta == 0.0 or np.abs(want_g).max() > 0    # (beta = 0, one live class: no false positive exists)
    print(f"C={C}: worst |closed form - autograd| = {worst:.2e}")


@pytest.mark.parametrize("C", CLASSES)
def test_dice_index_of_class_1_is_the_dice_ratio_of_bce_dice(C):
    """TI_1 at (0.5, 0.5, 0.5) = (2 I + 1) / (P + T + 1), the Nn / Dd of loss_ref._bce_dice: 1 - loss + bce with dice_weight 1"""
    for ii in (0, -100):
        z, t = L.constructed_inputs(C, ii)
        ti = R.reference("ce", z, t, ii, LAM, 0.5, 0.5, 0.5)["TI"][1]
        dice = L._bce_dice(z, t, ii, 1.0, np.float64)[0] - L._bce_dice(z, t, ii, 0.0, np.float64)[0]     # 1 - Nn / Dd
        assert abs((1.0 - ti) - dice) <= 1e-12, (C, ii, ti, dice)


def test_all_ignored_batch_gives_exactly_zero():
    z, t = L.constructed_inputs(3, -100)
    for dt_restate in (False, True):
        for alpha, beta, s in R.PARAM_SETS:
            t2 = np.full_like(t, 2)
            if dt_restate:
                loss, g = R.restate_f32("ce", z, t2, 2, LAM, alpha, beta, s)
            else:
                ref = R.reference("ce", z, t2, 2, LAM, alpha, beta, s)
                loss, g = ref["loss"], ref["grad"]
                assert ref["R"] == 0.0 and (ref["TI"] == 1.0).all()
            assert loss == 0.0 and not g.any()


def test_region_term_follows_pixel_validity_not_the_summed_weight():
    """valid pixels whose classes all carry weight 0: CE 0 (D == 0), the region term and its gradient alive"""
    z, t = L.constructed_inputs(3, -100)
    t = np.where(L.valid_mask(t, -100, 3), t % 2 + 1, t)
    ref = R.reference("weighted", z, t, -100, LAM, 0.5, 0.5, 1.0, weight=[3.0, 0.0, 0.0])
    assert ref["D"] == 0.0 and ref["ce_loss"] == 0.0 and ref["n_valid"] > 0
    assert ref["loss"] == LAM * ref["R"] > 0 and np.abs(ref["grad"]).max() > 0


# ------------------------------------------------------------------------------------------------ the bound
def _ratio(form, z, t, ii, params, kw, **control):
    alpha, beta, s = params
    ref = R.reference(form, z, t, ii, LAM, alpha, beta, s, **kw)
    loss, g = R.restate_f32(form, z, t, ii, LAM, alpha, beta, s, **control, **kw)
    bound = R.grad_bound(form, z, t, ii, LAM, alpha, beta, s, spec=ref["grad"], **kw)
    if not control:
        assert L.loss_ok(loss, ref["loss"]), (form, ii, params, loss, ref["loss"])
    return L.worst_ratio(g, ref["grad"], bound)


def test_float32_restatement_stays_within_a_quarter_of_the_bound():
    worst = {}
    for C in CLASSES:
        for ii in _ignores(C):
            z, t = L.constructed_inputs(C, ii)
            for params in R.PARAM_SETS:
                for form, kw in CE_FORMS:
                    r = _ratio(form, z, t, ii, params, L.form_kwargs(form, kw, C, ii))
                    worst[("constructed", form)] = max(worst.get(("constructed", form), 0.0), r)
    lay = R.big_layouts()                                                    # every layout once, the forms and parameter sets in turn
    for n, (batch, valid_from) in enumerate(lay):
        z, t = L.big_case(batch, valid_from)
        form, kw = (("ce", {}), ("weighted", {"eps": 0.1, "weight": [0.0, 0.7, 1.3]}))[n % 2]
        r = _ratio(form, z, t, -100, R.PARAM_SETS[2 if n in (0, 1) else 0], kw)
        worst[("big", form)] = max(worst.get(("big", form), 0.0), r)
    for key, r in sorted(worst.items()):
        print(f"{key[0]:12s} {key[1]:9s} worst restatement / bound = {r:.3f} (recorded {R.MEASURED[key[0]][key[1]]})")
    for key, r in worst.items():
        assert r <= 0.25, (key, r)
        assert r <= 1.25 * R.MEASURED[key[0]][key[1]] + 1e-3, (key, r)       # the recorded table is the measured one


@pytest.mark.parametrize("control", [{"swap": True}, {"flip_b": True}])
def test_comparator_controls_fail_the_bound(control):
    """the inputs can tell alpha from beta, and the sign of B_k: a restatement that gets either wrong misses the bound"""
    for C in (2, 3, 8):
        for ii in (0, -100):
            if "flip_b" in control and C == 2 and ii != -100:
                continue                         # one live class, every valid pixel its own: B_k reaches no element
            z, t = L.constructed_inputs(C, ii)
            r = _ratio("ce", z, t, ii, (0.3, 0.7, 1.0), {}, **control)
            print(f"C={C} ii={ii} {control}: ratio {r:.3g}")
            assert r > 1.0, (C, ii, control, r)


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_the_entry_point_and_lib_binds_it():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(fu_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}
    assert int(re.search(r"#define\s+FU_ABI_VERSION\s+(\d+)", txt).group(1)) == 5      # additive: no version bump
    assert re.search(r"typedef\s+struct\s+fu_region_loss\s*\{\s*float\s+weight\s*,\s*alpha\s*,\s*beta\s*,\s*smooth\s*;\s*\}"
                     r"\s*fu_region_loss\s*;", txt)
    assert "fu_loss_ce_region" in decl, "fu_loss_ce_region is not declared in floodunet.h"
    args = [a.strip() for a in decl["fu_loss_ce_region"].split(",")]
    assert len(args) == 13, args
    assert args[4] == "float label_smoothing" and args[5] == "float focal_gamma"
    assert args[6] == "const fu_region_loss* region" and args[11] == "float* region_out"
    res, sig = _lib.SIGNATURES["fu_loss_ce_region"]
    assert res is _lib._i and len(sig) == 13
    assert sig[4] is _lib._f and sig[5] is _lib._f and sig[6]._type_ is _lib.FuRegionLoss
    assert [f[0] for f in _lib.FuRegionLoss._fields_] == ["weight", "alpha", "beta", "smooth"]
    assert all(f[1] is _lib._f for f in _lib.FuRegionLoss._fields_)


# ------------------------------------------------------------------------------------------------ host-side checks
BAD = [dict(region_weight=-1), dict(region_weight=float("nan")), dict(region_weight=float("inf")),
       dict(region_weight=1, region_alpha=-0.5), dict(region_weight=1, region_alpha=0, region_beta=0),
       dict(region_weight=1, region_beta=float("inf")), dict(region_weight=1, region_smooth=0),
       dict(region_weight=1, region_smooth=float("nan")), dict(region_smooth=-1)]


def _no_gpu(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the GPU library was touched")))


def test_check_region_loss():
    from floodplanet_code_amd.unet import check_region_loss
    assert check_region_loss() == (0.0, 0.5, 0.5, 1.0)
    out = check_region_loss(1, 0, 1, 2)
    assert out == (1.0, 0.0, 1.0, 2.0) and all(type(v) is float for v in out)
    for bad in BAD:
        with pytest.raises(ValueError, match="region_"):
            check_region_loss(*(bad.get(k, d) for k, d in (("region_weight", 0.0), ("region_alpha", 0.5),
                                                            ("region_beta", 0.5), ("region_smooth", 1.0))))


def test_hipunet_checks_the_region_options_on_the_host(monkeypatch):
    from floodplanet_code_amd.unet import HipUNet
    _no_gpu(monkeypatch)
    net = HipUNet(2, 3, base_channels=8)
    t = torch.zeros(1, 16, 16, dtype=torch.int64)
    assert net.last_region_terms() is None
    with pytest.raises(ValueError, match="kind='ce'"):
        net._loss_raw(t, 0, torch.device("cpu"), kind="bce_dice", region_weight=1.0)
    for bad in BAD:
        with pytest.raises(ValueError, match="region_"):
            net._loss_raw(t, 0, torch.device("cpu"), **bad)
    with pytest.raises(ValueError, match="n_classes >= 2"):
        HipUNet(2, 1, base_channels=8)._loss_raw(t, -100, torch.device("cpu"), region_weight=1.0)


@pytest.mark.parametrize("name", ["ms_model", "ef_model", "lf_model"])
def test_model_ctor_keeps_and_checks_the_region_options(name, monkeypatch):
    _no_gpu(monkeypatch)
    kw = dict(ignore_index=0, base_channels=8)
    m = build_model(name, {"ms_image": 2}, 3, 1e-3, 50, None, region_weight=0.5, region_alpha=0.3, region_beta=0.7,
                    region_smooth=2, **kw)
    assert (m.region_weight, m.region_alpha, m.region_beta, m.region_smooth) == (0.5, 0.3, 0.7, 2.0)
    plain = build_model(name, {"ms_image": 2}, 3, 1e-3, 50, None, **kw)
    assert (plain.region_weight, plain.region_alpha, plain.region_beta, plain.region_smooth) == (0.0, 0.5, 0.5, 1.0)
    m.set_loss_options([1, 2, 3], 0.0, 0.5, 2.0, 1.0, 1.0, 0.5)            # trailing keywords, in this order
    assert (m.focal_gamma, m.region_weight, m.region_alpha, m.region_beta, m.region_smooth) == (0.5, 2.0, 1.0, 1.0, 0.5)
    m.set_loss_options([1, 2, 3], 0.25)                                     # the two-argument call: the term back at 0
    assert m.region_weight == 0.0 and m.label_smoothing == 0.25
    for bad in BAD:
        with pytest.raises(ValueError):
            build_model(name, {"ms_image": 2}, 3, 1e-3, 50, None, **kw, **bad)
        with pytest.raises(ValueError):
            m.set_loss_options(None, 0.0, 0.0, **bad)


def test_trainer_checks_the_region_options_on_the_host(monkeypatch):
    from floodplanet_code_amd.distributed import DataParallelTrainer
    from floodplanet_code_amd.unet import HipUNet
    _no_gpu(monkeypatch)
    net = HipUNet(2, 3, base_channels=8)
    tr = DataParallelTrainer(net, lr=1e-3, region_weight=1, region_alpha=1, region_beta=1)
    o = tr.loss_options
    assert (o.region_weight, o.region_alpha, o.region_beta, o.region_smooth) == (1.0, 1.0, 1.0, 1.0)
    assert all(type(v) is float for v in (o.region_weight, o.region_alpha, o.region_beta, o.region_smooth))
    assert DataParallelTrainer(net, lr=1e-3).region_weight == 0.0
    for bad in BAD:
        with pytest.raises(ValueError):
            DataParallelTrainer(net, lr=1e-3, **bad)


# ------------------------------------------------------------------------------------------------ command line
def _args(*extra):
    return fit.build_parser().parse_args(["/data", "--exp_dir", "/exp", *extra])


def _kw(*extra):
    return fit.cfg_from_args(_args(*extra))["model"]["model_kwargs"]


PLAIN = dict(optimizer_name="adam", base_channels=64, precision="fp32")


def test_fit_command_line_parses_the_region_flags():
    assert _kw("--region_loss", "dice") == dict(PLAIN, region_weight=1.0, region_alpha=0.5, region_beta=0.5, region_smooth=1.0)
    assert _kw("--region_loss", "jaccard", "--region_weight", "0.5", "--region_smooth", "0.1") == dict(
        PLAIN, region_weight=0.5, region_alpha=1.0, region_beta=1.0, region_smooth=0.1)
    kw = _kw("--region_loss", "tversky", "--tversky", "0.3", "0.7", "--focal_gamma", "2", "--class_weights", "0", "1", "2")
    assert (kw["region_alpha"], kw["region_beta"], kw["focal_gamma"], kw["class_weights"]) == (0.3, 0.7, 2.0, [0.0, 1.0, 2.0])
    assert all(type(kw[k]) is float for k in ("region_weight", "region_alpha", "region_beta", "region_smooth"))
    assert _kw() == PLAIN                                                    # absent: the config the command line always gave


def test_fit_command_line_rejects_bad_region_flags(capsys):
    for extra in (("--region_weight", "1"), ("--tversky", "0.3", "0.7"), ("--region_smooth", "1"),
                  ("--region_loss", "tversky"), ("--region_loss", "dice", "--tversky", "0.3", "0.7"),
                  ("--region_loss", "dice", "--region_weight", "-1"), ("--region_loss", "dice", "--region_weight", "nan"),
                  ("--region_loss", "dice", "--region_smooth", "0"), ("--region_loss", "tversky", "--tversky", "0", "0"),
                  ("--region_loss", "tversky", "--tversky", "-1", "1")):
        with pytest.raises(ValueError):
            fit.cfg_from_args(_args(*extra))
        with pytest.raises(SystemExit):                                      # a usage error, before any data is read
            fit.main(["/nonexistent", "--exp_dir", "/nonexistent", *extra])
    with pytest.raises(SystemExit):
        _args("--region_loss", "lovasz")
    capsys.readouterr()
