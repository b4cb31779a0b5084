"""CPU: the specification the op-level loss tests compare against (tests/tools/loss_ref.py) is what it claims to be.

  * its closed forms equal fp64 autograd of torch.nn.functional.cross_entropy (weight, ignore_index, label_smoothing), of
    tools/focal_ref.focal_loss and of oracle.bce_dice_loss to 1e-12 relative, its confusion matrix is torch.argmax's;
  * the NumPy float32 restatement of the same formulas stays within 1/4 of grad_bound on every element of every input set of
    tests/test_gpu_loss_ops.py -- that is how K was chosen (the measured figures are printed and recorded in loss_ref.py);
  * the comparator sees what it must: one element off by twice its bound, one pixel's row zeroed, and the
    log(sum_{k != 1} exp(z_k - max_all)) form of log(1 - p) that fu_loss_bce_dice had."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_oracle as O

sys.path.insert(0, os.path.dirname(__file__))
from tools import focal_ref  # noqa: E402
from tools import loss_ref as L  # noqa: E402

CLASSES = [1, 2, 3, 4, 5, 8]


def _ignore_values(C):
    return [0, C - 1, -100] if C > 1 else [0, -100]


def _torch_layout(z, t, requires_grad=True):
    P, C = z.shape
    zz = torch.from_numpy(np.ascontiguousarray(z.T)).double().reshape(1, C, P, 1).requires_grad_(requires_grad)
    return zz, torch.from_numpy(t).reshape(1, P, 1)


def _autograd(form, z, t, ii, kw):
    """fp64 loss and dL/dz [P, C] of the torch / oracle definition; the out-of-range targets are sent to the ignore value first
    (torch rejects them; the kernels and the specification drop them)."""
    P, C = z.shape
    zz, tt = _torch_layout(z, np.where(L.valid_mask(t, ii, C), t, ii))
    if form in ("ce", "weighted"):
        w = torch.tensor(kw["weight"], dtype=torch.float32).double() if kw.get("weight") is not None else None
        loss = F.cross_entropy(zz, tt, weight=w, ignore_index=ii, label_smoothing=kw.get("eps", 0.0))
        if not bool(torch.isfinite(loss)):                                  # torch: 0/0 -> NaN; the project: 0
            return 0.0, np.zeros((P, C))
    elif form == "focal":
        loss = focal_ref.focal_loss(zz, tt, kw["gamma"], kw["weight"], ii)
    else:
        loss = O.bce_dice_loss(zz, tt, ii, kw["dice_weight"])
    loss.backward()
    return loss.item(), zz.grad.reshape(C, P).numpy().T


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("C", CLASSES)
def test_closed_forms_equal_fp64_autograd(C):
    for ii in _ignore_values(C):
        z, t = L.constructed_inputs(C, ii)
        for label, form, kw in L.form_cases(C):
            kw = L.form_kwargs(form, kw, C, ii)
            ref = L.reference(form, z, t, ii, **kw)
            loss, grad = _autograd(form, z, t, ii, kw)
            d_loss = abs(ref["loss"] - loss) / max(1.0, abs(loss))
            d_grad = _rel(ref["grad"], grad) if np.abs(grad).max() > 0 else float(np.abs(ref["grad"]).max())
            print(f"C={C} ii={ii} {label}: loss {ref['loss']:.12f} |d| {d_loss:.1e}, gradient rel {d_grad:.1e}")
            assert d_loss <= 1e-12 and d_grad <= 1e-12, (C, ii, label, d_loss, d_grad)
            v = L.valid_mask(t, ii, C)
            assert ref["n_valid"] == int(v.sum()) == int(ref["confusion"].sum())
            assert not ref["grad"][~v].any()
            if form == "focal":                 # the float32 restatement's formulas, in fp64, are focal_ref's as well
                lf, gf = L._focal(z, t, ii, kw["gamma"], kw["weight"], np.float64)[:2]
                assert abs(lf - loss) <= 1e-12 * max(1.0, abs(loss)) and _rel(gf, grad) <= 1e-12


@pytest.mark.parametrize("C", CLASSES)
def test_counts_follow_torch_argmax_and_the_zero_denominator_rule(C):
    for ii in _ignore_values(C):
        z, t = L.constructed_inputs(C, ii)
        v = L.valid_mask(t, ii, C)
        am = torch.argmax(torch.from_numpy(z), dim=1).numpy()               # the first maximal index on the CPU
        want = np.zeros((C, C), np.int64)
        np.add.at(want, (t[v], am[v]), 1)
        assert np.array_equal(L.confusion(z, t, ii), want)
        census = L.planted_census(z, t, ii)
        for kind in L.expected_kinds(C, ii):
            assert census[kind] >= 2, (C, ii, kind, census)
        for bad in (-1, C, 255, ii):
            assert census[("target", bad)] >= 8 and not v[t == bad].any()
        # N == 0 (every target ignored) and D == 0 (only zero-weight classes present): loss 0, gradient 0
        dead = np.full_like(t, ii)
        for label, form, kw in L.form_cases(C):
            ref = L.reference(form, z, dead, ii, **L.form_kwargs(form, kw, C, ii))
            assert ref["loss"] == 0.0 and ref["n_valid"] == 0 and not ref["grad"].any(), label
            assert not L.grad_bound(form, z, dead, ii, 1, **L.form_kwargs(form, kw, C, ii)).any()
        if C >= 2 and ii != 0:
            only0 = np.zeros_like(t)
            w = [0.0] + [1.0] * (C - 1)
            for form, kw in (("weighted", {"eps": 0.0}), ("focal", {"gamma": 2.0})):
                ref = L.reference(form, z, only0, ii, weight=w, **kw)
                assert ref["loss"] == 0.0 and ref["D"] == 0.0 and ref["n_valid"] == t.size and not ref["grad"].any()


def _restatement_ratio(form, z, t, ii, trips, kw):
    """(worst ratio at K, at K / 2, float32 loss, fp64 loss)"""
    ref = L.reference(form, z, t, ii, **kw)
    loss32, g32 = L.restate_f32(form, z, t, ii, **kw)
    a, r = L.grad_bound_parts(form, z, t, ii, trips, **kw)
    at = [L.worst_ratio(g32, ref["grad"], L.EPS32 * (k * a + r)) for k in (L.K, L.K / 2)]
    return at[0], at[1], loss32, ref["loss"]


MEASURED = {}


@pytest.mark.parametrize("C", CLASSES)
def test_float32_restatement_stays_within_a_quarter_of_the_bound_constructed(C):
    P = np.prod(L.SHAPE_A)
    for ii in _ignore_values(C):
        z, t = L.constructed_inputs(C, ii)
        for label, form, kw in L.form_cases(C):
            kw = L.form_kwargs(form, kw, C, ii)
            trips = L.sum_trips(P, L.BD_LOSS_CAP if form == "bce_dice" else L.CE_LOSS_CAP)
            ratio, half, loss32, loss64 = _restatement_ratio(form, z, t, ii, trips, kw)
            MEASURED[form] = max(MEASURED.get(form, (0.0, 0.0)), (ratio, half))
            print(f"C={C} ii={ii} {label}: ratio at K={L.K:g} {ratio:.3f}, at K/2 {half:.3f}; loss {loss32!r} vs {loss64!r}")
            assert ratio <= 0.25, (C, ii, label, ratio)
            assert L.loss_ok(loss32, loss64), (C, ii, label, loss32, loss64)
    print("worst (ratio at K, at K/2) so far:", MEASURED)


@pytest.mark.parametrize("label,form,kw", L.BIG_FORMS, ids=[c[0] for c in L.BIG_FORMS])
def test_float32_restatement_stays_within_a_quarter_of_the_bound_big(label, form, kw):
    for batch, valid_from in L.big_layouts(form):
        z, t = L.big_case(batch, valid_from)
        trips = L.sum_trips(t.size, L.BD_LOSS_CAP if form == "bce_dice" else L.CE_LOSS_CAP)
        ratio, half, loss32, loss64 = _restatement_ratio(form, z, t, -100, trips, kw)
        print(f"{label} batch {batch} valid from {valid_from}: ratio at K={L.K:g} {ratio:.3f}, at K/2 {half:.3f}; "
              f"loss {loss32!r} vs {loss64!r}")
        assert ratio <= 0.25, (label, batch, valid_from, ratio)
        assert L.loss_ok(loss32, loss64)
        assert int(L.valid_mask(t, -100, 3).sum()) == t.size - valid_from > 0


def test_recorded_k_is_the_smallest_power_of_two_for_the_recorded_ratios():
    assert max(L.MEASURED[L.K].values()) <= 0.25 < max(L.MEASURED[L.K / 2].values())


def test_comparator_flags_one_element_off_by_twice_its_bound_and_one_zeroed_row():
    z, t = L.big_case(3, 0)
    assert t.size == 1051392
    kw = dict(L.BIG_FORMS[1][2])
    ref = L.reference("weighted", z, t, -100, **kw)
    bound = L.grad_bound("weighted", z, t, -100, L.sum_trips(t.size, L.CE_LOSS_CAP), **kw)
    assert L.worst_ratio(ref["grad"], ref["grad"], bound) == 0.0
    moved = ref["grad"].copy()
    moved[777777, 1] += 2.0 * bound[777777, 1]
    assert 1.9 <= L.worst_ratio(moved, ref["grad"], bound) <= 2.1
    pixel = int(np.flatnonzero(L.valid_mask(t, -100, 3) & (t != 0))[-1])     # a valid pixel of a weighted class, in the last trip
    zeroed = ref["grad"].copy()
    zeroed[pixel] = 0.0
    assert L.worst_ratio(zeroed, ref["grad"], bound) > 1e3
    wrong_zero = ref["grad"].copy()                                          # an invalid pixel's gradient must be exactly 0
    t2 = t.copy()
    t2[5] = -100
    wrong_zero[5, 0] = 1e-30
    b2 = L.grad_bound("weighted", z, t2, -100, 5, **kw)
    assert L.worst_ratio(wrong_zero, L.reference("weighted", z, t2, -100, **kw)["grad"], b2) == float("inf")


@pytest.mark.parametrize("C", [2, 3])
def test_single_maximum_form_of_log1mp_fails_on_the_saturated_input(C):
    """log(1 - p) as log(sum_{k != 1} exp(z_k - m)) - log(sum_k exp(z_k - m)) with m over ALL classes, in float32: denormal
    exponentials from a margin of 88 on, zeros from 104 on -- the loss is inf and the gradient rows lose their s1."""
    z, t = L.constructed_inputs(C, -100)
    kw = {"dice_weight": 0.7}
    ref = L.reference("bce_dice", z, t, -100, **kw)
    bound = L.grad_bound("bce_dice", z, t, -100, 1, **kw)
    loss_ok, g_ok = L.restate_f32("bce_dice", z, t, -100, **kw)
    assert L.loss_ok(loss_ok, ref["loss"]) and L.worst_ratio(g_ok, ref["grad"], bound) <= 0.25
    loss_bad, g_bad = L.restate_f32("bce_dice", z, t, -100, naive_log1mp=True, **kw)
    ratio = L.worst_ratio(g_bad, ref["grad"], bound)
    print(f"C={C}: spec {ref['loss']!r}, stable float32 {loss_ok!r}, single-maximum float32 {loss_bad!r}, gradient ratio {ratio:.3g}")
    assert not L.loss_ok(loss_bad, ref["loss"])
    assert ratio > 1.0
    # ... and only there: without the pixels where class 1 leads every other class by 80 or more the two forms agree
    lead = z[:, 1].astype(np.float64) - np.delete(z, 1, axis=1).max(axis=1)
    t_mild = np.where(lead >= 80.0, -100, t)
    ref = L.reference("bce_dice", z, t_mild, -100, **kw)
    loss_bad, g_bad = L.restate_f32("bce_dice", z, t_mild, -100, naive_log1mp=True, **kw)
    assert L.loss_ok(loss_bad, ref["loss"])
    assert L.worst_ratio(g_bad, ref["grad"], L.grad_bound("bce_dice", z, t_mild, -100, 1, **kw)) <= 1.0
