"""CPU: tests/tools/head_ref.py on its own -- the launch geometry it restates, the operand generator's promises at every shape
the GPU tests use, and the analytic bounds against a float32 restatement of the kernels' arithmetic (ratio <= 1 everywhere:
a violated bound would be a wrong derivation, never a reason to scale it)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from tools import head_ref as R   # noqa: E402

PRECS = list(R.PREC)


def test_geometry_restates_the_launch_code():
    # the forward's main shape: one block, two trips at one lane per pixel; 14 blocks at 16 lanes per pixel
    HW = R.FWD_MAIN[1] * R.FWD_MAIN[2]
    g1, g16 = R.fwd_geometry("fp32", 4, HW), R.fwd_geometry("fp32", 64, HW)
    assert (g1["ppb"], g1["grid"], g1["trips"]) == (256, 1, 2) and HW % 1024 != 0
    assert (g16["ppb"], g16["grid"]) == (16, 14) and HW % 64 != 0
    assert R.fwd_geometry("bf16", 128, HW)["n"] == 8 + 4 + 1 and R.fwd_geometry("fp32", 4, HW)["n"] == 4 + 0 + 1
    # the backward: below the cap one trip; at the cap every block makes a second, ragged trip
    for prec, C in (("fp32", 64), ("bf16", 128), ("fp16", 128)):
        g = R.bwd_geometry(prec, C, R.CAP_NPIX)
        assert (g["ppb"], g["nblk"], g["trips"], g["n"]) == (16, 2048, 2, 8 + 16)
        assert 2048 * 64 < R.CAP_NPIX and R.CAP_NPIX % 64 != 0             # a second trip, and a ragged one
    assert R.bwd_geometry("fp32", 4, 4099) == dict(lpp=1, ppb=256, nblk=5, trips=1, T=4, n=260)
    assert [R.widths(p) for p in PRECS] == [[4, 8, 16, 32, 64], [8, 16, 32, 64, 128], [8, 16, 32, 64, 128]]
    # the dynamic-LDS request of the block reduction: one pass of all classes fits 64 KiB except 16-bit with 8 classes
    for prec in PRECS:
        for C in R.widths(prec):
            ppb = R.bwd_geometry(prec, C, 4099)["ppb"]
            for k in range(1, 9):
                assert (ppb * (k * C + k) * 4 > 65536) == (prec != "fp32" and k == 8)
                assert ppb * (4 * C + 4) * 4 <= 65536


@pytest.mark.parametrize("prec", PRECS)
def test_generator_leaves_no_ambiguous_mask_and_plants_what_it_says(prec):
    HW = R.FWD_MAIN[1] * R.FWD_MAIN[2]
    shapes = {R.FWD_MAIN[0] * HW} | {b * h * w for b, h, w in R.FWD_SMALL} | set(R.BWD_NPIX)
    n_zero = n_dead = 0
    for C in R.widths(prec):
        for npix in sorted(shapes):
            ops = R.make_operands(prec, C, npix)
            R.check_plants(ops)
            n_zero += len(ops["zero_pre"])
            n_dead += len(ops["dead"])
    assert n_zero > 100 and n_dead > 100
    for C in (R.widths(prec)[0], R.widths(prec)[-1]):          # the grid-cap and coverage cases
        R.check_plants(R.make_operands(prec, C, R.CAP_NPIX))


def _forms(prec):
    return ((True, prec != "fp32"), (False, False))     # (BatchNorm prologue, fused sums); the fp32 kernel emits no sums


def _bwd_ratios(prec, ops, bn, sums):
    a, b = (ops["a"], ops["b"]) if bn else (None, None)
    mean, invstd = (ops["mean"], ops["invstd"]) if sums else (None, None)
    ref = R.bwd_ref(prec, ops["dl"], ops["y"], a, b, ops["w"], mean, invstd)
    got = R.restate_bwd(prec, ops["dl"], ops["y"], a, b, ops["w"], mean, invstd)
    return {k: R.worst_ratio(got[k], *ref[k]) for k in ref}


def _fwd_ratio(prec, ops, bn):
    a, b = (ops["a"], ops["b"]) if bn else (None, None)
    ref, bound = R.fwd_ref(prec, ops["y"], a, b, ops["w"], ops["bias"])
    return {"logits": R.worst_ratio(R.restate_fwd(prec, ops["y"], a, b, ops["w"], ops["bias"]), ref, bound)}


@pytest.mark.parametrize("prec", PRECS)
def test_float32_restatement_stays_within_every_bound(prec):
    worst = {}

    def take(ratios, case):
        for name, r in ratios.items():
            assert r <= 1.0, (case, name, r)
            worst[name] = max(worst.get(name, 0.0), r)
    HW = R.FWD_MAIN[1] * R.FWD_MAIN[2]
    fwd_npix = (R.FWD_MAIN[0] * HW,) + tuple(b * h * w for b, h, w in R.FWD_SMALL)
    for C in R.widths(prec):
        for k in R.CLASSES:
            for bn, sums in _forms(prec):
                for npix in fwd_npix:
                    take(_fwd_ratio(prec, R.take(R.make_operands(prec, C, npix), k), bn), (C, npix, k, bn))
                for npix in R.BWD_NPIX:
                    take(_bwd_ratios(prec, R.take(R.make_operands(prec, C, npix), k), bn, sums), (C, npix, k, bn))
    for k in (3, 8):                                    # the capped grid: two trips per thread
        C = R.widths(prec)[-1]
        take(_bwd_ratios(prec, R.take(R.make_operands(prec, C, R.CAP_NPIX), k), True, prec != "fp32"), (C, R.CAP_NPIX, k))
    print(f"MEASURED restatement {prec}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert set(worst) == set(R.MEASURED_RESTATEMENT[prec]) and all(v > 0.0 for v in worst.values())
    for k, v in R.MEASURED_RESTATEMENT[prec].items():
        assert abs(worst[k] - v) <= 2e-3, (k, worst[k], v)      # the table in head_ref.py is this run's


def test_a_dropped_pixel_or_a_wrong_mask_breaks_the_bounds():
    """The bounds are tight enough to see one lost term: without its last pixel, or with >= 0 for the strict mask in the
    second sum (planted exact zeros contribute g * xhat there), the restatement leaves them."""
    prec = "bf16"
    ops = R.take(R.make_operands(prec, 64, 1665), 3)
    ref = R.bwd_ref(prec, ops["dl"], ops["y"], ops["a"], ops["b"], ops["w"], ops["mean"], ops["invstd"])
    cut = R.restate_bwd(prec, ops["dl"][:-1], ops["y"][:-1], ops["a"], ops["b"], ops["w"], ops["mean"], ops["invstd"])
    assert R.worst_ratio(cut["db"], *ref["db"]) > 1.0 and R.worst_ratio(cut["dw"], *ref["dw"]) > 1.0
    y64 = ops["y"].astype(np.float64)
    pre = ops["a"].astype(np.float64) * y64 + ops["b"]
    g = ops["dl"].astype(np.float64) @ ops["w"]
    xh = (y64 - ops["mean"]) * ops["invstd"]
    s1_ge, s2_ge = (g * (pre >= 0)).sum(0), (g * (pre >= 0) * xh).sum(0)
    assert R.worst_ratio(s1_ge, *ref["s1"]) > 1.0 and R.worst_ratio(s2_ge, *ref["s2"]) > 1.0
