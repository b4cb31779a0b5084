"""CPU: tests/tools/bn_ref.py on its own -- the launch geometry it restates, the analytic bounds against a float32 restatement
of the kernels' arithmetic at every shape the GPU tests use (ratio <= 1 everywhere: a violated bound would be a wrong derivation,
never a reason to scale it), the fp64 reference against fp64 autograd, the exact operands (restatement == reference bit for bit)
and eleven deliberately wrong restatements, each of which must leave the bounds (ratio > 1)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
from tools import bn_ref as R   # noqa: E402

PRECS = list(R.PREC)
f32 = np.float32


class Worst(dict):
    def take(self, outs, refs, case, names=None):
        for name in names or refs:
            r = R.worst_ratio(outs[name], *refs[name])
            self[name] = max(self.get(name, 0.0), r)
            assert r <= 1.0, (case, name, r)

    def report(self, what):
        print(f"MEASURED_RESTATEMENT {what}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(self.items())))


def recorded(worst, key):
    """the figures kept in bn_ref.MEASURED_RESTATEMENT are the ones this run measures (to the third digit)"""
    for name, v in worst.items():
        assert abs(R.MEASURED_RESTATEMENT[key][name] - v) <= 2e-3, (key, name, v)


def test_geometry_restates_the_launch_code():
    assert R.bwd_geometry("plain", 8, 1) == dict(nb=1, rows=128, trips=1, T=1, n=129)
    assert R.bwd_geometry("plain", 12, 35) == dict(nb=1, rows=85, trips=1, T=1, n=86) and 85 * 3 == 255
    assert R.bwd_geometry("plain", 516, 6) == dict(nb=1, rows=1, trips=6, T=6, n=7)
    assert R.bwd_geometry("plain", 1024, 9) == dict(nb=2, rows=1, trips=5, T=5, n=6)
    assert R.bwd_geometry("plain", 64, 3072) == dict(nb=24, rows=16, trips=8, T=8, n=24)
    assert R.bwd_geometry("pool", 64, 3072, 768) == dict(nb=24, rows=16, trips=2, T=8, n=24)
    assert R.bwd_geometry("pool", 32, 1665, 19 * 23) == dict(nb=7, rows=32, trips=2, T=8, n=40) and 19 * 23 % (7 * 32) != 0
    assert R.bwd_geometry("pool", 1024, 16, 4) == dict(nb=2, rows=1, trips=2, T=8, n=9)
    # the head apply pass: 8 channels per lane, so twice the pixel rows of the grid's own estimate
    assert R.bwd_geometry("head", 8, 4099) == dict(nb=5, rows=256, trips=4, T=4, n=260)
    assert R.bwd_geometry("head", 128, 35) == dict(nb=1, rows=16, trips=3, T=3, n=19)
    # 35 and 4099 leave the second in-flight pixel of some head threads past the end: no whole number of pixel pairs per thread
    for C in R.HEAD_WIDTHS:
        for npix in (35, 4099):
            geo = R.bwd_geometry("head", C, npix)
            assert npix % (2 * geo["nb"] * geo["rows"]) != 0


def test_float32_mask_is_torchs_cpu_float32_pre_activation():
    ops = R.dense("fp32", "pool", (1, 32, 37, 45))
    z = R.pre32(ops["y"], ops["a"], ops["b"])
    zt = torch.from_numpy(ops["a"]) * torch.from_numpy(ops["y"]) + torch.from_numpy(ops["b"])
    assert np.array_equal(z, zt.numpy()) and np.array_equal(z > 0, (zt > 0).numpy())


@pytest.mark.parametrize("make", [R.dense, R.exact], ids=["dense", "exact"])
def test_operands_hold_the_decisions_the_kernels_must_take(make):
    """exact-zero pre-activations, windows with two and with four equal positive maxima, all-negative windows"""
    for prec in PRECS:
        for shape in R.POOL_SHAPES[1:]:
            p = R.plants(make(prec, "pool", shape))
            assert p["zero"] > 0 and p["tie4"] > 0, (shape, p)
            assert p["negative"] > 0 or shape[0] * (shape[2] // 2) * (shape[3] // 2) < 5, (shape, p)     # 4 x 4: four windows
            assert p["tie2"] > 0 or shape[2] * shape[3] <= 35, (shape, p)
        for shape in R.PLAIN_SHAPES[1:]:
            assert R.plants(make(prec, "plain", shape))["zero"] > 0, shape


@pytest.mark.parametrize("pooled", [False, True])
def test_reference_equals_fp64_autograd(pooled):
    """relu(batch_norm(y)) consumed by a skip path and by max_pool2d, on operands without ties or near-zero pre-activations"""
    B, C, H, W = 2, 8, 6, 10
    for seed in range(50):
        gen = torch.Generator().manual_seed(seed)
        y = torch.randn(B, C, H, W, generator=gen)
        gam, bet = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
        yd = y.double()
        mean = yd.mean((0, 2, 3))
        invstd = 1.0 / torch.sqrt(yd.var((0, 2, 3), unbiased=False) + 1e-5)
        a = gam.double() * invstd
        b = bet.double() - mean * a
        z = a.view(1, -1, 1, 1) * yd + b.view(1, -1, 1, 1)
        zs = torch.sort(torch.relu(z).reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4), 1)[0]
        if z.abs().min() > 1e-4 and ((zs[:, 3] - zs[:, 2]) > 1e-4).logical_or(zs[:, 3] == 0).all():
            break
    else:
        raise AssertionError("no seed without near-ties")
    g_skip = torch.randn(B, C, H, W, generator=gen)
    g_pool = torch.randn(B, C, H // 2, W // 2, generator=gen)
    y64, ga64, be64 = yd.clone().requires_grad_(True), gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    out = torch.relu(F.batch_norm(y64, None, None, ga64, be64, True, 0.0, 1e-5))
    obj = (out * g_skip.double()).sum()
    if pooled:
        # an all-masked window sends its gradient to a ReLU that is off: nothing arrives either way
        obj = obj + (F.max_pool2d(out, 2) * g_pool.double()).sum()
    obj.backward()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().numpy()     # noqa: E731
    ref = R.bwd_ref("fp32", "pool" if pooled else "plain", nhwc(y), a.numpy(), b.numpy(), mean.numpy(), invstd.numpy(),
                    g=nhwc(g_skip), gpool=nhwc(g_pool) if pooled else None)
    for name, want in (("dy", nhwc(y64.grad).reshape(-1, C)), ("dgamma", ga64.grad.numpy()), ("dbeta", be64.grad.numpy())):
        got = ref[name][0]
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name


def _ext(ops, kw, rows, route):
    S = R.bwd_ref(ops["prec"], route, **kw)
    return R.split_sums(np.stack([S["dbeta"][0], S["dgamma"][0]], 1), rows)


@pytest.mark.parametrize("prec", PRECS)
def test_restatement_stays_within_the_backward_bounds(prec):
    worst = {r: Worst() for r in ("plain", "pool", "head", "ext")}
    for route, shapes in (("plain", R.PLAIN_SHAPES), ("pool", R.POOL_SHAPES)):
        for shape in shapes:
            kw = R.call_args(R.dense(prec, route, shape))
            us = 2.0 ** -7 if prec == "fp16" else 1.0
            worst[route].take(R.restate_bwd(prec, route, unscale=us, **kw), R.bwd_ref(prec, route, unscale=us, **kw), (route, shape))
    for shape in R.PLAIN_SHAPES:
        ops = R.dense(prec, "plain", shape)
        kw = R.call_args(ops)
        for rows in R.EXT_ROWS:
            kw["ext"] = _ext(ops, R.call_args(ops), rows, "plain")
            worst["ext"].take(R.restate_bwd(prec, "plain", **kw), R.bwd_ref(prec, "plain", **kw), ("ext", shape, rows))
    if prec != "fp32":
        for C in R.HEAD_WIDTHS:
            for npix in R.HEAD_NPIX:
                ops = R.dense(prec, "head", (1, C, 1, npix))
                for ncls in R.HEAD_CLASSES:
                    kw = R.call_args(ops, ncls)
                    kw["ext"] = _ext(ops, kw, 3, "head")
                    worst["head"].take(R.restate_bwd(prec, "head", **kw), R.bwd_ref(prec, "head", **kw), ("head", C, npix, ncls))
    for route, w in worst.items():
        if w:
            w.report(f"{prec} {route}")
    for route, w in worst.items():
        if w:
            recorded(w, (prec, route))


def test_restatement_stays_within_the_forward_bounds():
    worst = Worst()
    cases = [(n, C) for grid in (R.STATS_FUSED, R.STATS_TWO_LEVEL) for C in grid["C"] for n in grid["n_part"]]
    for n_part, C in cases:
        ops = R.make_partials(n_part, C)
        got, nbt = R.restate_stats(**ops)
        assert nbt == 1
        worst.take(got, R.stats_ref(**ops), (n_part, C))
    for C in (4, 6, 64):
        ops = R.make_partials_count1(C)
        worst.take(R.restate_stats(**ops)[0], R.stats_ref(**ops), ("count1", C))
    worst.report("forward")
    recorded(worst, "forward")


@pytest.mark.parametrize("prec", PRECS)
def test_exact_operands_are_exact(prec):
    """restatement == fp64 reference bit for bit, and every dy is a value of bf16 and of fp16"""
    cases = [("plain", s, None) for s in R.PLAIN_SHAPES] + [("pool", s, None) for s in R.POOL_SHAPES]
    cases += [("plain", s, rows) for s in R.PLAIN_SHAPES[1:3] for rows in R.EXT_ROWS]
    if prec != "fp32":
        cases += [("head", (1, C, 1, n), 3) for C in R.HEAD_WIDTHS for n in R.HEAD_NPIX]
    for route, shape, rows in cases:
        ops = R.exact(prec, route, shape)
        for ncls in (R.HEAD_CLASSES if route == "head" else (None,)):
            kw = R.call_args(ops, ncls)
            if rows:
                kw["ext"] = R.exact_ext(shape[1], shape[0] * shape[2] * shape[3], rows)
            got, ref = R.restate_bwd(prec, route, **kw), R.bwd_ref(prec, route, **kw)
            for name in ref:
                assert np.array_equal(got[name].astype(np.float64), ref[name][0]), (route, shape, rows, ncls, name)
            for dt in ("bf16", "fp16"):
                assert np.array_equal(R.round_to(got["dy"], R.PREC[dt]["dt"]), got["dy"]), (route, shape, dt)
            assert np.abs(ref["coef"][0]).max() > 0 and np.abs(ref["dy"][0]).max() > 0


def _leaves_the_bounds(got, ref):
    return max(R.worst_ratio(got[name], *ref[name]) for name in ref) > 1.0


@pytest.mark.parametrize("mut,route,shape", [
    ("mask_ge", "plain", (1, 12, 5, 7)), ("pool_last", "pool", (1, 8, 5, 7)), ("pool_edge", "pool", (1, 8, 5, 7)),
    ("s1_minus_pixel", "plain", (1, 12, 5, 7)), ("neighbour_mean", "plain", (1, 12, 5, 7)),
    ("coef_unscaled", "pool", (1, 8, 5, 7)), ("drop_last_row", "plain", (1, 12, 9, 10)), ("swap_vectors", "plain", (1, 12, 5, 7))])
@pytest.mark.parametrize("prec", PRECS)
def test_a_wrong_backward_leaves_the_bounds(prec, mut, route, shape):
    kw = R.call_args(R.dense(prec, route, shape))
    us = 2.0 ** -7
    ref = R.bwd_ref(prec, route, unscale=us, **kw)
    assert not _leaves_the_bounds(R.restate_bwd(prec, route, unscale=us, **kw), ref)
    assert _leaves_the_bounds(R.restate_bwd(prec, route, unscale=us, mut=mut, **kw), ref), mut


@pytest.mark.parametrize("mut", ["no_clamp", "no_conv_bias", "nbt_per_channel"])
def test_a_wrong_forward_leaves_the_bounds(mut):
    ops = R.make_partials_count1(64) if mut == "no_clamp" else R.make_partials(33, 6)
    ref = R.stats_ref(**ops)
    good, nbt = R.restate_stats(**ops)
    bad, nbt_bad = R.restate_stats(mut=mut, **ops)
    assert not _leaves_the_bounds(good, ref) and nbt == 1
    if mut == "nbt_per_channel":
        assert nbt_bad != 1
    else:
        assert _leaves_the_bounds(bad, ref)


def test_maxpool_reference_selects():
    x = np.array([[[[1.0], [-0.0]], [[0.0], [-3.0]]]], f32)
    assert R.maxpool_ref("fp32", x)[0, 0, 0, 0] == 1.0
    assert R.maxpool_ref("bf16", -x)[0, 0, 0, 0] == 3.0 and R.maxpool_ref("fp32", x, f32([-1]), f32([0.5]))[0, 0, 0, 0] == 3.5
