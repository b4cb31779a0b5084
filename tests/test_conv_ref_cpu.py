"""CPU: tests/tools/conv_ref.py on its own -- the reference against torch in float64, the bounds against a float32 restatement
(F.conv2d in float32 on the same rounded operands, then the store rounding: ratio <= 1 everywhere, a violated bound would be a
wrong derivation, never a reason to scale it), the operand generators' promises, negative controls on the reference alone, and
the route table: every entry takes the route it is named for under its switches, asked of the launcher's own decision."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
from tools import conv_ref as R   # noqa: E402

from floodplanet_code_amd import _lib   # noqa: E402

f32, f64 = np.float32, np.float64
PRECS = list(R.PREC)
SMALL = 1.5e9            # cases whose reference costs more than this many FLOP are left to the GPU file (same generator code)


def flops(c):
    B, C0, C1, Cout, H, W = c["shape"]
    return 2.0 * B * H * W * len(R.taps_of(c)) * (C0 + C1) * Cout


def nchw(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).transpose(0, 3, 1, 2)))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


@pytest.fixture
def lib():
    lib = _lib.load()
    try:
        yield lib
    finally:
        R.reset_hooks(lib)


# ---- reference against torch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [list(range(9)), [4]], ids=["3x3", "centre"])
def test_reference_equals_torch_in_float64(taps):
    g = np.random.default_rng(0)
    z, dy, w = g.standard_normal((2, 7, 19, 12)), g.standard_normal((2, 7, 19, 10)), g.standard_normal((10, 12, 3, 3))
    wt = torch.from_numpy(w)
    if taps == [4]:
        wt = torch.from_numpy(R._embed(w.copy(), 1))
    y = nhwc(F.conv2d(nchw(z), wt, padding=1))
    dx = nhwc(torch.nn.grad.conv2d_input((2, 12, 7, 19), wt, nchw(dy), padding=1))
    dw = torch.nn.grad.conv2d_weight(nchw(z), w.shape, nchw(dy), padding=1).numpy()
    if taps == [4]:
        dw = R._embed(dw, 1)
    for got, ref in ((R.conv_nhwc(z, w, taps), y), (R.dgrad_nhwc(dy, w, taps), dx), (R.wgrad_nhwc(z, dy, taps), dw)):
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


# ---- the 16-bit prologue is the fma, bit for bit --------------------------------------------------------------------------------
def fma32(a, x, b):
    """round-to-nearest-even float32 of the EXACT a * x + b, by rational arithmetic"""
    e = Fraction(float(a)) * Fraction(float(x)) + Fraction(float(b))
    c = f32(float(e))
    cand = sorted({c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(-np.inf))}, key=lambda v: (abs(Fraction(float(v)) - e),
                  int(np.asarray(v, f32).view(np.uint32)) & 1))
    return cand[0]


@pytest.mark.parametrize("prec", R.LOWP)
def test_prologue_restates_the_fused_form_and_ambiguous_finds_the_double_rounding(prec):
    # a * x = 1 + 2^-7 + 2^-17 + 2^-24 is a float32 tie; b = 2^-60 is lost in the float64 sum, which then rounds to even, while the
    # fma sees it and rounds up
    a, x, b = f32(1.0 + 2.0 ** -17), f32(1.0 + 2.0 ** -7), f32(2.0 ** -60)
    x3 = np.full((1, 1, 1, 1), x, f32)
    lo = f32(1.0 + 2.0 ** -7 + 2.0 ** -17)
    assert f32(f64(a) * f64(x) + f64(b)) == lo and fma32(a, x, b) == np.nextafter(lo, f32(2))
    assert R.ambiguous(x3, np.array([a]), np.array([b])).all()
    # an EXACT tie is no hazard: one rounding, to even, as the fma's
    assert not R.ambiguous(x3, np.array([a]), np.array([f32(0)])).any() and fma32(a, x, f32(0)) == lo
    c = R.BY_NAME["fwd_fast32_two_sources"]
    o = R.dense_operands(prec, c)
    assert o["replaced"] == 0 and not R.ambiguous(o["x0"], o["a"], o["b"]).any()
    assert (o["a"] > 0).any() and (o["a"] < 0).any()
    z = R.prologue(prec, o["x0"], o["a"], o["b"])
    idx = np.random.default_rng(1).integers(0, o["x0"].size, 3000)
    xs, ch = o["x0"].reshape(-1)[idx], idx % o["x0"].shape[-1]
    want = np.array([max(fma32(o["a"][k], v, o["b"][k]), f32(0)) for v, k in zip(xs, ch)], f32)
    assert np.array_equal(R.round_to(want, R.PREC[prec]["dt"]).astype(f64), z.reshape(-1)[idx])
    # the two-rounding form (bn_act: what the fp32 kernels and the whole-net references use) is another function: it differs from
    # the fused one in float32 at a good share of the elements, and still after the 16-bit rounding at a few
    two = np.maximum((o["x0"] * o["a"]).astype(f32) + o["b"], f32(0))
    fused = np.maximum((o["a"].astype(f64) * o["x0"] + o["b"]).astype(f32), f32(0))
    assert two.dtype == f32 and (two != fused).mean() > 0.01
    print(f"MEASURED {prec}: two-rounding and fused prologue differ at {int((R.round_to(two, R.PREC[prec]['dt']) != z).sum())} of {z.size} "
          "staged elements")


# ---- bounds against a float32 restatement ----------------------------------------------------------------------------------------
RESTATE = [(2, 8, 0, 64, 32, 16), (2, 32, 32, 64, 32, 16), (2, 256, 0, 64, 32, 16), (2, 16, 8, 40, 9, 11)]


@pytest.mark.parametrize("prec", PRECS)
def test_bounds_hold_for_a_float32_restatement(prec):
    dt = R.PREC[prec]["dt"]
    worst = {}

    def take(name, got, ref, bound):
        r = R.worst_ratio(got, ref, bound)
        worst[name] = max(worst.get(name, 0.0), r)
        assert r <= 1.0, (prec, name, r)
    for shape in RESTATE:
        B, C0, C1, Cout, H, W = shape
        for kind in ("fwd", "dgrad", "wgrad"):
            c = R.case("restate", kind, shape, "-", bn=True, prec=prec)
            o = R.dense_operands(prec, c)
            wt = torch.from_numpy(o["w"])
            if kind == "dgrad":
                dx = nhwc(torch.nn.grad.conv2d_input((B, C0 + C1, H, W), wt, nchw(o["dy"]), padding=1))
                assert dx.dtype == f32
                take("dx", R.round_to(dx, dt), *R.dgrad_ref(prec, o["dy"], o["w"]))
                continue
            z = R.staged_input(prec, o)
            z32 = z.astype(f32)
            assert np.array_equal(z32.astype(f64), z)
            if kind == "fwd":
                acc = nhwc(F.conv2d(nchw(z32), wt, padding=1))
                assert acc.dtype == f32
                ref = R.fwd_ref(prec, z, o["w"], o["bias"], 256)
                take("y", R.round_to(acc + o["bias"], dt), *ref["y"])
                # a tile's 256 pixels in float32, the tiles in float64: the partial rows and their collapse
                rows = acc.reshape(-1, Cout)
                part = [rows[i:i + 256] for i in range(0, rows.shape[0], 256)]
                take("sum", f32(sum(p.sum(0, dtype=f32).astype(f64) for p in part)), *ref["sum"])
                take("sqsum", f32(sum((p * p).sum(0, dtype=f32).astype(f64) for p in part)), *ref["sqsum"])
            else:
                dw = torch.nn.grad.conv2d_weight(nchw(z32), o["w"].shape, nchw(o["dy"]), padding=1).numpy()
                assert dw.dtype == f32
                take("dw", dw, *R.wgrad_ref(prec, z, o["dy"], B * H * W))
    print(f"MEASURED restatement {prec}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert set(worst) == set(R.MEASURED_RESTATEMENT[prec])


# ---- generator promises --------------------------------------------------------------------------------------------------------
def exact_result(prec, c, o):
    if c["kind"] == "fwd":
        z = R.staged_input(prec, o)
        return z, R.conv_nhwc(z, o["w"], R.taps_of(c)) + o["bias"], R.conv_nhwc(np.abs(z), np.abs(o["w"]), R.taps_of(c)) + np.abs(o["bias"])
    if c["kind"] == "dgrad":
        return None, R.dgrad_nhwc(o["dy"], o["w"], R.taps_of(c)), R.dgrad_nhwc(np.abs(o["dy"]), np.abs(o["w"]), R.taps_of(c))
    z = R.staged_input(prec, o)
    return z, R.wgrad_nhwc(z, o["dy"], R.taps_of(c)), R.wgrad_nhwc(np.abs(z), np.abs(o["dy"]), R.taps_of(c))


@pytest.mark.parametrize("name", [c["name"] for c in R.TABLE])
def test_exact_operands_are_exact_and_planted(name):
    c = R.BY_NAME[name]
    B, C0, C1, Cout, H, W = c["shape"]
    o = R.exact_operands(c)
    src = "dy" if c["kind"] == "dgrad" else "x0"
    # every planted position is there: crossings of the special rows and columns, first and last image, and every first and
    # last channel of an 8-channel chunk (so the last of source 0 and the first of source 1) carries a nonzero that survives
    # the prologue
    prec0 = R.precisions(c)[0]
    zin = np.asarray(o["dy"], f64) if c["kind"] == "dgrad" else R.staged_input(prec0, o)
    pos = R.planted_positions(B, H, W, zin.shape[-1], c["th"])
    assert all(zin[p] != 0 for p in pos)
    assert {p[3] for p in pos} == set(R.special_channels(zin.shape[-1]))
    assert {p[0] for p in pos} == {0, B - 1}
    ys, xs = {p[1] for p in pos}, {p[2] for p in pos}
    assert {0, H - 1} <= ys and {0, W - 1} <= xs
    assert all({k - 1, k} <= xs for k in range(16, W, 16)) and all({k - 1, k} <= ys for k in range(min(c["th"], 16), H, min(c["th"], 16)))
    if C1 and c["kind"] != "dgrad":
        assert (zin[..., C0 - 1] != 0).any() and (zin[..., C0] != 0).any()
    assert (o[src] == np.round(o[src])).all() and np.abs(o[src]).max() <= 2
    if c["kind"] == "wgrad":
        assert all(o["dy"][p] != 0 for p in R.planted_positions(B, H, W, Cout, c["th"]))
    if flops(c) > SMALL:
        return
    for prec in R.precisions(c):
        z, ref, mag = exact_result(prec, c, o)
        # the effective terms per output: sum |z| |w| + |bias| stays inside what the element type adds exactly
        cap = R.EXACT_CAP if c["kind"] != "wgrad" else 2.0 ** 24 * R.EXACT_UNIT
        assert mag.max() <= cap, (name, mag.max())
        dens = (zin != 0).mean()
        assert 0 < dens <= 0.03, dens
        # float64, float32 and the element type agree bit for bit
        wt = None if c["kind"] == "wgrad" else torch.from_numpy(o["w"])
        if c["kind"] == "fwd":
            r32 = nhwc(F.conv2d(nchw(z.astype(f32)), wt, torch.from_numpy(o["bias"]), padding=1))
        elif c["kind"] == "dgrad":
            r32 = nhwc(torch.nn.grad.conv2d_input((B, C0 + C1, H, W), wt, nchw(o["dy"]), padding=1))
        else:
            r32 = R._embed(torch.nn.grad.conv2d_weight(nchw(z.astype(f32)), (Cout, C0 + C1, 3, 3), nchw(o["dy"]), padding=1).numpy(),
                           c["center"])
        assert r32.dtype == f32 and np.array_equal(r32.astype(f64), ref), name
        if c["kind"] != "wgrad":
            assert np.array_equal(R.round_to(ref, R.PREC[prec]["dt"]).astype(f64), ref), name
            if prec == "bf16" and c["kind"] == "fwd" and B * H * W <= 4096:           # an evaluation in the element type itself
                rb = F.conv2d(nchw(z.astype(f32)).bfloat16(), wt.bfloat16(), torch.from_numpy(o["bias"]).bfloat16(), padding=1)
                assert np.array_equal(nhwc(rb.float()).astype(f64), ref), name


@pytest.mark.parametrize("prec", PRECS)
def test_dense_operands_hold_element_type_values_and_no_ambiguous_prologue(prec):
    for c in R.TABLE:
        if prec not in R.precisions(c) or flops(c) > SMALL:
            continue
        o = R.dense_operands(prec, c)
        dt = R.PREC[prec]["dt"]
        for k in ("x0", "x1", "dy", "w"):
            if o.get(k) is not None:
                assert np.array_equal(R.round_to(o[k], dt), o[k]), (c["name"], k)
        if c["bn"] and c["kind"] != "dgrad":
            assert (o["a"] > 0).any() and (o["a"] < 0).any()
            if prec != "fp32":
                assert not R.ambiguous(o["x0"], o["a"], o["b"]).any()
        if c["center"]:
            assert (R._embed(o["w"].copy(), 1) == o["w"]).all() and (o["w"][:, :, 1, 1] != 0).any()
        if c["kind"] == "fwd":
            y = R.fwd_ref(prec, R.staged_input(prec, o), o["w"], o["bias"], 256, R.taps_of(c))["y"][0]
            assert np.abs(y).max() < 100          # far inside fp16's 65504


# ---- negative controls on the reference alone ------------------------------------------------------------------------------------
def corruptions(z, w, C0, where):
    """{name: corrupted float64 accumulator}: what a subtly wrong kernel would give.  where = (b, y, x, channel) of a nonzero of
    z off the image border, whose 8-channel group is dropped from the centre tap at its own pixel."""
    B, H, W, Ci = z.shape
    ref = R.conv_nhwc(z, w)
    out = {}
    b, y, x, ch = where
    s = x + 1 if x + 2 < W else x - 1           # the column right of `where` is read in place of where's
    z2 = z.copy()
    z2[:, :, x, :] = z[:, :, s, :]
    out["halo column shifted by one"] = ref.copy()
    out["halo column shifted by one"][:, :, x - 1, :] = R.conv_nhwc(z2, w)[:, :, x - 1, :]
    g0 = 8 * (ch // 8)
    drop = ref.copy()
    drop[b, y, x, :] -= z[b, y, x, g0:g0 + 8] @ w[:, g0:g0 + 8, 1, 1].T
    out["one 8-channel group of one tap dropped at one pixel"] = drop
    w2 = w.copy()
    w2[:, :, 0, 1], w2[:, :, 2, 1] = w[:, :, 2, 1], w[:, :, 0, 1]
    out["two taps swapped"] = R.conv_nhwc(z, w2)
    if C0 < Ci:
        z3 = z.copy()
        z3[..., C0] = z[..., 0]
        out["source 1's first channel taken from source 0"] = R.conv_nhwc(z3, w)
    return ref, out


@pytest.mark.parametrize("prec", R.LOWP)
def test_negative_controls_exact_operands_fail_every_corruption(prec):
    for name in ("fwd_rs4_two_sources", "fwd_tap1_32", "fwd_c8_two_channel_tiles"):
        c = R.BY_NAME[name]
        if c["center"]:
            c = dict(c, center=0)                                   # the corruptions are of a 3x3
        o = R.exact_operands(c)
        z = R.staged_input(prec, o)
        B, H, W, _ = z.shape
        pos = [p for p in R.planted_positions(B, H, W, z.shape[-1], c["th"]) if 0 < p[1] < H - 1 and 1 < p[2] < W - 2]
        ref, bad = corruptions(z, o["w"].astype(f64), c["shape"][1], pos[len(pos) // 2])
        assert len(bad) == (4 if c["shape"][2] else 3)
        for what, r in bad.items():
            assert not np.array_equal(r, ref), (name, what)


@pytest.mark.parametrize("prec", R.LOWP)
@pytest.mark.parametrize("cin", [8, 64])
def test_negative_control_dense_bound_sees_a_dropped_channel_group(prec, cin):
    """Cin <= 64 only: at Cin = 256 the worst-case constant hides a single group (the module docstring's table)."""
    c = R.case("neg", "fwd", (2, cin, 0, 64, 32, 16), "-", bn=True)
    o = R.dense_operands(prec, c)
    z, w = R.staged_input(prec, o), o["w"].astype(f64)
    ref, bound = R.fwd_ref(prec, z, w, o["bias"], 256)["y"]
    zp = R._pad(z)
    g = np.random.default_rng(3)
    hits, N = 0, 300
    for _ in range(N):
        b, y, x, t, grp = g.integers(2), g.integers(32), g.integers(16), g.integers(9), g.integers(cin // 8)
        ky, kx = divmod(int(t), 3)
        d = zp[b, y + ky, x + kx, 8 * grp:8 * grp + 8] @ w[:, 8 * grp:8 * grp + 8, ky, kx].T
        got = R.round_to(ref[b, y, x] - d, R.PREC[prec]["dt"])
        hits += R.worst_ratio(got, ref[b, y, x], bound[b, y, x]) > 1.0 or not zp[b, y + ky, x + kx, 8 * grp:8 * grp + 8].any()
    print(f"MEASURED dropped-group detection {prec} Cin {cin}: {hits / N:.3f}")
    assert hits / N >= 0.9
    clean = R.round_to(ref, R.PREC[prec]["dt"])
    assert R.worst_ratio(clean, ref, bound) <= 1.0


# ---- the route table -------------------------------------------------------------------------------------------------------------
def test_every_table_entry_takes_the_route_it_is_named_for(lib):
    for c in R.TABLE:
        with R.hooks(lib, c):
            assert R.route_of(lib, c) == c["route"], c["name"]
    # ... and the switches are off again: forced routes are gone
    assert R.route_of(lib, R.BY_NAME["fwd_fast_tall"]) != "fast_tall" and R.route_of(lib, R.BY_NAME["dgrad_general64"]) != "general64"
    assert R.route_of(lib, R.BY_NAME["wgrad_lockstep128"]) == "pp"
    lowp = [c for c in R.TABLE if c["prec"] == "lowp"]
    assert {c["route"] for c in lowp if c["kind"] == "fwd"} == set(R.CONV_ROUTES)
    assert {c["route"] for c in lowp if c["kind"] == "dgrad"} == set(R.CONV_ROUTES)     # (a dgrad from 8 channels takes c8 too)
    assert {c["route"] for c in lowp if c["kind"] == "wgrad"} == set(R.WGRAD_ROUTES)
    for i in range(64):                     # the names are the library's own, all of them
        for kind, names in ((0, R.CONV_ROUTES), (2, R.WGRAD_ROUTES)):
            n = lib.fu_test_conv_route_name(kind, i).decode()
            assert (n in names) == (i < len(names)), (kind, i, n)
    f32c = [c for c in R.TABLE if c["prec"] == "fp32"]
    assert {(c["kind"], c["route"]) for c in f32c} == {("fwd", "f32_th4"), ("fwd", "f32_th8"), ("dgrad", "f32_th4"),
                                                       ("dgrad", "f32_th8"), ("wgrad", "f32")}
    assert {c["lock"] for c in lowp if c["route"] in ("pp", "lockstep128") and c["kind"] == "wgrad"} == {0, 1, 2}


def test_table_shapes_hold_the_conditions_they_were_chosen_for(lib):
    for c in R.TABLE:
        B, C0, C1, Cout, H, W = c["shape"]
        assert flops(c) <= 11e9, c["name"]
        if c["kind"] == "wgrad":
            for prec in R.precisions(c):
                n, S, per = R.wgrad_chain(prec, c, lib)
                assert n == min(B * H * W, per * np.prod(R.WGRAD_TILE[c["route"]])) + S + 4
                assert n <= R.DENSE_WGRAD_MAX_N, (c["name"], n)       # the dense element-wise bound is asserted on every case
    chain = {name: R.wgrad_chain("bf16", R.BY_NAME[name], lib) for name in ("wgrad_lockstep64", "wgrad_pp_two_tiles_per_split")}
    assert chain["wgrad_lockstep64"][1:] == (36, 1) and chain["wgrad_pp_two_tiles_per_split"][1:] == (64, 2)   # S == nPix; tiles > S
    kinds = {k: [c for c in R.TABLE if c["kind"] == k and c["prec"] == "lowp"] for k in ("fwd", "dgrad", "wgrad")}
    assert any(c["shape"][2] for c in kinds["fwd"]) and any(c["shape"][2] for c in kinds["wgrad"]) and any(c["shape"][2] for c in kinds["dgrad"])
    assert any(c["bn"] for c in kinds["fwd"]) and any(not c["bn"] for c in kinds["fwd"])
    # the persistent kernel's second trip: more tiles than the 256 workgroups its launcher starts at most
    for name in ("fwd_pp_second_trip", "dgrad_pp_second_trip"):
        B, C0, C1, Cout, H, W = R.BY_NAME[name]["shape"]
        n_out = Cout if name.startswith("fwd") else C0 + C1
        assert B * (H // 32) * (W // 16) * (n_out // 64) > 256


def test_one_tap_hook_reaches_the_route_query_only_through_the_case(lib):
    c = R.BY_NAME["fwd_tap1_32"]
    with R.hooks(lib, c):
        lib.fu_test_force_full_taps(1)
        assert R.route_of(lib, c) == "fast32"        # fu_test_force_full_taps overrides the embedded 1x1
    assert R.route_of(lib, dict(c, center=0)) == "fast32"
