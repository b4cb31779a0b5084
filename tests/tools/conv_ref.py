"""fp64 reference of the 3x3 convolutions (forward with its batch statistics, dgrad, wgrad) over the exact values the kernels
multiply, analytic per-element bounds of a float32 evaluation of them, the two operand generators and the route table of the
op-level tests (tests/test_conv_ref_cpu.py pins this file without a GPU, tests/test_gpu_conv_ops.py runs the kernels to it).

Layout: activations NHWC [B, H, W, C] float32 arrays holding values the element type represents exactly, weights OIHW
[Cout, Cin, 3, 3], bias [Cout], a / b [C0] float32 or None (the BatchNorm + ReLU prologue of source 0).

PARITY DEFINITION
  16-bit   z = round_to(max(fma(a, x, b), 0))   one float32 rounding (bn_act_fused), then the rounding to the element type of
           the staging (bn_relu_pack8, the fast / rs / pp staging, fu_wgrad_bf16.hip).  prologue() restates it bit for bit:
           a * x is exact in float64 (24 x 11 bits), so float32(float64(a * x + b)) is the fma unless the float64 sum sits on a
           float32 rounding boundary; ambiguous() finds those elements and the generator replaces them.
  fp32     z = max(fl(fl(a * x) + b), 0)        two float32 roundings (bn_act): numpy's float32 operators.
  forward  acc = sum_{tap, ci} z * w,  y = round_to(acc + bias);  statistics sum_p acc and sum_p acc^2 of the UNROUNDED, bias-free
           accumulator (every epilogue adds `a` / `v` before the bias: fu_conv_bf16.hip, _fast, _rs, _pp, fu_conv_f32.hip)
  dgrad    dx = round_to(sum_{tap, co} dy * w), split at D0 into one or two destinations
  wgrad    dw[co, ci, tap] = sum_p dy * z in float32 OIHW

BOUNDS (derived, none fitted).  A sum of n products accumulated in float32 in ANY order in which no term passes through more
than n roundings differs from the exact sum by at most g(n) sum |a| |b|, g(n) = n u / (1 - n u).
  * 16-bit MFMA routes: u = 2^-23.  The products of two 16-bit values are exact in float32; the internal rounding of a
    16-bit-input MFMA's additions is not documented, and a unit of 2^-23 covers round to nearest, chopping and align-then-
    truncate alike.  fp32: u = 2^-24 (v_mfma_f32_32x32x2_f32 is bitwise a k-ordered fmaf chain: one rounding per term).
  * forward: n = taps * Cin + 1 (the bias addition), dgrad: n = taps * Cout; taps = 9, or 1 on the one-tap routes.
    bound = b32 + one rounding to the element type (head_ref.store_bound), b32 = g(n) (sum |z| |w| + |bias|); where
    sum |z| |w| + |bias| = 0 the bound is 0 and the result must be exactly 0.
  * statistics: the kernels add a tile's accumulators in float32 (per lane, across lanes, across waves: at most T = pixels of
    the route's tile roundings for any term, STAT_TILE_PX), write one partial row per tile (launch's nPix rows, at most
    conv3x3_num_stat_tiles) and the hook's collapse adds the rows in float64 and rounds once.  With e = g(taps * Cin) sum|z||w|
    the accumulator's own error:
        sum   bound = sum_p e + g(T + 1) sum_p (|acc| + e)
        sqsum bound = sum_p (2 |acc| e + e^2) + g(T + 2) sum_p (|acc| + e)^2        (one more rounding: the square)
  * wgrad: every pixel of the batch feeds one element.  A workgroup accumulates its perSplit pixel tiles in one float32
    accumulator (<= min(B H W, perSplit * tile pixels) roundings, +3 for the cross-wave sum of the 8-channel kernel), the reduce
    (fu_conv.hip) adds the S slabs: <= ceil(S / SL) + 2 float32 additions per split lane, the lanes in float64, one rounding.
        n = min(B H W, perSplit * tile) + S + 4,   bound = g(n) sum_p |dy| |z|
    S is the launcher's own (fu_test_wgrad_slab; fp32: wgrad_split_shared restated in wgrad_chain).  A constant of n ~ 8000 would
    be looser than the norm check the dense tests keep, so the element-wise bound is asserted only where n * 2^-23 < 1e-4
    (DENSE_WGRAD_MAX_N) -- which every case of the table is: the split-K plans give a workgroup one or two 128-pixel stages, n =
    74 .. 324.  The bound still scales with sum |dy| |z| over every pixel, so it is weak against one lost product; the exact
    operands carry the structure.

TWO OPERAND KINDS
  dense   randn activations, randn / (3 sqrt(Cin)) weights, a prologue with both signs of a, a bias: accumulation and store.
  exact   sparse small integers (activations) times integers / 8 (weights, bias): every product and every partial sum is exact
          in the element type and in float32 (sum |z| |w| + |bias| <= EXACT_CAP = 256 / 8, asserted), so the reference IS the
          answer and the tests assert bit equality.  Nonzeros are planted at the crossings of the special columns (0, W - 1,
          both sides of every 16-pixel seam) with the special rows (0, H - 1, both sides of every seam of the case's tile
          height), in the first and last image, on the first and last channel of every 8-channel chunk (which holds every
          16 / 32-chunk edge, the last channel of source 0 and the first of source 1); the weights are dense, so both sides
          of the D0 boundary and every tap carry values.  Random nonzeros fill the rest at min(2 %, 8 / (9 Cin)): the cap, not
          the nominal density, is what the CPU test asserts.  Structure (tap, channel, seam, halo, split-K ownership) is what
          these see; the dense bound cannot see a single product at Cin = 256.
"""
import ctypes
import functools
import zlib

import numpy as np
import torch

from .head_ref import PREC, round_to, store_bound   # noqa: F401  (the element types' eps / tiny, the store rounding)
from .resample_ref import worst_ratio               # noqa: F401

f32, f64 = np.float32, np.float64
U = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -23, "fp16": 2.0 ** -23}
LOWP = ("bf16", "fp16")
DENSE_WGRAD_MAX_N = 838                  # n * 2^-23 < 1e-4
EXACT_UNIT, EXACT_CAP = 0.125, 32.0      # weights and bias are integers / 8; sums up to 256 units are exact in bf16's 8 bits
# pixels of one statistics row (the route's tile): conv_geometry's tw x th of every launcher
STAT_TILE_PX = {"general64": 256, "general32": 256, "tap1_64": 256, "tap1_32": 256, "fast64": 256, "fast32": 256,
                "fast_tall": 512, "rs4": 256, "rs8": 512, "pp": 512, "c8": 1024, "f32_th4": 64, "f32_th8": 128}
# pixels of one weight-gradient stage: 8 x 16 (WCfg<.., 8>, WPCfg), 8 x 32 (WC8), 4 x 16 (k_wgrad_f32)
WGRAD_TILE = {"tap1_wide": (8, 16), "tap1_narrow": (8, 16), "pp": (8, 16), "lockstep128": (8, 16), "lockstep64": (8, 16),
              "c8": (8, 32), "f32": (4, 16)}

# worst err / bound of the float32 restatement (F.conv2d in float32 on the rounded operands, then round_to) over the small
# cases of test_conv_ref_cpu.py, as that test printed them
MEASURED_RESTATEMENT = {
    "fp32": dict(y=0.063, dx=0.004, dw=0.020, sum=0.010, sqsum=0.008),
    "bf16": dict(y=0.992, dx=0.927, dw=0.003, sum=0.003, sqsum=0.003),
    "fp16": dict(y=0.955, dx=0.660, dw=0.008, sum=0.003, sqsum=0.004),
}
# worst err / bound on the MI355X per precision, output ("fwd" = y, "dgrad" = dx, "wgrad" = dw, "stats" = the larger of sum and
# sqsum) and route, dense operands, as test_gpu_conv_ops.py printed them (a pass is <= 1; "+full_taps": the embedded 1x1 under
# fu_test_force_full_taps).  The 16-bit outputs sit near 1 by construction -- the store rounding reaches the element type's unit
# roundoff -- and the fp32 figures show the accumulator's own share.  Every exact case was bit-equal; the file takes about 20 s.
MEASURED_GPU = {
    "bf16": {
        "stats": {
            "general32": 0.001, "general64": 0.000, "fast32": 0.000, "fast64": 0.000, "fast_tall": 0.000,
            "rs4": 0.000, "rs8": 0.000, "pp": 0.000, "c8": 0.000, "tap1_32": 0.001, "tap1_32+full_taps": 0.000,
            "tap1_64": 0.001, "tap1_64+full_taps": 0.000},
        "fwd": {
            "general32": 0.952, "general64": 0.959, "fast32": 0.865, "fast64": 0.974, "fast_tall": 0.974,
            "rs4": 0.919, "rs8": 0.968, "pp": 0.942, "c8": 0.988, "tap1_32": 0.986, "tap1_32+full_taps": 0.948,
            "tap1_64": 0.991, "tap1_64+full_taps": 0.967},
        "dgrad": {
            "general32": 0.915, "general64": 0.973, "fast32": 0.876, "fast64": 0.967, "fast_tall": 0.967,
            "rs4": 0.909, "rs8": 0.967, "pp": 0.911, "c8": 0.989, "tap1_32": 0.984, "tap1_32+full_taps": 0.954,
            "tap1_64": 0.992, "tap1_64+full_taps": 0.967},
        "wgrad": {
            "lockstep64": 0.001, "pp": 0.001, "lockstep128": 0.001, "c8": 0.000, "tap1_wide": 0.000,
            "tap1_wide+full_taps": 0.001, "tap1_narrow": 0.001, "tap1_narrow+full_taps": 0.001},
    },
    "fp16": {
        "stats": {
            "general32": 0.000, "general64": 0.000, "fast32": 0.000, "fast64": 0.000, "fast_tall": 0.000,
            "rs4": 0.000, "rs8": 0.000, "pp": 0.000, "c8": 0.000, "tap1_32": 0.000, "tap1_32+full_taps": 0.000,
            "tap1_64": 0.001, "tap1_64+full_taps": 0.000},
        "fwd": {
            "general32": 0.811, "general64": 0.780, "fast32": 0.502, "fast64": 0.857, "fast_tall": 0.857,
            "rs4": 0.668, "rs8": 0.827, "pp": 0.710, "c8": 0.956, "tap1_32": 0.941, "tap1_32+full_taps": 0.724,
            "tap1_64": 0.966, "tap1_64+full_taps": 0.806},
        "dgrad": {
            "general32": 0.692, "general64": 0.883, "fast32": 0.469, "fast64": 0.817, "fast_tall": 0.817,
            "rs4": 0.641, "rs8": 0.846, "pp": 0.651, "c8": 0.958, "tap1_32": 0.956, "tap1_32+full_taps": 0.791,
            "tap1_64": 0.964, "tap1_64+full_taps": 0.797},
        "wgrad": {
            "lockstep64": 0.001, "pp": 0.002, "lockstep128": 0.001, "c8": 0.000, "tap1_wide": 0.000,
            "tap1_wide+full_taps": 0.001, "tap1_narrow": 0.001, "tap1_narrow+full_taps": 0.001},
    },
    "fp32": {
        "stats": {
            "f32_th4": 0.001, "f32_th8": 0.001},
        "fwd": {
            "f32_th4": 0.018, "f32_th8": 0.033},
        "dgrad": {
            "f32_th4": 0.009, "f32_th8": 0.052},
        "wgrad": {
            "f32": 0.023},
    },
}


def gamma(n, prec):
    u = U[prec]
    return n * u / (1.0 - n * u)


# ---- the prologue ------------------------------------------------------------------------------------------------------------
def prologue(prec, x, a, b):
    """float64 z [B, H, W, C] of source 0: what the kernels stage (see the module docstring)"""
    if a is None:
        return np.asarray(x, f64)
    if prec == "fp32":
        p = np.asarray(x, f32) * np.asarray(a, f32)
        s = p + np.asarray(b, f32)
        assert s.dtype == f32
        return np.maximum(s, f32(0)).astype(f64)
    s = np.asarray(a, f64) * np.asarray(x, f64) + np.asarray(b, f64)
    return round_to(np.maximum(s.astype(f32), f32(0)), PREC[prec]["dt"]).astype(f64)


def ambiguous(x, a, b):
    """elements where float32(float64(a * x + b)) could differ from the fma: the float64 sum is INEXACT (TwoSum leaves a
    remainder; an exact sum rounds once, ties included, exactly as the fma does) and sits within 2^-20 of a half-ulp of a
    float32 rounding boundary.  h is half the spacing above |s32|, h / 2 half the spacing below it when |s32| is a power of two."""
    ax, b = np.asarray(a, f64) * np.asarray(x, f64), np.broadcast_to(np.asarray(b, f64), np.shape(x))
    s = ax + b
    bv = s - ax
    inexact = ((ax - (s - bv)) + (b - bv)) != 0
    s32 = s.astype(f32)
    err = np.abs(s - s32.astype(f64))
    h = np.spacing(np.abs(s32)).astype(f64) / 2
    return inexact & (np.minimum(np.abs(err - h), np.abs(err - h / 2)) < h * 2.0 ** -20)


# ---- float64 convolutions, NHWC, as nine shifted matrix products -------------------------------------------------------------
def _pad(x):
    return np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))


def _cols(z, taps):
    """[B H W, len(taps) * C]: the shifted copies of z side by side (tap 3 * ky + kx reads pixel (y + ky - 1, x + kx - 1))"""
    B, H, W, C = z.shape
    zp = _pad(z)
    cols = np.empty((B, H, W, len(taps) * C))
    for i, t in enumerate(taps):
        ky, kx = divmod(t, 3)
        cols[..., i * C:(i + 1) * C] = zp[:, ky:ky + H, kx:kx + W, :]
    return cols.reshape(B * H * W, -1)


def conv_nhwc(z, w, taps=range(9)):
    """[B, H, W, Cout] = sum over the given taps (3 * ky + kx) of the shifted z times w[:, :, ky, kx]; float64"""
    z, w, taps = np.asarray(z, f64), np.asarray(w, f64), list(taps)
    B, H, W, _ = z.shape
    wm = np.concatenate([w[:, :, t // 3, t % 3].T for t in taps], 0)
    return (_cols(z, taps) @ wm).reshape(B, H, W, -1)


def dgrad_nhwc(dy, w, taps=range(9)):
    """[B, H, W, Cin]: the convolution of dy with the transposed, mirrored weights"""
    wt = np.asarray(w, f64).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
    return conv_nhwc(dy, wt, [8 - t for t in taps])


def wgrad_nhwc(z, dy, taps=range(9)):
    """OIHW [Cout, Cin, 3, 3]; the taps not asked for stay 0"""
    z, dy, taps = np.asarray(z, f64), np.asarray(dy, f64), list(taps)
    Ci, Co = z.shape[-1], dy.shape[-1]
    g = (dy.reshape(-1, Co).T @ _cols(z, taps)).reshape(Co, len(taps), Ci)
    out = np.zeros((Co, Ci, 3, 3))
    for i, t in enumerate(taps):
        out[:, :, t // 3, t % 3] = g[:, i, :]
    return out


# ---- references with their bounds ----------------------------------------------------------------------------------------------
def fwd_parts(z, w, taps=range(9)):
    """(acc, sum |z| |w|): the two convolutions every forward bound needs, shared between the routes that run one shape"""
    return conv_nhwc(z, w, taps), conv_nhwc(np.abs(z), np.abs(w), taps)


def dgrad_parts(dy, w, taps=range(9)):
    return dgrad_nhwc(dy, w, taps), dgrad_nhwc(np.abs(dy), np.abs(w), taps)


def wgrad_parts(z, dy, taps=range(9)):
    return wgrad_nhwc(z, dy, taps), wgrad_nhwc(np.abs(z), np.abs(dy), taps)


def fwd_ref(prec, z, w, bias, stat_px, taps=range(9), parts=None, chain_taps=None):
    """{"y" | "sum" | "sqsum": (ref, bound)}; z = the concatenated, staged input [B, H, W, Cin] in float64.  chain_taps: the
    taps the kernel really accumulates (9 for an embedded 1x1 under fu_test_force_full_taps: its zeros cost roundings)."""
    taps = list(taps)
    n = (chain_taps or len(taps)) * z.shape[-1]
    bias = np.asarray(bias, f64)
    acc, mag = parts or fwd_parts(z, w, taps)
    y, ymag = acc + bias, mag + np.abs(bias)
    e = gamma(n, prec) * mag
    am = np.abs(acc) + e
    ax = (0, 1, 2)
    return {"y": (y, store_bound(prec, y, ymag, gamma(n + 1, prec) * ymag)),
            "sum": (acc.sum(ax), e.sum(ax) + gamma(stat_px + 1, prec) * am.sum(ax)),
            "sqsum": ((acc * acc).sum(ax), (2 * np.abs(acc) * e + e * e).sum(ax) + gamma(stat_px + 2, prec) * (am * am).sum(ax))}


def dgrad_ref(prec, dy, w, taps=range(9), parts=None, chain_taps=None):
    """(ref, bound) of dx [B, H, W, Cin] (both destinations side by side: split at D0 by the caller)"""
    taps = list(taps)
    n = (chain_taps or len(taps)) * dy.shape[-1]
    dx, mag = parts or dgrad_parts(dy, w, taps)
    return dx, store_bound(prec, dx, mag, gamma(n, prec) * mag)


def wgrad_ref(prec, z, dy, n, taps=range(9), parts=None):
    """(ref, bound) of dw OIHW for a chain of n roundings (wgrad_chain)"""
    dw, mag = parts or wgrad_parts(z, dy, list(taps))
    return dw, gamma(n, prec) * mag


def wgrad_chain(prec, case, lib=None):
    """n of the module docstring for a weight-gradient case: (n, S, perSplit)"""
    B, C0, C1, Cout, H, W = case["shape"]
    if prec == "fp32":                                   # wgrad_split_shared, fu_conv_f32.hip
        th, tw = WGRAD_TILE["f32"]
        npix = B * -(-H // th) * -(-W // tw)
        s = max(1, min(npix, -(-512 // (-(-(C0 + C1) // 64) * -(-Cout // 64)))))
        per = -(-npix // s)
        S = -(-npix // per)
    else:
        with hooks(lib, case):
            used = ctypes.c_int64()
            r = lib.fu_test_wgrad_slab(C0, int(case["bn"]), C1, Cout, case["center"], B, H, W, ctypes.byref(used), None)
            route = lib.fu_test_conv_route_name(2, r).decode()
        th, tw = WGRAD_TILE[route]
        npix = B * -(-H // th) * -(-W // tw)
        S = used.value // (9 * (C0 + C1) * Cout)
        per = -(-npix // S)
        assert -(-npix // per) == S
    return min(B * H * W, per * th * tw) + S + 4, S, per


# ---- the route table -------------------------------------------------------------------------------------------------------------
def case(name, kind, shape, route, bn=False, th=16, general=0, tile=0, lock=0, center=0, bnsums=0, prec="lowp"):
    """shape = (B, C0, C1, Cout, H, W): sources / destinations 0 and 1 have C0 and C1 channels, dy / y has Cout.  th: the tile
    height whose seams the exact operands straddle.  general / tile / lock: fu_test_force_general_conv, fu_test_conv_tile_mode,
    fu_test_force_lockstep_wgrad; center: fu_test_op_center_only; bnsums: through fu_op_conv3x3_dgrad_bnsums (dx only)."""
    return dict(name=name, kind=kind, shape=shape, route=route, bn=bn, th=th, general=general, tile=tile, lock=lock,
                center=center, bnsums=bnsums, prec=prec)


TABLE = [
    # ---- 16-bit forward: every ConvRoute ------------------------------------------------------------------------------------
    case("fwd_general32_ragged", "fwd", (2, 16, 8, 40, 9, 11), "general32", bn=True),        # the source switches inside a chunk
    case("fwd_general64", "fwd", (4, 24, 16, 128, 128, 128), "general64", general=1),        # wg256 = 512; 40 channels: 2 chunks
    case("fwd_fast32_one_tile", "fwd", (1, 96, 0, 32, 16, 16), "fast32"),
    case("fwd_fast32_two_sources", "fwd", (2, 64, 32, 96, 48, 80), "fast32", bn=True),
    case("fwd_fast64", "fwd", (4, 32, 0, 128, 128, 128), "fast64", bn=True, tile=1, th=32),
    case("fwd_fast_tall", "fwd", (4, 32, 0, 128, 128, 128), "fast_tall", bn=True, tile=2, th=32),
    case("fwd_rs4", "fwd", (2, 64, 0, 64, 48, 48), "rs4", bn=True, tile=3),
    case("fwd_rs4_two_sources", "fwd", (1, 64, 64, 128, 96, 32), "rs4", bn=True, tile=3),
    case("fwd_rs8", "fwd", (4, 32, 0, 256, 128, 128), "rs8", tile=3, th=32),                 # wg512 = 512
    case("fwd_pp_odd_chunks", "fwd", (3, 96, 0, 64, 64, 32), "pp", tile=4, th=32),           # 12 tiles, 3 chunks
    case("fwd_pp_two_sources", "fwd", (4, 64, 64, 64, 64, 32), "pp", bn=True, tile=4, th=32),
    case("fwd_pp_second_trip", "fwd", (3, 64, 0, 128, 96, 240), "pp", bn=True, tile=4, th=32),   # 270 tiles > 256 workgroups
    case("fwd_c8_tall", "fwd", (2, 8, 0, 64, 64, 48), "c8", th=64),                          # 16 x 64 tiles
    case("fwd_c8_two_channel_tiles", "fwd", (1, 8, 0, 128, 48, 32), "c8"),                   # 16 x 16 tiles
    case("fwd_tap1_32", "fwd", (2, 64, 32, 64, 48, 48), "tap1_32", bn=True, center=1),
    case("fwd_tap1_64", "fwd", (4, 64, 0, 128, 128, 128), "tap1_64", center=1),
    # ---- 16-bit dgrad: the roles swapped (Cout channels in, C0 + C1 out, split at D0 = C0) ----------------------------------------
    case("dgrad_general32_ragged", "dgrad", (2, 16, 8, 40, 9, 11), "general32"),
    case("dgrad_general64", "dgrad", (4, 96, 32, 24, 128, 128), "general64", general=1),
    case("dgrad_fast32", "dgrad", (2, 64, 32, 96, 48, 80), "fast32"),
    case("dgrad_fast64", "dgrad", (4, 64, 64, 32, 128, 128), "fast64", tile=1, th=32),
    case("dgrad_fast_tall", "dgrad", (4, 64, 64, 32, 128, 128), "fast_tall", tile=2, th=32),
    case("dgrad_rs4", "dgrad", (2, 64, 0, 64, 48, 48), "rs4", tile=3),
    case("dgrad_rs4_two_destinations", "dgrad", (1, 64, 64, 128, 96, 32), "rs4", tile=3),
    case("dgrad_rs8", "dgrad", (4, 256, 0, 32, 128, 128), "rs8", tile=3, th=32),
    case("dgrad_pp_odd_chunks", "dgrad", (3, 64, 0, 96, 64, 32), "pp", tile=4, th=32),
    case("dgrad_pp_two_destinations", "dgrad", (4, 128, 64, 64, 32, 16), "pp", tile=4, th=32),
    case("dgrad_pp_second_trip", "dgrad", (3, 128, 0, 64, 96, 240), "pp", tile=4, th=32),
    case("dgrad_c8_tall", "dgrad", (2, 64, 0, 8, 64, 48), "c8", th=64),                       # a dgrad from 8 channels is eligible too
    case("dgrad_c8_two_channel_tiles", "dgrad", (1, 128, 0, 8, 48, 32), "c8"),
    case("dgrad_tap1_32", "dgrad", (2, 64, 0, 64, 48, 48), "tap1_32", center=1),
    case("dgrad_tap1_64", "dgrad", (4, 128, 0, 64, 128, 128), "tap1_64", center=1),
    case("dgrad_bnsums_rs4", "dgrad", (2, 64, 0, 64, 64, 48), "rs4", tile=3, bnsums=1),
    case("dgrad_bnsums_pp", "dgrad", (1, 64, 0, 256, 64, 64), "pp", tile=4, th=32, bnsums=1),
    # ---- 16-bit wgrad: every WgradRoute, the ping-pong kernel's three stagings -------------------------------------------------
    case("wgrad_lockstep64", "wgrad", (2, 32, 32, 64, 48, 48), "lockstep64", bn=True, th=8),         # S == nPix
    case("wgrad_pp_whole_tile", "wgrad", (2, 64, 64, 128, 48, 48), "pp", bn=True, th=8),
    case("wgrad_lockstep128", "wgrad", (2, 64, 64, 128, 48, 48), "lockstep128", bn=True, th=8, lock=1),
    case("wgrad_pp_general_staging", "wgrad", (2, 64, 64, 128, 48, 48), "pp", bn=True, th=8, lock=2),
    case("wgrad_pp_ragged", "wgrad", (2, 128, 64, 64, 40, 24), "pp", bn=True, th=8),
    case("wgrad_pp_two_tiles_per_split", "wgrad", (16, 128, 0, 128, 32, 32), "pp", th=8),            # 128 tiles, 64 splits
    case("wgrad_c8", "wgrad", (3, 8, 0, 64, 40, 96), "c8", th=8),
    case("wgrad_tap1_wide", "wgrad", (2, 128, 0, 64, 48, 48), "tap1_wide", th=8, center=1),
    case("wgrad_tap1_narrow", "wgrad", (2, 32, 32, 64, 48, 48), "tap1_narrow", bn=True, th=8, center=1),
    # ---- fp32: both TH instantiations of k_conv3x3_f32 (forward and dgrad), k_wgrad_f32 ------------------------------------------
    case("f32_fwd_th4_ragged", "fwd", (2, 16, 8, 40, 9, 11), "f32_th4", bn=True, th=4, prec="fp32"),   # Cin = 24, N = 40
    case("f32_fwd_th8_ragged", "fwd", (2, 12, 8, 72, 90, 250), "f32_th8", bn=True, th=8, prec="fp32"),  # Cin = 20, N = 72
    case("f32_dgrad_th4_ragged", "dgrad", (2, 16, 8, 40, 9, 11), "f32_th4", th=4, prec="fp32"),
    case("f32_dgrad_th8_two_destinations", "dgrad", (2, 40, 32, 12, 90, 250), "f32_th8", th=8, prec="fp32"),
    case("f32_wgrad_ragged", "wgrad", (2, 16, 8, 40, 9, 11), "f32", bn=True, th=4, prec="fp32"),
]
BY_NAME = {c["name"]: c for c in TABLE}
assert len(BY_NAME) == len(TABLE)
CONV_ROUTES = ("general64", "general32", "tap1_64", "tap1_32", "c8", "pp", "rs8", "rs4", "fast_tall", "fast64", "fast32")
WGRAD_ROUTES = ("tap1_wide", "tap1_narrow", "c8", "pp", "lockstep128", "lockstep64")


def precisions(c):
    return LOWP if c["prec"] == "lowp" else (c["prec"],)


class hooks:
    """the case's switches set on the library, and ALWAYS reset on the way out"""

    def __init__(self, lib, c):
        self.lib, self.c = lib, c

    def __enter__(self):
        c, lib = self.c, self.lib
        lib.fu_test_force_general_conv(c["general"])
        lib.fu_test_conv_tile_mode(c["tile"])
        lib.fu_test_force_lockstep_wgrad(c["lock"])
        lib.fu_test_op_center_only(c["center"])
        return self

    def __exit__(self, *exc):
        reset_hooks(self.lib)


def reset_hooks(lib):
    lib.fu_test_force_general_conv(0)
    lib.fu_test_conv_tile_mode(0)
    lib.fu_test_force_lockstep_wgrad(0)
    lib.fu_test_force_full_taps(0)
    lib.fu_test_op_center_only(0)


def route_of(lib, c):
    """the route the launcher takes for the case under the switches currently set (no GPU needed)"""
    B, C0, C1, Cout, H, W = c["shape"]
    if c["prec"] == "fp32":
        if c["kind"] == "wgrad":
            return "f32"
        n = Cout if c["kind"] == "fwd" else C0 + C1
        return "f32_th%d" % lib.fu_test_conv_f32_tile_rows(B, H, W, n)
    if c["kind"] == "fwd":
        r = lib.fu_test_conv_route(0, C0, int(c["bn"]), C1, Cout, 0, c["center"], 0, B, H, W)
        return lib.fu_test_conv_route_name(0, r).decode()
    if c["kind"] == "dgrad":
        r = lib.fu_test_conv_route(1, Cout, 0, 0, C0, C1, c["center"], c["bnsums"], B, H, W)
        return lib.fu_test_conv_route_name(1, r).decode()
    r = lib.fu_test_conv_route(2, C0, int(c["bn"]), C1, Cout, 0, c["center"], 0, B, H, W)
    return lib.fu_test_conv_route_name(2, r).decode()


def taps_of(c):
    return [4] if c["center"] else list(range(9))


# ---- operands ----------------------------------------------------------------------------------------------------------------
def special_axis(n, step):
    """0, n - 1 and both sides of every seam (a multiple of step)"""
    s = {0, n - 1}
    for k in range(step, n, step):
        s.update((k - 1, k))
    return sorted(s)


def special_channels(C):
    """first and last channel of every 8-channel chunk (a ragged tail's last channel included)"""
    s = set()
    for k in range(0, C, 8):
        s.update((k, min(k + 7, C - 1)))
    return sorted(s)


def planted_positions(B, H, W, C, th):
    """[(image, row, column, channel)]: two channels at every crossing of a special row and column, first and last image.
    Rows: the seams of min(th, 16) pixels, which hold those of the 32- and 64-row tiles."""
    ys, xs, cs = special_axis(H, min(th, 16)), special_axis(W, 16), special_channels(C)
    imgs = sorted({0, B - 1})
    k = max(1, -(-len(cs) // (len(ys) * len(xs) * len(imgs))))      # enough channels per crossing to reach every special one
    out, i = [], 0
    for b in imgs:
        for y in ys:
            for x in xs:
                for ch in sorted({cs[(i * k + j) % len(cs)] for j in range(k)} | {cs[(7 * i + 3) % len(cs)]}):
                    out.append((b, y, x, ch))
                i += 1
    return out


def _embed(w, center):
    """an embedded 1x1: every tap but the centre one is zero"""
    if center:
        w[:, :, [0, 0, 0, 1, 1, 2, 2, 2], [0, 1, 2, 0, 2, 0, 1, 2]] = 0
    return w


def _seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=4)
def _dense(prec, shape, kind, bn, center):
    B, C0, C1, Cout, H, W = shape
    dt = PREC[prec]["dt"]
    g = torch.Generator().manual_seed(_seed(shape, kind, bn))
    rn = lambda *s: torch.randn(*s, generator=g).numpy()   # noqa: E731
    Cin = C0 + C1
    o = dict(w=_embed(round_to(rn(Cout, Cin, 3, 3) / (3.0 * Cin ** 0.5), dt), center))
    if kind in ("fwd", "wgrad"):
        o["x0"], o["x1"] = round_to(rn(B, H, W, C0), dt), (round_to(rn(B, H, W, C1), dt) if C1 else None)
        o["a"] = o["b"] = None
        if bn:
            a = (torch.rand(C0, generator=g) + 0.5).numpy()
            a[1::3] *= -1                                    # both signs of a
            o["a"], o["b"] = a.astype(f32), (rn(C0) * 0.3).astype(f32)
            if prec != "fp32":
                amb = ambiguous(o["x0"], o["a"], o["b"])
                o["replaced"] = int(amb.sum())
                o["x0"] = np.where(amb, f32(1.0), o["x0"])
        o["bias"] = (rn(Cout) * 0.1).astype(f32)
    if kind in ("dgrad", "wgrad"):
        o["dy"] = round_to(rn(B, H, W, Cout), dt)
    if kind == "dgrad":
        # the BatchNorm whose output gradient dx is (fu_op_conv3x3_dgrad_bnsums reads them; dx does not depend on them)
        o["y"] = round_to(rn(B, H, W, C0), dt)
        o["bn_a"], o["bn_b"] = (torch.rand(C0, generator=g) + 0.5).numpy().astype(f32), (rn(C0) * 0.3).astype(f32)
        o["mean"], o["invstd"] = (rn(C0) * 0.1).astype(f32), (torch.rand(C0, generator=g) + 0.5).numpy().astype(f32)
    return o


def dense_operands(prec, c):
    """float32 arrays of element-type values: x0, x1, a, b, w, bias (fwd, wgrad), dy (dgrad, wgrad); shared between the
    routes that run one shape"""
    return _dense(prec, c["shape"], c["kind"], c["bn"], c["center"])


def _ints(g, shape, hi):
    """random integers in -hi..hi without 0"""
    v = torch.randint(1, hi + 1, shape, generator=g).numpy().astype(f32)
    return v * np.where(torch.rand(shape, generator=g).numpy() < 0.5, f32(-1), f32(1))


def _sparse(g, B, H, W, C, th, density, a=None):
    """sparse integers [B, H, W, C] with the planted positions, and the mask of the planted ones.  With a prologue (a; b is 0
    or -1) a planted value is 2 sign(a): a x + b >= 1 > 0, it survives the ReLU."""
    x = _ints(g, (B, H, W, C), 2) * (torch.rand(B, H, W, C, generator=g).numpy() < density)
    planted = np.zeros((B, H, W, C), bool)
    for (b, y, xx, ch) in planted_positions(B, H, W, C, th):
        planted[b, y, xx, ch] = True
        x[b, y, xx, ch] = 2.0 * (np.sign(a[ch]) if a is not None else (1.0 if (y + xx + ch) % 2 else -1.0))
    return x.astype(f32), planted


@functools.lru_cache(maxsize=4)
def _exact(shape, kind, bn, th, center):
    B, C0, C1, Cout, H, W = shape
    g = torch.Generator().manual_seed(_seed(shape, kind, bn, th, 1))
    Cin = C0 + C1
    taps = 1 if center else 9
    o = dict(a=None, b=None)
    if kind in ("fwd", "wgrad"):
        a = b = None
        if bn:
            a = np.array([1.0, -1.0, 2.0, 1.0, -2.0], f32)[np.arange(C0) % 5]
            b = np.array([0.0, -1.0, 0.0], f32)[np.arange(C0) % 3]
        x, planted = _sparse(g, B, H, W, Cin, th, min(0.02, 8.0 / (taps * Cin)), None if a is None else np.concatenate([a, np.ones(C1, f32)]))
        o.update(a=a, b=b, planted=planted)
        o["w"] = _embed(_ints(g, (Cout, Cin, 3, 3), 3) * f32(EXACT_UNIT), center)
        o["bias"] = _ints(g, (Cout,), 3) * f32(EXACT_UNIT)
        if kind == "fwd":                                    # thin the random nonzeros wherever a sum would leave the cap
            aa = None if a is None else np.concatenate([a, np.ones(C1, f32)])
            bb = None if b is None else np.concatenate([b, np.zeros(C1, f32)])
            for _ in range(8):
                z = prologue("bf16", x, aa, bb)
                over = (conv_nhwc(np.abs(z), np.abs(o["w"]), [4] if center else range(9)) + np.abs(o["bias"])).max(-1) > EXACT_CAP
                if not over.any():
                    break
                near = _pad(over[..., None].astype(f64))
                near = sum(near[:, ky:ky + H, kx:kx + W, :] for ky in range(3) for kx in range(3)) > 0
                x = np.where(near & ~planted, f32(0), x)
            else:
                raise AssertionError("the planted nonzeros alone leave the exact range")
        o["x0"], o["x1"] = np.ascontiguousarray(x[..., :C0]), (np.ascontiguousarray(x[..., C0:]) if C1 else None)
    if kind == "wgrad":
        o["dy"], o["dy_planted"] = _sparse(g, B, H, W, Cout, th, 0.02)        # dw is float32: sums below 2^24 / 8 are exact
    if kind == "dgrad":
        o["w"] = _embed(_ints(g, (Cout, Cin, 3, 3), 3) * f32(EXACT_UNIT), center)
        dy, planted = _sparse(g, B, H, W, Cout, th, min(0.02, 8.0 / (taps * Cout)))
        for _ in range(8):
            over = dgrad_nhwc(np.abs(dy), np.abs(o["w"]), [4] if center else range(9)).max(-1) > EXACT_CAP
            if not over.any():
                break
            near = _pad(over[..., None].astype(f64))
            near = sum(near[:, ky:ky + H, kx:kx + W, :] for ky in range(3) for kx in range(3)) > 0
            dy = np.where(near & ~planted, f32(0), dy)
        else:
            raise AssertionError("the planted nonzeros alone leave the exact range")
        o.update(dy=dy, planted=planted)
        gg = torch.Generator().manual_seed(5)
        o["y"] = torch.randn(B, H, W, C0, generator=gg).numpy().astype(f32)
        o["bn_a"], o["bn_b"] = np.ones(C0, f32), np.zeros(C0, f32)
        o["mean"], o["invstd"] = np.zeros(C0, f32), np.ones(C0, f32)
    return o


def exact_operands(c):
    """the sparse integer operands of the case (the same for every precision)"""
    return _exact(c["shape"], c["kind"], c["bn"], c["th"], c["center"])


def staged_input(prec, o):
    """float64 [B, H, W, C0 + C1]: source 0 through its prologue beside source 1"""
    z = prologue(prec, o["x0"], o["a"], o["b"])
    return z if o["x1"] is None else np.concatenate([z, np.asarray(o["x1"], f64)], -1)


# ---- where a wrong element sits ------------------------------------------------------------------------------------------------
def locate(c, idx, got, ref):
    """a failing element's place: image, tile, offset inside the tile, channel chunk"""
    if c["kind"] == "wgrad":
        co, ci, ky, kx = (int(i) for i in idx)
        return f"dw[c_out {co} (tile {co // 64}), c_in {ci} (chunk of 8: {ci // 8}, of 32: {ci // 32}), tap ({ky}, {kx})] got {got} ref {ref}"
    b, y, x, ch = (int(i) for i in idx)
    th = c["th"]
    return (f"image {b}, tile (row {y // th}, column {x // 16}) of {th} x 16, offset ({y % th}, {x % 16}), channel {ch} "
            f"(chunk of 8: {ch // 8}, of 32: {ch // 32}, of 64: {ch // 64}) got {got} ref {ref}")


def worst_element(got, ref, bound):
    """index of the element with the largest err / bound (any inexact element where the bound is 0 first)"""
    err = np.abs(np.asarray(got, f64) - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return np.unravel_index(int(np.argmax(ratio)), ratio.shape)
