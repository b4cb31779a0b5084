"""GPU: the decoder's resampling kernels on their own, through the fu_op_* test hooks, elementwise against the fp64 restatement
of tests/tools/resample_ref.py (pinned to ATen by tests/test_resample_ref_cpu.py) -- never against the code under test.

  k_upsample2<T, 1> / <T, 4>   fu_op_upsample2       bilinear x2 (align_corners) of z or relu(a*z+b), F.pad to outH x outW
  k_upsample2_bwd<T>           fu_op_upsample2_bwd   its adjoint: crop the pad, gather through the host-built tap tables
  k_depth_to_space<T>          fu_op_depth_to_space  ConvTranspose2d(k=2, s=2) phase interleave + F.pad   (pure copy)
  k_space_to_depth<T>          fu_op_space_to_depth  its adjoint, the pad dropped                         (pure copy)

BOUNDS (u = 2^-24, the unit roundoff of float32; mag = sum over the taps of |weight * value|, the same product as the
reference on absolute values).  They are derived, not tuned; the measured worst err / bound is written next to each.

* The reference has the kernel's own float32 weights: l1 = clamp(scale * o - i0) and 1 - l1 are formed by the same float32
  expressions in the forward kernel, in the host tables of the backward (build_axis) and in axis_taps(), so no weight error
  enters -- which is what lets the bounds be a few u.  A kernel with another weight (an fp64 lambda, a fused scale * o - i0)
  is ~1e-5 mag away and fails.
* Forward, fp32: out = wy0 * (wx0 * p00 + wx1 * p01) + wy1 * (wx0 * p10 + wx1 * p11), 4 taps.  The weights carry one
  rounding each (1 - l1; the reference has the same one), and a tap reaches the result through an inner and an outer
  multiply-add chain of at most 3 roundings (two products and an add; 2 where the compiler contracts), each relative to a
  partial sum that is <= mag in absolute value: <= 6 u mag (1 + O(u)) < 8 u mag = 2^-21 mag.
* Backward, fp32: one input pixel gathers at most 4 output rows x 4 output columns (no column of axis_matrix(n) has more than
  4 non-zeros, test_resample_ref_cpu.py), i.e. <= 16 taps.  Per tap: one rounding of w = wy * xw, at most one in a merged
  table weight ((1 - l1) + l1 where both taps of an output index fall on the same input index), two for the accumulate
  (product and add; one when contracted).  The accumulate roundings are relative to partial sums <= mag, the weight
  roundings to their own tap: (16 + 3) u mag < 32 u mag = 2^-19 mag.
* 16-bit: the inputs are rounded to the element type first (what the kernel loads), the arithmetic is the same float32
  arithmetic, and the result is rounded once on the store: + eps |ref| with the suite's eps (bf16 2^-8, fp16 2^-11), the unit
  roundoff of the type.  That term is relative only in the type's normal range: fp16 underflows gradually below 2^-14
  = 6.1e-5, where round-to-nearest errs by up to half the subnormal spacing, 2^-25 absolute.  relu(a*z+b) next to zeros
  produces such results by the thousand (ref = mag ~ 1e-6: both other terms are ~1e-9), so the fp16 store term is
  max(eps |ref|, 2^-25) -- the two agree at 2^-14, so nothing widens in the normal range, and a store that flushed
  subnormals to zero instead of rounding them (up to 6.1e-5 off) still fails.  bf16 has float32's exponent range: no such
  term.  The BatchNorm+ReLU prologue is reproduced in float32 as relu(x * a + b) with a separate multiply and add, as bn_act
  does (fu_common.h), so the reference interpolates the kernel's own z, bit for bit.

MEASURED worst err / bound over the shape table (MI355X; a pass is <= 1):
  forward   fp32 0.416   bf16 0.996   fp16 1.000 (0.9995+: an exact half-way case of the subnormal grid)
  backward  fp32 0.152   bf16 0.995   fp16 0.994
  adjoint   |diff| / tol: fp32 0.000, bf16 0.021, fp16 0.010
The fp32 figures are the kernels' arithmetic: 3.3 u mag forward, 4.9 u mag backward.  The 16-bit figures sit at 1 by
construction: eps is the type's unit roundoff and round-to-nearest reaches it; the float32 part underneath is the fp32 row.
The fp16 forward under a purely relative store term (eps |ref|, no subnormal term), same run: 0.78 - 1.00 on the rows without
prologue up to 37 x 37, 1.09 / 2.05 on (16,128,63,32,127,65) / (32,128,32,32,66,64) without prologue, and with the prologue
85.1 on (2,8,16,16,32,32), 151.6 on (1,64,18,18,37,37), 542.2 on (16,128,32,32,66,64), 2046.0 on the two four-row shapes
(= 1 / (2^-11 + 2^-21): a result below 2^-25 stored as 0) -- all of them results below 2^-14, all within 2^-25 absolute.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from tools.resample_ref import (MANY_WORKGROUPS, ROWS4, SHAPES, bwd_bound, fwd_bound, pad_offsets, rows4_workgroups,   # noqa: E402
                                upsample_bwd_ref, upsample_ref, worst_ratio)

from floodplanet_code_amd import _lib   # noqa: E402
from floodplanet_code_amd._lib import check, ptr   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32

# vec = channels per 16-byte vector of the row kernels; eps = the element type's rounding unit as the suite uses it
# tiny = half the spacing of the type's subnormals where a result of these tests can land there (fp16: below 2^-14)
PREC = {"fp32": dict(code=_lib.FU_F32, dt=torch.float32, eps=0.0, tiny=0.0, vec=4),
        "bf16": dict(code=_lib.FU_BF16, dt=torch.bfloat16, eps=2.0 ** -8, tiny=0.0, vec=8),
        "fp16": dict(code=_lib.FU_F16, dt=torch.float16, eps=2.0 ** -11, tiny=2.0 ** -25, vec=8)}
PAD3 = SHAPES[3]        # (1, 8, 7, 9, 17, 21): py0 = px0 = 1 and two pad rows / columns behind the window


@pytest.fixture(params=list(PREC))
def prec(request):
    return PREC[request.param]


def shape_for(shape, P):
    """The 16-bit types carry 8 channels per vector: twice the channels on the table's MANY_WORKGROUPS rows keeps their
    workgroup count."""
    B, C, H, W, oh, ow = shape
    return (B, 2 * C if P["vec"] == 8 and shape in MANY_WORKGROUPS else C, H, W, oh, ow)


def stream():
    return torch.cuda.current_stream().cuda_stream


def rounded(x, P):
    """float32 NCHW values that the element type holds exactly"""
    return x.to(P["dt"]).float()


def to_dev(x, P):       # float32 NCHW (cpu, already rounded) -> device NHWC of the element type
    return x.permute(0, 2, 3, 1).contiguous().to(P["dt"]).to(DEV)


def to_np(t):           # device NHWC -> float32 NCHW numpy
    return t.float().permute(0, 3, 1, 2).contiguous().cpu().numpy()


def pad_mask(H, W, oh, ow):
    py0, px0 = pad_offsets(H, W, oh, ow)
    m = np.ones((oh, ow), bool)
    m[py0:py0 + 2 * H, px0:px0 + 2 * W] = False
    return m


def run_fwd(P, x, a, b, shape):
    B, C, H, W, oh, ow = shape
    lib = _lib.load()
    dx = to_dev(x, P)
    da, db = (None, None) if a is None else (torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    out = torch.full((B, oh, ow, C), float("nan"), device=DEV, dtype=P["dt"])
    check(lib.fu_op_upsample2(P["code"], ptr(dx), ptr(da), ptr(db), ptr(out), B, H, W, C, oh, ow, stream()))
    torch.cuda.synchronize()
    return out


def run_bwd(P, g, shape):
    B, C, H, W, oh, ow = shape
    lib = _lib.load()
    dg = to_dev(g, P)
    gsrc = torch.full((B, H, W, C), float("nan"), device=DEV, dtype=P["dt"])
    check(lib.fu_op_upsample2_bwd(P["code"], ptr(dg), ptr(gsrc), B, H, W, C, oh, ow, stream()))
    torch.cuda.synchronize()
    return gsrc


def make_z(P, shape, bn, seed):
    """(x, a, b, z): x rounded to the element type; z = what the kernel interpolates, formed in float32 as bn_act forms it"""
    B, C, H, W, _, _ = shape
    g = torch.Generator().manual_seed(seed)
    x = rounded(torch.randn(B, C, H, W, generator=g), P)
    if not bn:
        return x, None, None, x.numpy()
    a = (torch.rand(C, generator=g) + 0.5).numpy()
    b = (torch.randn(C, generator=g) * 0.3).numpy()
    prod = x.numpy() * a[None, :, None, None]                     # float32 product, rounded ...
    z = np.maximum(prod + b[None, :, None, None], f32(0))         # ... then a float32 add: two roundings, no fma
    assert z.dtype == np.float32
    return x, a, b, z


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bnrelu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_forward(shape, bn, prec):
    """k_upsample2<T, 1> on the rows below 2048 workgroups, k_upsample2<T, 4> on ROWS4 (with its tail and its per-row masks)."""
    P = prec
    four_rows = shape in ROWS4
    shape = shape_for(shape, P)
    B, C, H, W, oh, ow = shape
    if four_rows:   # if the dispatch threshold of launch_upsample2 moves, say that this case no longer reaches the variant
        assert rows4_workgroups(shape, P["vec"]) >= 2048
    x, a, b, z = make_z(P, shape, bn, seed=21)
    got = to_np(run_fwd(P, x, a, b, shape))
    assert np.isfinite(got).all()                                  # the NaN prefill is gone everywhere
    assert (got[:, :, pad_mask(H, W, oh, ow)] == 0).all()          # the pad is exactly zero
    ref, mag = upsample_ref(z, oh, ow)
    r = worst_ratio(got, ref, fwd_bound(ref, mag, P["eps"], P["tiny"]))
    print(f"MEASURED fwd {P['dt']} {shape} bn={bn}: err/bound {r:.3f}")
    if P["tiny"]:   # the same elements under a purely relative store term, eps |ref|: what gradual underflow does to it
        r0 = worst_ratio(got, ref, fwd_bound(ref, mag, P["eps"]))
        print(f"MEASURED fwd {P['dt']} {shape} bn={bn}: without the subnormal term {r0:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_backward(shape, prec):
    """k_upsample2_bwd<T>: one input row per workgroup row, gather lists with merged weights (H = 1), py0 / px0 > 0."""
    P = prec
    shape = shape_for(shape, P)
    B, C, H, W, oh, ow = shape
    gen = torch.Generator().manual_seed(22)
    g = rounded(torch.randn(B, C, oh, ow, generator=gen), P)      # non-zero in the pad as well
    out = run_bwd(P, g, shape)
    got = to_np(out)
    ref, mag = upsample_bwd_ref(g.numpy(), H, W)
    r = worst_ratio(got, ref, bwd_bound(ref, mag, P["eps"], P["tiny"]))
    print(f"MEASURED bwd {P['dt']} {shape}: err/bound {r:.3f}")
    assert r <= 1.0
    # what g_dst carries in the pad does not reach g_src: other values there, the same bits out
    pad = torch.from_numpy(pad_mask(H, W, oh, ow))
    if bool(pad.any()):
        g2 = g.clone()
        g2[:, :, pad] = rounded(torch.full((int(pad.sum()),), 1e4), P)
        assert torch.equal(run_bwd(P, g2, shape), out)


def test_wrong_references_fail_the_same_check(prec):
    """Negative control: the bound check of the two tests above, on the kernels' outputs, passes against the restatement and
    fails against one with px0 off by one and against one with l1 and 1 - l1 exchanged."""
    P = prec
    B, C, H, W, oh, ow = PAD3
    x, _, _, z = make_z(P, PAD3, False, seed=23)
    gen = torch.Generator().manual_seed(24)
    g = rounded(torch.randn(B, C, oh, ow, generator=gen), P)
    y, gx = to_np(run_fwd(P, x, None, None, PAD3)), to_np(run_bwd(P, g, PAD3))

    def fwd_ok(**kw):
        ref, mag = upsample_ref(z, oh, ow, **kw)
        return worst_ratio(y, ref, fwd_bound(ref, mag, P["eps"], P["tiny"])) <= 1.0

    def bwd_ok(**kw):
        ref, mag = upsample_bwd_ref(g.numpy(), H, W, **kw)
        return worst_ratio(gx, ref, bwd_bound(ref, mag, P["eps"], P["tiny"])) <= 1.0

    assert fwd_ok() and bwd_ok()
    assert pad_offsets(H, W, oh, ow)[1] == 1
    assert not fwd_ok(px0=2) and not bwd_ok(px0=2)
    assert not fwd_ok(swap=True) and not bwd_ok(swap=True)


def test_forward_and_backward_are_adjoint(prec):
    """<up(x), g> == <x, up_bwd(g)> on the kernels' own outputs, summed in fp64: the two kernels apply one matrix and its
    transpose (device-evaluated weights forward, host tables backward).  Nothing of the restatement enters the two sides; it
    supplies only the magnitudes of the tolerance, sum |g| fwd_bound + sum |x| bwd_bound."""
    P = prec
    B, C, H, W, oh, ow = PAD3
    x, _, _, z = make_z(P, PAD3, False, seed=25)
    gen = torch.Generator().manual_seed(26)
    g = rounded(torch.randn(B, C, oh, ow, generator=gen), P)
    y = to_np(run_fwd(P, x, None, None, PAD3)).astype(np.float64)
    gx = to_np(run_bwd(P, g, PAD3)).astype(np.float64)
    gn, xn = g.numpy().astype(np.float64), x.numpy().astype(np.float64)
    lhs, rhs = float((y * gn).sum()), float((xn * gx).sum())
    fref, fmag = upsample_ref(z, oh, ow)
    bref, bmag = upsample_bwd_ref(gn, H, W)
    tol = float((np.abs(gn) * fwd_bound(fref, fmag, P["eps"], P["tiny"])).sum()
                + (np.abs(xn) * bwd_bound(bref, bmag, P["eps"], P["tiny"])).sum())
    print(f"MEASURED adjoint {P['dt']}: <up x, g> = {lhs:.9g}  <x, up^T g> = {rhs:.9g}  "
          f"|diff| / tol = {abs(lhs - rhs) / tol:.3f}")
    assert abs(lhs) > 1.0                                          # not a vacuous pair of sums
    assert abs(lhs - rhs) <= tol


# ---- the two shuffles of ConvTranspose2d(k=2, s=2): pure copies, so bit equality with torch indexing ------------------------
SHUFFLE_SHAPES = [(2, 8, 5, 6, 10, 12),      # B, C, h, w, outH, outW: no pad
                  (1, 16, 17, 20, 35, 41),   # bottom / right pad of 1, more than one workgroup
                  (2, 8, 3, 3, 9, 8)]        # py0 = px0 = 1, two pad rows behind the window, one column


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def phases(C, h, w, py0, px0):
    """(channel slice of the 4C-channel map, row slice, column slice of the padded map) of the four phases p = 2 ky + kx"""
    for ky in (0, 1):
        for kx in (0, 1):
            p = 2 * ky + kx
            yield slice(p * C, (p + 1) * C), slice(py0 + ky, py0 + 2 * h, 2), slice(px0 + kx, px0 + 2 * w, 2)


@pytest.mark.parametrize("shape", SHUFFLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_convtranspose_shuffles_are_exact_copies(shape, prec):
    P = prec
    dt = P["dt"]
    B, C, h, w, oh, ow = shape
    lib = _lib.load()
    py0, px0 = pad_offsets(h, w, oh, ow)
    gen = torch.Generator().manual_seed(27)
    fi = torch.finfo(dt)
    y4 = torch.randn(B, h, w, 4 * C, generator=gen).to(dt)
    # values a copy must not touch: the sign of zero, the smallest subnormal, the largest finite, the smallest normal
    y4.view(-1)[:4] = torch.tensor([-0.0, fi.tiny * fi.eps, fi.max, -fi.tiny], dtype=torch.float64).to(dt)
    want_up = torch.zeros(B, oh, ow, C, dtype=dt)
    for cs, rs, xs in phases(C, h, w, py0, px0):
        want_up[:, rs, xs, :] = y4[..., cs]
    dy4 = y4.to(DEV)
    up = torch.full((B, oh, ow, C), float("nan"), device=DEV, dtype=dt)
    check(lib.fu_op_depth_to_space(P["code"], ptr(dy4), ptr(up), B, h, w, C, oh, ow, stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(up.cpu()), bits(want_up))              # the window bit for bit, the pad +0 from a NaN prefill

    # the adjoint: the pad of the incoming gradient is dropped -- it carries NaN here, the result must not
    gup = torch.randn(B, oh, ow, C, generator=gen).to(dt)
    want_g4 = torch.empty(B, h, w, 4 * C, dtype=dt)
    for cs, rs, xs in phases(C, h, w, py0, px0):
        want_g4[..., cs] = gup[:, rs, xs, :]
    gup.permute(0, 3, 1, 2)[:, :, torch.from_numpy(pad_mask(h, w, oh, ow))] = float("nan")
    dgup = gup.to(DEV)
    g4 = torch.full((B, h, w, 4 * C), float("nan"), device=DEV, dtype=dt)
    check(lib.fu_op_space_to_depth(P["code"], ptr(dgup), ptr(g4), B, h, w, C, oh, ow, stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(g4.cpu()), bits(want_g4))

    back = torch.full((B, h, w, 4 * C), float("nan"), device=DEV, dtype=dt)
    check(lib.fu_op_space_to_depth(P["code"], ptr(up), ptr(back), B, h, w, C, oh, ow, stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(back.cpu()), bits(y4))                 # space_to_depth(depth_to_space(y4)) == y4
