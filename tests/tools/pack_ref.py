"""The packed 3x3 weight copies of a context and the eval-mode BatchNorm fold, stated in plain numpy / torch-CPU from the
layout comments of include/floodunet.h (fu_test_get_pack) -- not from the kernels that write them.  Everything here is
exact: the GPU tests compare bits.

  value            w[co][ci][tap] (tap = 3 ky + kx), times scale[co] in fp32 when a scale is given, +0.0 for ci >= cin_real,
                   rounded once by torch's CPU cast (round to nearest even)
  bf16 / fp16      wf[tap][co][ci_pad]    wd[8 - tap][ci_pad][co]
  fp32             wf[tap][ci_pad][co]    wd[8 - tap][co][ci_pad]
"""
import math
from fractions import Fraction

import numpy as np
import torch

PRECS = ("bf16", "fp16", "fp32")
_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
BN_EPS = np.float32(1e-5)


def _f32(t):
    return torch.as_tensor(np.asarray(t, dtype=np.float32) if not isinstance(t, torch.Tensor) else t.detach().cpu().float())


def pack_ref(w_oihw, cin_pad, prec, scale=None):
    """OIHW fp32 [cout, cin_real, 3, 3] -> (wf, wd) as raw bits: uint16 arrays for bf16 / fp16, float32 arrays for fp32, in
    the shapes of the module docstring."""
    w = _f32(w_oihw)
    cout, cin_real = w.shape[0], w.shape[1]
    assert w.shape[2:] == (3, 3) and cin_pad >= cin_real and prec in PRECS
    v = w.reshape(cout, cin_real, 9)
    if scale is not None:
        v = v * _f32(scale).reshape(cout, 1, 1)             # one fp32 multiply per element
    full = torch.zeros(cout, cin_pad, 9, dtype=torch.float32)     # +0.0 in the channel padding, whatever the scale's sign
    full[:, :cin_real] = v
    if prec == "fp32":
        wf = full.permute(2, 1, 0).contiguous().numpy()                      # [tap][ci][co]
    else:
        bits = full.to(_DTYPE[prec]).view(torch.int16).numpy().view(np.uint16)   # the one rounding
        wf = np.ascontiguousarray(bits.transpose(2, 0, 1))                   # [tap][co][ci]
    wd = np.ascontiguousarray(wf[::-1].transpose(0, 2, 1))                   # [8 - tap], the two channel axes swapped
    return wf, wd


def round_to_f32(q):
    """An exact rational -> the nearest float32, ties to even (overflow: inf).  q != 0."""
    q = Fraction(q)
    sign, q = (-1.0 if q < 0 else 1.0), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    elif Fraction(2) ** (e + 1) <= q:
        e += 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)            # spacing of float32 in this binade (subnormals: 2^-149)
    n = q / quantum
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    val = fl * quantum
    if val >= Fraction(2) ** 128:
        return np.float32(sign * math.inf)
    return np.float32(sign * float(val))                    # val is a float32 value: the conversions are exact


def fma32(a, b, c):
    """float32 fma(a, b, c): a * b + c rounded once, to nearest even.  Exact rational arithmetic, no float64 detour."""
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return np.float32(np.float64(a) * np.float64(b) + np.float64(c))    # inf / NaN rules (the product is exact)
    q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if q == 0:      # the sign of an exact zero: IEEE's rule for a sum of zeros, +0 for a cancellation
        return np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    return round_to_f32(q)


def fold_ref(gamma, beta, rm, rv, bias):
    """The eval fold of one conv + BatchNorm: (scale, fold_bias), float32 arrays [C].
    invstd = float32(1 / sqrt(float64(rv) + float64(float32(1e-5)))); scale = gamma * invstd (one fp32 multiply);
    fold_bias = fma(scale, bias, beta - rm * scale) with the product and the difference each rounded in fp32 and the fma
    correctly rounded."""
    gamma, beta, rm, rv, bias = (np.asarray(_f32(t).numpy(), dtype=np.float32) for t in (gamma, beta, rm, rv, bias))
    with np.errstate(all="ignore"):
        invstd = (1.0 / np.sqrt(rv.astype(np.float64) + np.float64(BN_EPS))).astype(np.float32)
        scale = gamma * invstd
        shift = beta - rm * scale                            # numpy float32: two roundings
    assert scale.dtype == np.float32 and shift.dtype == np.float32
    fbias = np.array([fma32(s, b, t) for s, b, t in zip(scale, bias, shift)], dtype=np.float32).reshape(scale.shape)
    return scale, fbias


def center_w3_ref(w_1x1):
    """A 1x1 conv weight [cout, cin, 1, 1] as the centre tap (4) of an OIHW 3x3 one, zeros elsewhere."""
    w = _f32(w_1x1)
    w3 = torch.zeros(w.shape[0], w.shape[1], 3, 3, dtype=torch.float32)
    w3[:, :, 1, 1] = w.reshape(w.shape[0], w.shape[1])
    return w3


def convT_w3_ref(w, b):
    """ConvTranspose2d(cin, cout, 2, 2) weight [cin][cout][2][2] and bias [cout] -> the embedded 1x1 conv to 4 cout
    phase-major channels: w3[(p * cout + co)][ci][centre] = w[ci][co][ky][kx] with p = 2 ky + kx, zeros on the other
    taps; bias4[(p, co)] = b[co]."""
    w, b = _f32(w), _f32(b)
    cin, cout = w.shape[0], w.shape[1]
    w3 = torch.zeros(4 * cout, cin, 3, 3, dtype=torch.float32)
    for ky in range(2):
        for kx in range(2):
            p = 2 * ky + kx
            w3[p * cout:(p + 1) * cout, :, 1, 1] = w[:, :, ky, kx].t()
    return w3, b.repeat(4)


def is_nan_bits(x, prec):
    x = np.asarray(x)
    if prec == "fp32":
        return np.isnan(x)
    exp, man = (0x7F80, 0x007F) if prec == "bf16" else (0x7C00, 0x03FF)
    return ((x & exp) == exp) & ((x & man) != 0)


def mismatches(got, want, prec):
    """Indices (flat) at which two arrays of raw values -- float32, or the uint16 codes of bf16 / fp16 -- differ in their
    bits; a NaN matches a NaN whatever its payload, nothing else is forgiven (+0.0 and -0.0 differ)."""
    got, want = np.asarray(got), np.asarray(want)
    dt = np.float32 if prec == "fp32" else np.uint16
    assert got.dtype == want.dtype == dt and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    gi, wi = (got.view(np.uint32), want.view(np.uint32)) if prec == "fp32" else (got, want)
    return np.flatnonzero(~((gi == wi) | (is_nan_bits(got, prec) & is_nan_bits(want, prec))))
