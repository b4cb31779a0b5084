"""The layout, gather and channel-copy operations of fu_layout.hip, stated in plain numpy from what the kernels are
documented to mean (the comments of fu_layout.hip, view_src_pixel in fu_common.h, the hooks' comments in
include/floodunet.h) -- whole-array index arithmetic, not their loops.  Everything here is exact: the GPU tests compare bits.

  bits              an array of raw codes: uint32 for fp32, uint16 for bf16 / fp16
  to_bits           float32 -> the element type, by an explicit round-to-nearest-even on the integer bits (pinned to torch's
                    CPU casts by tests/test_layout_ref_cpu.py)
  from_bits         the element type -> float32 (exact)
  NCHW -> NHWC      dst[b, y, x, c] = src[b, off + c, y, x] for c < C, +0.0 for C <= c < c_pad
  NHWC -> NCHW      dst[b, c, y, x] = src[b, y, x, c] for c < C; the padding channels are not read
  gather            the same as NCHW -> NHWC on the sources concatenated along the channel axis
  views             destination sample v * B + b is view codes[v] of sample b; a code is a bit set, 1 = flip(-1), 2 = flip(-2),
                    4 = transpose, applied in the order transpose, flip(-1), flip(-2)
  copy_channels     dst[p, dst_off + c] = src[p, src_off + c] for c < C, as it is or as relu(a[c] * x + b[c]): the product and
                    the sum each rounded in float32 (bn_act: two roundings, no fma), then one rounding to the element type.
                    The ReLU is C's fmaxf(x, 0): a NaN gives 0, and so does a zero of either sign (as +0.0).
  centre tap        w3[i, 4] = w[i], +0.0 on the other eight taps; and back, dw[i] = dw3[i, 4]
"""
import numpy as np

from .pack_ref import PRECS, is_nan_bits, mismatches   # noqa: F401  (the bit comparison of the pack tests)

f32 = np.float32
VEC = {"fp32": 4, "bf16": 8, "fp16": 8}                   # elements per 16-byte vector
BITS_DTYPE = {"fp32": np.uint32, "bf16": np.uint16, "fp16": np.uint16}

# exact ties: bf16 keeps 8 significant bits, fp16 11; the even neighbour is below for 1 + u/2 and above for 1 + 3u/2
# (the list of tests/test_gpu_weight_pack.py, with the infinities and the NaN its NaN layer adds)
EDGES = [0.0, -0.0,
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),            # bf16 ties, both directions
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11),        # fp16 ties
         2.0 ** -14 * (1 + 2.0 ** -11),                                                    # fp16: tie at the smallest normal
         3.3e-6, -2.0 ** -24 * 2.5, 2.0 ** -24 * 1.5,                                      # fp16 subnormals (inexact, and ties)
         2.0 ** -25, -(2.0 ** -26), 2.0 ** -25 * 1.0000001,                                # at, below and just above half the smallest
         65520.0, -65520.0, 70000.0, 65519.996, -1e-30,
         float("inf"), float("-inf"), float("nan")]


# ----------------------------------------------------------------------------------------------------------------------
# number formats
# ----------------------------------------------------------------------------------------------------------------------
def _bf16_bits(u):
    """uint32 float32 codes -> uint16 bf16 codes: keep the top 16 bits, round the rest to nearest, ties to even"""
    u = u.astype(np.uint64)
    keep, rest = u >> 16, u & 0xFFFF
    up = (rest > 0x8000) | ((rest == 0x8000) & ((keep & 1) == 1))
    out = keep + up                                         # a carry runs into the exponent: the next binade, or infinity
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (keep & 0x8000) | 0x7FC0, out).astype(np.uint16)


def _fp16_bits(u):
    """uint32 float32 codes -> uint16 IEEE fp16 codes, round to nearest even with gradual underflow"""
    u = u.astype(np.uint64)
    sign = (u >> 16) & 0x8000
    mag = u & 0x7FFFFFFF
    exp = (mag >> 23).astype(np.int64) - 127                # unbiased float32 exponent
    man = (mag & 0x7FFFFF) | 0x800000                       # 24 significant bits (float32 subnormals end as 0 either way)
    # the result in units of the fp16 code's last place: normal range 2^(exp - 10), subnormal range 2^-24
    shift = np.where(exp >= -14, 13, np.minimum(-1 - exp, 25)).astype(np.uint64)
    keep = man >> shift
    rest = man & ((np.uint64(1) << shift) - np.uint64(1))
    half = np.uint64(1) << (shift - np.uint64(1))
    keep = keep + ((rest > half) | ((rest == half) & ((keep & 1) == 1)))
    # normal: keep has the implicit one at bit 10, so (exp + 14) << 10 plus keep is the code (a carry moves the exponent up);
    # subnormal: keep is the code (a carry to 0x400 is the smallest normal)
    code = np.where(exp >= -14, ((np.maximum(exp, -14) + 14).astype(np.uint64) << np.uint64(10)) + keep, keep)
    code = np.where(code >= 0x7C00, 0x7C00, code)           # overflow (65520 and above) and infinity
    code = np.where(mag > 0x7F800000, 0x7E00, code)         # NaN
    return (sign | code).astype(np.uint16)


def to_bits(x, prec):
    """float32 values -> the raw codes of `prec`"""
    assert prec in PRECS
    x = np.ascontiguousarray(x, dtype=f32)
    u = x.view(np.uint32)
    return u.copy() if prec == "fp32" else (_bf16_bits(u) if prec == "bf16" else _fp16_bits(u))


def from_bits(bits, prec):
    """the raw codes of `prec` -> float32 values (every bf16 / fp16 value is a float32 value)"""
    bits = np.ascontiguousarray(bits, dtype=BITS_DTYPE[prec])
    if prec == "fp32":
        return bits.view(f32).copy()
    if prec == "bf16":
        return (bits.astype(np.uint32) << 16).view(f32)
    return bits.view(np.float16).astype(f32)


# ----------------------------------------------------------------------------------------------------------------------
# NCHW <-> NHWC, gathers, views
# ----------------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc(x, C, c_pad, prec, ch_off=0):
    """x float32 [B, srcC, H, W] -> bits [B, H, W, c_pad]: channels [ch_off, ch_off + C), +0.0 above them"""
    x = np.asarray(x, dtype=f32)
    B, srcC, H, W = x.shape
    assert 0 <= ch_off and ch_off + C <= srcC and C <= c_pad
    out = np.zeros((B, H, W, c_pad), f32)
    out[..., :C] = np.moveaxis(x[:, ch_off:ch_off + C], 1, -1)
    return to_bits(out, prec)


def nhwc_to_nchw(bits, C, prec):
    """bits [B, H, W, c_pad] -> float32 codes (uint32) [B, C, H, W]"""
    v = from_bits(bits, prec)
    return to_bits(np.moveaxis(v[..., :C], -1, 1), "fp32")


def view_of(x, code):
    """view `code` of images [..., H, W]: transpose, then flip(-1), then flip(-2)"""
    assert 0 <= code <= 7
    if code & 4:
        assert x.shape[-1] == x.shape[-2], "a transposing view needs a square image"
        x = np.swapaxes(x, -1, -2)
    if code & 1:
        x = x[..., ::-1]
    if code & 2:
        x = x[..., ::-1, :]
    return x


def gather(srcs, C, c_pad, prec, ch_off=0, codes=None):
    """srcs: float32 [B, c_k, H, W] arrays side by side along the channel axis -> bits [B, H, W, c_pad], or with view
    codes [len(codes) * B, H, W, c_pad], view-major"""
    cat = np.concatenate([np.asarray(s, dtype=f32) for s in srcs], axis=1)
    if codes is not None:
        cat = np.concatenate([view_of(cat, c) for c in codes], axis=0)
    return nchw_to_nhwc(cat, C, c_pad, prec, ch_off)


# ----------------------------------------------------------------------------------------------------------------------
# channel-window copy, centre tap
# ----------------------------------------------------------------------------------------------------------------------
def copy_channels(src_bits, src_off, dst_bits, dst_off, C, prec, a=None, b=None):
    """src_bits [npix, srcC], dst_bits [npix, dstC] (what the destination held before) -> what it holds after"""
    src_bits, out = np.asarray(src_bits), np.array(dst_bits, copy=True)
    assert src_bits.dtype == out.dtype == BITS_DTYPE[prec] and src_bits.shape[0] == out.shape[0]
    assert 0 <= src_off and src_off + C <= src_bits.shape[1] and 0 <= dst_off and dst_off + C <= out.shape[1]
    win = src_bits[:, src_off:src_off + C]
    if a is not None:
        a, b = np.asarray(a, dtype=f32).reshape(1, C), np.asarray(b, dtype=f32).reshape(1, C)
        with np.errstate(all="ignore"):
            prod = from_bits(win, prec) * a                 # float32 product, rounded ...
            pre = prod + b                                  # ... then a float32 sum: two roundings
        assert prod.dtype == f32 and pre.dtype == f32
        win = to_bits(np.where(pre > 0, pre, f32(0.0)), prec)
    out[:, dst_off:dst_off + C] = win
    return out


def center_to_w3(w):
    """w float32 [n] -> float32 codes (uint32) [n, 9]"""
    w = np.asarray(w, dtype=f32).reshape(-1)
    w3 = np.zeros((w.size, 9), f32)
    w3[:, 4] = w
    return to_bits(w3, "fp32")


def center_from_w3(dw3):
    """dw3 float32 [n * 9] -> float32 codes (uint32) [n]"""
    return to_bits(np.asarray(dw3, dtype=f32).reshape(-1, 9)[:, 4], "fp32")


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def edge_input(shape, seed, edges=EDGES):
    """float32 normal values of `shape` with `edges` (as many as fit) written at seeded, distinct places"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(f32)
    flat = x.reshape(-1)
    vals = np.asarray(edges, dtype=f32)[: flat.size]
    flat[rng.choice(flat.size, vals.size, replace=False)] = vals
    return x
