"""fp64 restatement of the decoder's resampling: bilinear x2 with align_corners=True followed by F.pad, and its adjoint.

The interpolation weights are formed in float32 exactly as ATen forms them (area_pixel_compute_scale<float> and
compute_source_index_and_lambda, the expressions build_axis in fu_plan.hip cites); everything after that is float64.  A pure
float64 reference is about 1e-5 away at these sizes: a kernel within that distance of it could still carry a wrong weight.
tests/test_resample_ref_cpu.py pins this file to torch on the CPU.

Tensors are numpy arrays in NCHW.  Each function returns (ref, mag): mag is the same product on the absolute values of
its input, i.e. sum_taps |weight * value| per output element, the scale every rounding-error bound is stated in.
"""
import numpy as np

f32 = np.float32


def axis_taps(n):
    """Per output index o of a 2n-long axis: (i0, i1, l0, l1) with the weights as float32, as ATen computes them."""
    out = 2 * n
    scale = f32(n - 1) / f32(out - 1) if out > 1 else f32(0)
    o = np.arange(out)
    src = (scale * o.astype(f32)).astype(f32)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n - 1)
    l1 = np.clip((src - i0.astype(f32)).astype(f32), f32(0), f32(1))
    l0 = (f32(1) - l1).astype(f32)
    return i0, i1, l0, l1


def axis_matrix(n, swap=False):
    """float64 [2n, n] interpolation matrix of one axis.  swap=True exchanges l1 and 1 - l1 (a deliberately wrong
    reference for negative controls)."""
    i0, i1, l0, l1 = axis_taps(n)
    if swap:
        l0, l1 = l1, l0
    m = np.zeros((2 * n, n), np.float64)
    o = np.arange(2 * n)
    np.add.at(m, (o, i0), l0.astype(np.float64))
    np.add.at(m, (o, i1), l1.astype(np.float64))
    return m


def pad_offsets(H, W, outH, outW):
    """top / left offset of the 2H x 2W window inside outH x outW (F.pad([dx // 2, dx - dx // 2, dy // 2, dy - dy // 2]))"""
    assert outH >= 2 * H and outW >= 2 * W
    return (outH - 2 * H) // 2, (outW - 2 * W) // 2


def upsample_ref(z, outH, outW, px0=None, swap=False):
    """ref = pad(My . z . Mx^T) for z [B,C,H,W] -> [B,C,outH,outW], zeros in the pad.  px0 / swap build wrong references."""
    z = np.asarray(z, np.float64)
    B, C, H, W = z.shape
    py0, px0_ = pad_offsets(H, W, outH, outW)
    px0 = px0_ if px0 is None else px0
    assert 0 <= px0 and px0 + 2 * W <= outW
    my, mx = axis_matrix(H, swap), axis_matrix(W, swap)
    outs = []
    for v in (z, np.abs(z)):
        full = np.zeros((B, C, outH, outW), np.float64)
        full[:, :, py0:py0 + 2 * H, px0:px0 + 2 * W] = np.einsum("oh,bchw,pw->bcop", my, v, mx, optimize=True)
        outs.append(full)
    return outs[0], outs[1]


def upsample_bwd_ref(g, H, W, px0=None, swap=False):
    """ref = My^T . crop(g) . Mx for g [B,C,outH,outW] -> [B,C,H,W]; whatever g carries in the pad is dropped."""
    g = np.asarray(g, np.float64)
    outH, outW = g.shape[2:]
    py0, px0_ = pad_offsets(H, W, outH, outW)
    px0 = px0_ if px0 is None else px0
    assert 0 <= px0 and px0 + 2 * W <= outW
    my, mx = axis_matrix(H, swap), axis_matrix(W, swap)
    crop = g[:, :, py0:py0 + 2 * H, px0:px0 + 2 * W]
    return tuple(np.einsum("oh,bcop,pw->bchw", my, v, mx, optimize=True) for v in (crop, np.abs(crop)))


U32 = 2.0 ** -24                 # unit roundoff of float32


def store_rounding(ref, mag, eps, tiny):
    """One round-to-nearest store of a value ~ref to a 16-bit type: eps |ref| in the normal range, tiny below it (half the
    spacing of the subnormals: the error is absolute there).  Nothing where mag == 0: the float32 result is an exact zero."""
    return np.where(mag > 0, np.maximum(eps * np.abs(ref), tiny), 0.0)


def fwd_bound(ref, mag, eps=0.0, tiny=0.0):
    """Elementwise bound of the forward kernel: 2^-21 mag (+ one store rounding to a 16-bit type)."""
    return 8 * U32 * mag + store_rounding(ref, mag, eps, tiny)


def bwd_bound(ref, mag, eps=0.0, tiny=0.0):
    """Elementwise bound of the backward kernel: 2^-19 mag (+ one store rounding to a 16-bit type)."""
    return 32 * U32 * mag + store_rounding(ref, mag, eps, tiny)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements; inf if got is not finite or differs where the bound is 0 (the pad, an
    all-zero window: exact).  A kernel passes with a ratio <= 1."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    if (err[bound == 0] != 0).any():
        return float("inf")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# one table for the CPU pin of this file and for the GPU tests of the kernels: (B, C, H, W, outH, outW)
SHAPES = [
    (2, 8, 16, 16, 32, 32),      # no pad
    (1, 16, 4, 5, 9, 11),        # bottom / right pad of 1
    (2, 8, 1, 2, 2, 5),          # H = 1: scale_y = 0, both taps on one source row (merged weights in the backward tables)
    (1, 8, 7, 9, 17, 21),        # difference 3: py0 = px0 = 1, two pad rows / columns after
    (1, 64, 18, 18, 37, 37),     # many channel vectors per row
    (16, 64, 63, 32, 127, 65),   # four rows per thread (2560 workgroups): outH % 4 == 3, pad row and column
    (16, 64, 32, 32, 66, 64),    # py0 = 1, outH % 4 == 2 over many workgroups -- 4 x 17 x 16 = 1088: still one row per thread
    (32, 64, 32, 32, 66, 64),    # the same at twice the batch: 2176 workgroups, four rows per thread with py0 = 1
]
# the rows that must run k_upsample2<T, 4> (launch_upsample2: from 2048 workgroups of that variant on)
ROWS4 = (SHAPES[5], SHAPES[7])
# the rows whose channel count the 16-bit runs double (8 channels per vector instead of 4): the same workgroup counts
MANY_WORKGROUPS = (SHAPES[5], SHAPES[6], SHAPES[7])


def rows4_workgroups(shape, vec):
    """workgroups launch_upsample2 counts for its four-rows-per-thread variant; vec = channels per 16-byte vector"""
    B, C, H, W, outH, outW = shape
    return -(-outW * (C // vec) // 256) * -(-outH // 4) * B
