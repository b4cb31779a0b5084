"""fp64 reference of the BatchNorm kernels (fu_bn.hip) -- forward finalisation from given partial sums, BatchNorm + ReLU backward
(plain, with the 2x2 max-pool backward folded in, with the head gradient recomputed, with the two sums supplied from outside) --
with analytic per-element bounds of the kernels' float32 evaluation, a float32 restatement of the kernels' arithmetic (for
tests/test_bn_ref_cpu.py only) and the generators of `dense` and `exact` operands.

Layout: y, g [B, H, W, C] float32 arrays holding values the element type represents exactly, g_pool [B, H/2, W/2, C], a / b /
mean / invstd [C] float32, head: dl [P, K], w [K, C] float32; external sums [rows, C, 2] float32.  Results are [P, C] / [C].

    m   = [fl(fl(a*y) + b) > 0]                 float32, two roundings: bn_act_pre's parity definition.  A DECISION, not a rounding:
                                                the reference takes it from the float32 value, numpy float32 reproduces it exactly
    gt  = g                                     plain
        = g + g_pool routed to the first maximum (row-major) of max(z, 0) in every complete 2x2 window         pooled
        = dl . w                                head
    xh  = (y - mean) * invstd                   s1 = sum_p gt*m     s2 = sum_p gt*m*xh     c1 = s1/N   c2 = s2/N
    dy  = a * (gt*m - c1 - xh*c2)               dbeta = unscale * s1     dgamma = unscale * s2     db = sum_p dy
With external sums S = sum of the supplied rows in fp64, coef's reference is S / N and the dy reference uses it ROUNDED ONCE
to float32 (what any correct finalisation hands the apply pass); nothing is recomputed from g.

BOUNDS.  u = 2^-24, gamma(n) = n u / (1 - n u): a sum of terms in any order in which no term passes through more than n
roundings is within gamma(n) * sum |terms| of the exact sum.  No fitted constant; n comes from bwd_geometry, which restates
bn_bwd_blocks and the kernels' thread layout in one place.
* xh32 = fl(fl(y - mean) * invstd): two roundings, |xh32 - xh| <= dxh = u (2 + u) |xh|.
* gt32: plain 0 (g is an operand); pooled u |gt| where a pool gradient is added (ONE rounding); head gamma(ncls) sum_k |dl||w|
  (o = 0; o += dl*w per class: ncls roundings at most, an fma saves one).  Call it dg.
* s1, s2, db: a thread adds its T terms in visiting order (T pixels, or 4 x its windows; s2 by fma: one rounding per term), the
  block adds its `rows` LDS rows in order, the finalisation adds the blocks in fp64 and rounds ONCE to float32:
  n = T + rows (T for the thread's first term, rows - 1 inexact LDS additions, the last rounding; the fp64 stage of <= 2048
  rows is < 2^-42 relative, far inside the one exact addition that n counts).
      ds1 = sum m dg + gamma(n) sum m (|gt| + dg)
      ds2 = sum m (dg (|xh| + dxh) + |gt| dxh) + gamma(n) sum m (|gt| + dg)(|xh| + dxh)
  External sums: the only error is the fp64 addition of the rows, ds = (rows + 4) 2^-53 sum |row|.
* coef = fl(S / N): dc = ds / N + u |c|.  (External sums, against the once-rounded reference: ds / N + 2 u |c| -- two roundings of
  two fp64 values ds / N apart.)
* dgamma, dbeta: unscale * ds + u |value|  (unscale is a power of two in fp64: exact).
* dy, every operation counted unfused (the expression is not under contract(off); an fma only removes a rounding):
      t1 = fl(gm - c1)    e1 = m dg + dc1 + u (|gm| + m dg + |c1| + dc1)
      t2 = fl(xh * c2)    e2 = (|xh| + dxh) dc2 + dxh |c2| + u (|xh| + dxh)(|c2| + dc2)
      t3 = fl(t1 - t2)    e3 = e1 + e2 + u (|E| + e1 + e2),  E = gm - c1 - xh c2
      dy = fl(a * t3)     e  = |a| e3 + u |a| (|E| + e3)
  then the store: e + max(eps (|dy| + e), tiny) with eps / tiny of the element type as head_ref.PREC (fp32: none).
  db takes the float32 dy BEFORE the store: bound sum e + gamma(n) sum (|dy| + e).
* forward, from partials [n_part][C][2] (S = sum, Q = sum of squares, count elements): the fp64 two-stage sums perturb
  m0 = S / count by dm = (n_part + 4) 2^-53 sum |S_t| / count and var = max(Q / count - m0^2, 0) by
  dv = (n_part + 4) 2^-53 (Q / count + m0^2); the clamp is 1-Lipschitz.  Carried per channel:
      invstd = fl((var + eps)^-1/2):  di = [(max(var - dv, 0) + eps)^-1/2 - invstd] + 4 2^-53 invstd, + u (invstd + di)
      mean   = fl(m0 + conv_bias):    dmean = dm + 2^-53 |mean|, + u (|mean| + dmean)
      a      = fl(gamma * invstd32):  da = |gamma| dinvstd + u |gamma| (invstd + dinvstd)
      b      = fl(beta - fl(mean32 * a32)), two roundings:  (|mean| + dmean) da + dmean |a| + u (|mean| + dmean)(|a| + da), + u (|b| + that)
      rmean' = fl(fl(om * rmean) + fl(mom * mean32)), three roundings; om = fl(1 - mom) in float32 is the coefficient's definition
      rvar'  = the same with fl(unbiased), unbiased = var * count / (count - 1) (count > 1)
      nbt    goes up by exactly 1 per call.
"""
import functools

import numpy as np
import torch

from .head_ref import PREC, gamma, round_to   # noqa: F401  (the element types' eps / tiny / dtype; the same gamma(n))
from .resample_ref import worst_ratio   # noqa: F401

f32 = np.float32
U32 = 2.0 ** -24
U64 = 2.0 ** -53
BNB_THREADS, BNB_MAX_BLOCKS, BNB_PIX_PER_THREAD = 256, 2048, 8      # fu_elem.h / bn_bwd_blocks

# (B, C, H, W) and the branch each is the smallest to reach
PLAIN_SHAPES = [
    (1, 8, 1, 1),        # one pixel: 127 of the block's 128 pixel rows idle
    (1, 12, 5, 7),       # C / 4 = 3 does not divide 256: thread 255 owns no pixel row (the `row < rows` guard)
    (1, 516, 2, 3),      # C / 4 = 129 > 128: one pixel row per block, 127 idle threads, the epilogue's c += 256 loop runs 3 times
    (1, 1024, 3, 3),     # the widest: one pixel row, every thread busy, 4 channels per thread in the epilogue
    (2, 64, 32, 48),     # 24 blocks, 8 pixels per thread
]
POOL_SHAPES = [
    (1, 8, 1, 1),        # no complete window: the only window has one pixel on the map and no pool output
    (1, 8, 5, 7),        # an odd edge row and column: windows with two and with one pixel on the map
    (1, 32, 37, 45),     # several blocks, odd edges, a ragged last trip over the windows
    (1, 1024, 4, 4),     # the widest pooled shape (C / 4 = 256 divides 256): one window per block
    (2, 64, 32, 48),     # 24 blocks, two windows per thread
]
HEAD_WIDTHS, HEAD_CLASSES, HEAD_NPIX = (8, 16, 64, 128), (1, 2, 3, 5, 8), (1, 35, 4099)
EXT_ROWS = (1, 3, 385, 2048)
STATS_FUSED = dict(C=(4, 8, 64, 1024), n_part=(1, 2, 127, 128, 129, 384, 385, 513, 1025))
STATS_TWO_LEVEL = dict(C=(1, 6, 33, 70), n_part=(1, 31, 32, 33, 257))
POOL2_SHAPES = ["V", (2, 8, 5, 7), (1, 64, 37, 45), (1, 64, 4, 70)]     # "V": (1, V, 2, 2), V = channels per 16-byte vector

# worst ratio of the float32 restatement against the bounds over the shapes above (tests/test_bn_ref_cpu.py prints them)
MEASURED_RESTATEMENT = {
    ("fp32", "plain"): dict(coef=0.235, db=0.104, dbeta=0.246, dgamma=0.272, dy=0.420),
    ("fp32", "pool"): dict(coef=0.161, db=0.069, dbeta=0.157, dgamma=0.161, dy=0.402),
    ("fp32", "ext"): dict(coef=0.990, db=0.167, dbeta=0.999, dgamma=1.000, dy=0.860),
    ("bf16", "plain"): dict(coef=0.232, db=0.094, dbeta=0.003, dgamma=0.259, dy=0.995),
    ("bf16", "pool"): dict(coef=0.150, db=0.044, dbeta=0.002, dgamma=0.150, dy=0.995),
    ("bf16", "head"): dict(coef=0.990, db=0.376, dbeta=0.999, dgamma=0.996, dy=0.996),
    ("bf16", "ext"): dict(coef=0.997, db=0.151, dbeta=1.000, dgamma=1.000, dy=0.995),
    ("fp16", "plain"): dict(coef=0.308, db=0.091, dbeta=0.003, dgamma=0.253, dy=0.993),
    ("fp16", "pool"): dict(coef=0.146, db=0.057, dbeta=0.002, dgamma=0.146, dy=0.995),
    ("fp16", "head"): dict(coef=0.990, db=0.376, dbeta=0.999, dgamma=0.999, dy=1.000),
    ("fp16", "ext"): dict(coef=0.993, db=0.175, dbeta=0.995, dgamma=0.998, dy=0.995),
    "forward": dict(a=0.891, b=0.837, invstd=0.996, mean=0.998, rmean=0.825, rvar=0.877),
}
# (with external sums dgamma / dbeta / coef are ONE rounding of an fp64 value against a bound of one rounding: 1 by construction;
# the 16-bit dy sits at the store rounding; the 16-bit dbeta of plain / pool is small because sums of 8- and 11-bit values are
# mostly exact in float32)
# worst ratio of the kernels against the bounds on an MI355X (tests/test_gpu_bn_ops.py prints them)
MEASURED_GPU = {
    'fp32 plain': dict(coef=0.235, db=0.104, dbeta=0.246, dgamma=0.272, dy=0.420),
    'fp32 pool': dict(coef=0.161, db=0.069, dbeta=0.157, dgamma=0.161, dy=0.402),
    'bf16 plain': dict(coef=0.232, db=0.087, dbeta=0.003, dgamma=0.259, dy=0.995),
    'bf16 pool': dict(coef=0.150, db=0.049, dbeta=0.002, dgamma=0.150, dy=0.995),
    'fp16 plain': dict(coef=0.308, db=0.092, dbeta=0.003, dgamma=0.253, dy=0.993),
    'fp16 pool': dict(coef=0.146, db=0.057, dbeta=0.002, dgamma=0.146, dy=0.995),
    'fp32 ext': dict(coef=0.990, db=0.167, dbeta=0.999, dgamma=1.000, dy=0.860),
    'bf16 ext': dict(coef=0.997, db=0.148, dbeta=1.000, dgamma=1.000, dy=0.995),
    'fp16 ext': dict(coef=0.993, db=0.152, dbeta=0.995, dgamma=0.998, dy=0.995),
    'bf16 head': dict(coef=0.990, db=0.376, dbeta=0.999, dgamma=0.996, dy=0.996),
    'fp16 head': dict(coef=0.990, db=0.376, dbeta=0.999, dgamma=0.999, dy=1.000),
    'forward fused': dict(a=0.891, b=0.913, invstd=0.996, mean=0.999, rmean=0.895, rvar=0.877),
    'forward two_level': dict(a=0.784, b=0.722, invstd=0.899, mean=0.956, rmean=0.768, rvar=0.762),
}


def _f64(*xs):
    return tuple(None if x is None else np.asarray(x, np.float64) for x in xs)


def bwd_geometry(route, C, npix, nwin=0):
    """bn_bwd_blocks and the kernels' layout: blocks, pixel rows per block, trips, terms per thread T, chain length n"""
    rows4 = BNB_THREADS // (C // 4)
    nb = max(1, min(BNB_MAX_BLOCKS, -(-npix // (rows4 * BNB_PIX_PER_THREAD))))
    rows = BNB_THREADS // (C // 8) if route == "head" else rows4          # the head apply pass: 8 channels per lane
    items = nwin if route == "pool" else npix
    trips = -(-items // (nb * rows))
    T = trips * (4 if route == "pool" else 1)
    return dict(nb=nb, rows=rows, trips=trips, T=T, n=T + rows)


# ---- 2x2 windows, odd edges included ------------------------------------------------------------------------------------------
def to_windows(x, fill=0.0):
    """[B, H, W, C] -> [B, ceil(H/2), ceil(W/2), 4, C], q = 2 * row + column inside the window; `fill` off the map"""
    B, H, W, C = x.shape
    Hw, Ww = (H + 1) // 2, (W + 1) // 2
    p = np.full((B, 2 * Hw, 2 * Ww, C), fill, x.dtype)
    p[:, :H, :W] = x
    return p.reshape(B, Hw, 2, Ww, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, Hw, Ww, 4, C)


def from_windows(xw, H, W):
    B, Hw, Ww, _, C = xw.shape
    return xw.reshape(B, Hw, Ww, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * Hw, 2 * Ww, C)[:, :H, :W]


def pre32(y, a, b):
    """the float32 pre-activation fl(fl(a*y) + b)"""
    z = (np.asarray(y, f32) * np.asarray(a, f32)).astype(f32) + np.asarray(b, f32)
    assert z.dtype == f32
    return z


def route_pool(z32, gpool, last=False, edge=False):
    """g_pool [B, Ho, Wo, C] paid to the first maximum (row-major) of max(z, 0) of every complete window -> [B, H, W, C] float64.
    last / edge: the two wrong rules of the CPU test (last of tied maxima; incomplete windows paid from their neighbour)."""
    B, H, W, C = z32.shape
    Ho, Wo = H // 2, W // 2
    zw = to_windows(np.maximum(z32, f32(0)), fill=-1.0)
    am = 3 - np.argmax(zw[:, :, :, ::-1], axis=3) if last else np.argmax(zw, axis=3)
    gp = np.zeros(zw.shape[:3] + (C,), np.float64)
    gp[:, :Ho, :Wo] = gpool
    if edge:
        gp[:, Ho:] = gp[:, Ho - 1:Ho] if Ho else 1.0
        gp[:, :, Wo:] = gp[:, :, Wo - 1:Wo] if Wo else 1.0
    routed = np.zeros(zw.shape, np.float64)
    np.put_along_axis(routed, am[:, :, :, None, :], gp[:, :, :, None, :], axis=3)
    on_map = to_windows(np.ones(z32.shape, bool), fill=False)
    return from_windows(np.where(on_map, routed, 0.0), H, W)


def store_bound(prec, ref, e):
    """e plus one rounding of a float32 value within e of ref to the element type; exact where ref and e are 0"""
    eps, tiny = PREC[prec]["eps"], PREC[prec]["tiny"]
    if eps == 0.0:
        return e
    return np.where((ref == 0) & (e == 0), 0.0, e + np.maximum(eps * (np.abs(ref) + e), tiny))


# ---- fp64 reference and bounds of the backward -------------------------------------------------------------------------------
def bwd_ref(prec, route, y, a, b, mean, invstd, g=None, gpool=None, dl=None, w=None, ext=None, unscale=1.0):
    """{name: (ref, bound)} for dy [P, C], dgamma, dbeta, db [C], coef [C, 2].  route: "plain", "pool" or "head"."""
    B, H, W, C = y.shape
    N = B * H * W
    z32 = pre32(y, a, b)
    m = (z32 > 0).reshape(N, C)
    y64, a64, mean64, inv64 = _f64(y.reshape(N, C), a, mean, invstd)
    if route == "head":
        dl64, w64 = _f64(dl, w)
        gt = dl64 @ w64
        dg = gamma(w64.shape[0]) * (np.abs(dl64) @ np.abs(w64))
    elif route == "pool":
        routed = route_pool(z32, np.asarray(gpool, np.float64))
        gt = (np.asarray(g, np.float64) + routed).reshape(N, C)
        dg = np.where(routed.reshape(N, C) != 0, U32 * np.abs(gt), 0.0)
    else:
        gt, dg = np.asarray(g, np.float64).reshape(N, C), np.zeros((N, C))
    nwin = B * ((H + 1) // 2) * ((W + 1) // 2)
    n = bwd_geometry(route, C, N, nwin)["n"]
    gm, agm, dgm = gt * m, np.abs(gt) * m, dg * m
    xh = (y64 - mean64) * inv64
    dxh = U32 * (2 + U32) * np.abs(xh)
    axh = np.abs(xh) + dxh
    if ext is None:
        S = np.stack([gm.sum(0), (gm * xh).sum(0)], 1)
        dS = np.stack([dgm.sum(0) + gamma(n) * (agm + dgm).sum(0),
                       (dgm * axh + agm * dxh).sum(0) + gamma(n) * ((agm + dgm) * axh).sum(0)], 1)
        c = S / N
        dc = dS / N + U32 * np.abs(c)
        coef = (c, dc)
    else:
        e = np.asarray(ext, np.longdouble)
        S = e.sum(0).astype(np.float64)
        dS = (e.shape[0] + 4) * U64 * np.abs(e).sum(0).astype(np.float64)
        coef = (S / N, dS / N + U32 * np.abs(S / N))
        c = (S / N).astype(f32).astype(np.float64)
        dc = dS / N + 2 * U32 * np.abs(c)
    c1, c2, dc1, dc2 = c[:, 0], c[:, 1], dc[:, 0], dc[:, 1]
    E = gm - c1 - xh * c2
    e1 = dgm + dc1 + U32 * (agm + dgm + np.abs(c1) + dc1)
    e2 = axh * dc2 + dxh * np.abs(c2) + U32 * axh * (np.abs(c2) + dc2)
    e3 = e1 + e2 + U32 * (np.abs(E) + e1 + e2)
    dy = a64 * E
    e = np.abs(a64) * e3 + U32 * np.abs(a64) * (np.abs(E) + e3)
    nd = bwd_geometry(route, C, N, nwin)["n"]
    out = {"dy": (dy, store_bound(prec, dy, e)),
           "db": (dy.sum(0), e.sum(0) + gamma(nd) * (np.abs(dy) + e).sum(0)),
           "coef": coef}
    for name, j in (("dbeta", 0), ("dgamma", 1)):
        v = S[:, j] * unscale
        out[name] = (v, dS[:, j] * unscale + U32 * np.abs(v))
    return out


def split_sums(S, rows, seed=0):
    """[rows, C, 2] float32 rows whose sum is S [C, 2] up to the rounding of the last row: how a producer leaves its sums behind"""
    rng = np.random.default_rng(seed)
    part = rng.standard_normal((rows,) + S.shape) * (np.abs(S) / max(rows, 1) ** 0.5 + 1e-3)
    part = part.astype(f32)
    part[-1] = (S - part[:-1].astype(np.float64).sum(0)).astype(f32)
    return part


# ---- float32 restatement of the backward kernels (CPU test only) ---------------------------------------------------------------
def _thread_chains(terms, nb, rows, fma_with=None):
    """terms [items, L, C] float32 -> per-thread sums [nb, rows, C]: thread (blk, row) visits item (trip * nb + blk) * rows + row
    and adds its L terms in order; fma_with: a second factor, term = fma(terms, fma_with, sum)"""
    items, L, C = terms.shape
    blk, row = np.arange(nb)[:, None], np.arange(rows)[None, :]
    s = np.zeros((nb, rows, C), f32)
    for trip in range(-(-items // (nb * rows))):
        it = (trip * nb + blk) * rows + row
        ok = (it < items)[..., None]
        it = np.where(it < items, it, 0)
        for q in range(L):
            t = np.where(ok, terms[it, q], f32(0))
            if fma_with is None:
                s = s + t
            else:
                x = np.where(ok, fma_with[it, q], f32(0))
                s = (t.astype(np.float64) * x + s).astype(f32)
    assert s.dtype == f32
    return s


def _block_rows(acc, drop_last=False):
    """the block's LDS rows in order (float32) -> [nb, C]"""
    t = np.zeros_like(acc[:, 0])
    for r in range(acc.shape[1] - (1 if drop_last else 0)):
        t = t + acc[:, r]
    assert t.dtype == f32
    return t


def restate_bwd(prec, route, y, a, b, mean, invstd, g=None, gpool=None, dl=None, w=None, ext=None, unscale=1.0, mut=None):
    """{name: float32 array} as bwd_ref, every operation of the kernels a separate float32 rounding.  mut: one deliberate defect."""
    B, H, W, C = y.shape
    N = B * H * W
    a, b, mean, invstd = (np.asarray(v, f32) for v in (a, b, mean, invstd))
    z32 = pre32(y, a, b)
    m = (z32 >= 0) if mut == "mask_ge" else (z32 > 0)
    if route == "head":
        o = np.zeros((N, C), f32)
        for k in range(w.shape[0]):
            o = o + np.asarray(dl, f32)[:, k:k + 1] * np.asarray(w, f32)[k]
        gt = o.reshape(B, H, W, C)
    elif route == "pool":
        routed = route_pool(z32, gpool, last=mut == "pool_last", edge=mut == "pool_edge").astype(f32)
        gt = np.asarray(g, f32) + routed
    else:
        gt = np.asarray(g, f32)
    gm = np.where(m, gt, f32(0))
    mean_x = np.roll(mean, 1) if mut == "neighbour_mean" else mean
    xh = (np.asarray(y, f32) - mean_x) * invstd
    assert gm.dtype == f32 and xh.dtype == f32
    if route == "pool":
        tw = lambda v: to_windows(v).reshape(-1, 4, C)     # noqa: E731
        nwin = B * ((H + 1) // 2) * ((W + 1) // 2)
    else:
        tw = lambda v: v.reshape(N, 1, C)                  # noqa: E731
        nwin = 0
    geo = bwd_geometry(route, C, N, nwin)
    nb, rows = geo["nb"], geo["rows"]
    drop = mut == "drop_last_row"
    if ext is None:
        gm1 = tw(gm).copy()
        if mut == "s1_minus_pixel":
            flat = gm1.reshape(-1, C)                       # every channel loses its largest term
            flat[np.abs(flat).argmax(0), np.arange(C)] = 0
        s1 = _block_rows(_thread_chains(gm1, nb, rows), drop).astype(np.float64).sum(0)
        s2 = _block_rows(_thread_chains(tw(gm), nb, rows, fma_with=tw(xh)), drop).astype(np.float64).sum(0)
        S = np.stack([s1, s2], 1)
    else:
        S = np.asarray(ext, np.float64).sum(0)
    coef = (S / N).astype(f32)
    if mut == "coef_unscaled":
        coef = (S / N * unscale).astype(f32)
    c1, c2 = coef[:, 0], coef[:, 1]
    dy = a * ((gm - c1) - xh * c2)
    assert dy.dtype == f32
    db = _block_rows(_thread_chains(tw(dy), nb, rows), drop).astype(np.float64).sum(0).astype(f32)
    dyo = round_to(dy.reshape(N, C), PREC[prec]["dt"])
    if mut == "swap_vectors":
        dyo = dyo.copy()
        dyo[:, 0:4], dyo[:, 4:8] = dyo[:, 4:8].copy(), dyo[:, 0:4].copy()
    return dict(dy=dyo, db=db, coef=coef, dbeta=(S[:, 0] * unscale).astype(f32), dgamma=(S[:, 1] * unscale).astype(f32))


# ---- forward finalisation --------------------------------------------------------------------------------------------------------
def stats_ref(partials, count, conv_bias, gamma, beta, eps, momentum, rmean=None, rvar=None):
    """{name: (ref, bound)} for mean, invstd, a, b and, with rmean / rvar, their updates; partials [n_part, C, 2] float32"""
    p = np.asarray(partials, np.longdouble)
    n_part = p.shape[0]
    S, Q = p[:, :, 0].sum(0).astype(np.float64), p[:, :, 1].sum(0).astype(np.float64)
    k = (n_part + 4) * U64
    m0 = S / count
    dm = k * np.abs(p[:, :, 0]).sum(0).astype(np.float64) / count
    var = np.maximum(Q / count - m0 * m0, 0.0)
    dv = k * (Q / count + m0 * m0)
    eps64, mom, om = float(f32(eps)), float(f32(momentum)), float(f32(1) - f32(momentum))
    bias, gam, bet = _f64(np.zeros_like(S) if conv_bias is None else conv_bias, gamma, beta)
    inv = 1.0 / np.sqrt(var + eps64)
    di = (1.0 / np.sqrt(np.maximum(var - dv, 0.0) + eps64) - inv) + 4 * U64 * inv
    di = di + U32 * (inv + di)
    mean = m0 + bias
    dmean = dm + U64 * np.abs(mean)
    dmean = dmean + U32 * (np.abs(mean) + dmean)
    A = gam * inv
    dA = np.abs(gam) * di + U32 * np.abs(gam) * (inv + di)
    am, aA = np.abs(mean) + dmean, np.abs(A) + dA
    Bv = bet - mean * A
    dB = am * dA + dmean * np.abs(A) + U32 * am * aA
    dB = dB + U32 * (np.abs(Bv) + dB)
    out = {"mean": (mean, dmean), "invstd": (inv, di), "a": (A, dA), "b": (Bv, dB)}
    if rmean is not None:
        unb = var * (count / (count - 1.0)) if count > 1 else var
        dunb = (dv * (count / (count - 1.0)) if count > 1 else dv) + 4 * U64 * unb
        dunb = dunb + U32 * (unb + dunb)
        for name, old, new, dnew in (("rmean", rmean, mean, dmean), ("rvar", rvar, unb, dunb)):
            old = np.asarray(old, np.float64)
            t1, t2 = om * old, mom * new
            e2 = mom * dnew + U32 * mom * (np.abs(new) + dnew)
            e = U32 * np.abs(t1) + e2
            out[name] = (t1 + t2, e + U32 * (np.abs(t1 + t2) + e))
    return out


def restate_stats(partials, count, conv_bias, gamma, beta, eps, momentum, rmean=None, rvar=None, nbt=0, mut=None):
    """bn_fwd_finish: fp64 sums, then every float32 operation on its own.  Returns the outputs and the new nbt."""
    p = np.asarray(partials, np.float64)
    C = p.shape[1]
    S, Q = p[:, :, 0].sum(0), p[:, :, 1].sum(0)
    m0 = S / count
    var = Q / count - m0 * m0
    if mut != "no_clamp":
        var = np.maximum(var, 0.0)
    mean = m0 + (0.0 if conv_bias is None or mut == "no_conv_bias" else np.asarray(conv_bias, np.float64))
    with np.errstate(invalid="ignore"):
        inv = (1.0 / np.sqrt(var + float(f32(eps)))).astype(f32)
    meanf = mean.astype(f32)
    A = np.asarray(gamma, f32) * inv
    Bv = np.asarray(beta, f32) - meanf * A
    out = dict(mean=meanf, invstd=inv, a=A, b=Bv)
    if rmean is not None:
        unb = (var * (count / (count - 1.0)) if count > 1 else var).astype(f32)
        om, mom = f32(1) - f32(momentum), f32(momentum)
        out["rmean"] = om * np.asarray(rmean, f32) + mom * meanf
        out["rvar"] = om * np.asarray(rvar, f32) + mom * unb
    assert all(v.dtype == f32 for v in out.values())
    return out, nbt + (C if mut == "nbt_per_channel" else 1)


def make_partials(n_part, C, seed=0, cnt=64):
    """partials [n_part, C, 2] of n_part tiles of cnt elements each, count, and the planted channels:
    channel 0 constant (every element 3: var = 0 up to rounding, the clamp), the last channel |mean| / std = 1e3"""
    rng = np.random.default_rng(1000 * seed + 31 * n_part + C)
    mu, sd = rng.standard_normal(C) * 0.5, rng.random(C) + 0.5
    mu[C - 1] = 1e3 * sd[C - 1]
    tm = mu + sd * rng.standard_normal((n_part, C)) / cnt ** 0.5
    tv = sd ** 2 * (1 + 0.2 * rng.standard_normal((n_part, C)).clip(-3, 3))
    part = np.stack([cnt * tm, cnt * (tv + tm * tm)], 2)
    part[:, 0, 0], part[:, 0, 1] = cnt * 3.0, cnt * 9.0
    ops = dict(partials=part.astype(f32), count=n_part * cnt, conv_bias=(rng.standard_normal(C) * 0.1).astype(f32),
               gamma=(rng.random(C) + 0.5).astype(f32), beta=(rng.standard_normal(C) * 0.3).astype(f32), eps=1e-5, momentum=0.1,
               rmean=(rng.standard_normal(C) * 0.2).astype(f32), rvar=(rng.random(C) + 0.5).astype(f32))
    return ops


def make_partials_count1(C, seed=0):
    """one tile of one element: S = y, Q = fl(y*y), count = 1 (var = 0 up to the rounding of Q; unbiased = var)"""
    ops = make_partials(1, C, seed, cnt=1)
    yv = ops["partials"][:, :, 0]
    ops["partials"][:, :, 1] = yv * yv
    return ops


# ---- operands of the backward -------------------------------------------------------------------------------------------------
def _coefficients(y, gamma_, beta, eps=1e-5):
    yd = y.astype(np.float64)
    mean = yd.mean((0, 1, 2))
    invstd = 1.0 / np.sqrt(yd.var((0, 1, 2)) + eps)
    a = gamma_ * invstd
    return mean.astype(f32), invstd.astype(f32), a.astype(f32), (beta - mean * a).astype(f32)


@functools.lru_cache(maxsize=4)
def dense(prec, route, shape, seed=0):
    """Random operands in the element type, nothing kept away from zeros or ties, with planted decisions:
      * channel 1 has a = 2, b = -1 and y = 0.5 at every 7th pixel: a pre-activation exactly 0 (masked: the mask is a strict > 0);
      * channel 0, every 5th window from 1: four equal positive maxima; from 2: two equal positive maxima (positions 1 and 2);
      * every 5th window from 4: all channels negative (the pool gradient goes to position 0 and is masked there).
    head: dl [P, 8], w [8, C] (the callers cut the classes down)."""
    dt = PREC[prec]["dt"]
    B, C, H, W = shape
    N = B * H * W
    gen = torch.Generator().manual_seed(20261020 + 1000 * seed + 7 * C + H * W)
    rnd = lambda *s: torch.randn(*s, generator=gen).numpy()     # noqa: E731
    y = rnd(B, H, W, C)
    gamma_, beta = torch.rand(C, generator=gen).numpy() + 0.5, rnd(C) * 0.3
    mean, invstd, a, b = _coefficients(round_to(y, dt), gamma_, beta)
    if C > 1:
        a[1], b[1] = 2.0, -1.0
    yw = to_windows(y)
    Hw, Ww = yw.shape[1:3]
    wi = np.arange(B * Hw * Ww).reshape(B, Hw, Ww)
    hi, lo, neg = (1.0 - b) / a, (0.25 - b) / a, (-1.0 - b) / a
    yw[wi % 5 == 4] = neg
    if route == "pool":
        yw[wi % 5 == 1, :, 0] = hi[0]
        sel = wi % 5 == 2
        yw[sel, 0, 0], yw[sel, 3, 0], yw[sel, 1, 0], yw[sel, 2, 0] = lo[0], lo[0], hi[0], hi[0]
    y = np.ascontiguousarray(from_windows(yw, H, W))
    yf = y.reshape(N, C)
    if C > 1:
        yf[np.arange(N) % 7 == 3, 1] = 0.5
    y = round_to(y, dt)
    ops = dict(prec=prec, route=route, shape=shape, y=y, a=a, b=b, mean=mean, invstd=invstd)
    if route == "head":
        ops["dl"] = rnd(N, 8).astype(f32)
        ops["w"] = np.clip(rnd(8, C) * 0.2, -0.75, 0.75).astype(f32)
    else:
        ops["g"] = round_to(rnd(B, H, W, C), dt)
    if route == "pool":
        ops["gpool"] = round_to(rnd(B, H // 2, W // 2, C), dt)
    return ops


def plants(ops):
    """counts of the planted decisions: exact-zero pre-activations, windows with 2 / 4 equal positive maxima, all-negative windows"""
    z = pre32(ops["y"], ops["a"], ops["b"])
    H, W = z.shape[1:3]
    zw = to_windows(np.maximum(z, f32(0)), fill=-1.0)[:, :H // 2, :W // 2]
    top = zw.max(3, keepdims=True)
    ties = ((zw == top) & (top > 0)).sum(3)
    return dict(zero=int((z == 0).sum()), tie2=int((ties == 2).sum()), tie4=int((ties == 4).sum()),
                negative=int((zw.max(3) == 0).all(-1).sum()))


@functools.lru_cache(maxsize=4)
def exact(prec, route, shape, seed=0):
    """Operands on which every intermediate of the kernels is exact in float32 and every output in bf16 and fp16, so the fp64
    reference, the restatement and the kernels must agree bit for bit: a, invstd in {1, 2} (powers of two), mean, b, y, g and
    dl * w small integers, t = y - mean in -2..2 so that z = a (t + 1) is 0 at t = -1 (masked) and ties abound.  c1 = s1 / N and
    c2 = s2 / N are made small integers whatever N is: without external sums the skip gradient is adjusted by +-1 steps on
    unmasked pixels with t = 1 (moves s2) and then t = 0 (moves s1 alone) until both sums are multiples of N (for a power-of-two N
    the adjustment is still needed to keep dy inside bf16's 8 bits); external rows are integers that add up to N * k."""
    B, C, H, W = shape
    N = B * H * W
    rng = np.random.default_rng(77 + 1000 * seed + 13 * C + H * W)
    ch = np.arange(C)
    a = np.where(ch % 2 == 0, 1.0, 2.0).astype(f32)
    invstd = np.where(ch % 3 == 0, 2.0, 1.0).astype(f32)
    mean = ((ch % 5) - 2).astype(f32)
    b = (a * (1 - mean)).astype(f32)
    pattern = np.array([0, 1, 0, -1, 2, 0, 1, -2, 1, 0, 1])
    t = pattern[(np.arange(N)[:, None] * 3 + ch[None, :]) % len(pattern)]
    if route == "pool":                                   # whole windows of one value: four equal positive maxima (t = 0 and
        tw = to_windows(t.reshape(B, H, W, C).astype(np.float64))     # t = 1: z = a (t + 1) > 0) and all-negative windows
        wi = np.arange(tw.shape[0] * tw.shape[1] * tw.shape[2]).reshape(tw.shape[:3])
        for kind, tv in ((1, 0), (2, -2), (3, 1)):
            tw[wi % 4 == kind] = tv
        t = from_windows(tw, H, W).reshape(N, C).astype(np.int64)
    y = (t + mean).astype(f32).reshape(B, H, W, C)
    ops = dict(prec=prec, route=route, shape=shape, y=y, a=a, b=b, mean=mean, invstd=invstd)
    if route == "head":
        ops["dl"] = rng.integers(-1, 3, (N, 8)).astype(f32)
        ops["w"] = rng.integers(-1, 2, (8, C)).astype(f32)
        return ops
    g = rng.integers(-2, 4, (N, C)).astype(np.float64)
    routed = 0.0
    if route == "pool":
        ops["gpool"] = rng.integers(-2, 3, (B, H // 2, W // 2, C)).astype(f32)
        routed = route_pool(pre32(y, a, b), ops["gpool"]).reshape(N, C)
    um = t >= 0
    for c in range(C):                                     # s2 / invstd = sum gt t and s1 = sum gt -> multiples of N
        for tv, wgt in ((1, t[:, c]), (0, np.ones(N))):
            gt = (g[:, c] + (routed[:, c] if route == "pool" else 0.0)) * um[:, c]
            s = (gt * wgt).sum()
            idx = np.flatnonzero(um[:, c] & (t[:, c] == tv))
            k = int(round(s / N)) or (1 if len(idx) * 4 >= N else 0)   # a multiple other than 0 wherever there is room for one
            r = k * N - int(s)
            step = 1 if r > 0 else -1
            while r != 0:                                  # one step per pixel and round: the adjustment is spread evenly
                room = idx[np.abs(g[idx, c] + step) <= 8][:abs(r)]
                assert len(room), ("exact operands: no room to adjust", shape, c, tv)
                g[room, c] += step
                r -= step * len(room)
    ops["g"] = g.astype(f32).reshape(B, H, W, C)
    return ops


def exact_ext(C, N, rows, seed=0):
    """[rows, C, 2] integer rows that add up to N * (k1, k2), k1 in -1..2, k2 in {-2, 0, 2}"""
    rng = np.random.default_rng(5 + seed + rows + C)
    part = rng.integers(-3, 4, (rows, C, 2)).astype(np.float64)
    k = np.stack([rng.integers(-1, 3, C), 2 * rng.integers(-1, 2, C)], 1)
    part[0] += N * k - part.sum(0)
    assert (np.abs(part) < 2 ** 24).all()
    return part.astype(f32)


def call_args(ops, ncls=None):
    """the keyword operands of bwd_ref / restate_bwd"""
    kw = {k: ops[k] for k in ("y", "a", "b", "mean", "invstd")}
    for k in ("g", "gpool"):
        if k in ops:
            kw[k] = ops[k]
    if "dl" in ops:
        kw["dl"], kw["w"] = np.ascontiguousarray(ops["dl"][:, :ncls]), np.ascontiguousarray(ops["w"][:ncls])
    return kw


# ---- 2x2 max-pool ---------------------------------------------------------------------------------------------------------------
def maxpool_ref(prec, x, a=None, b=None):
    """[B, H/2, W/2, C] float32: the pool only selects, so the output is the element-type rounding of the float32 value
    max over the window of relu(fl(fl(a*x) + b)), or of x itself without the prologue"""
    z = np.asarray(x, f32) if a is None else np.maximum(pre32(x, a, b), f32(0))
    B, H, W, C = z.shape
    zw = to_windows(z)[:, :H // 2, :W // 2]
    return round_to(zw.max(3), PREC[prec]["dt"])
