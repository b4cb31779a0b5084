"""fp64 reference of the 1x1 head (OutConv, fu_head.hip), analytic per-element bounds of an fp32 evaluation of it, a float32
restatement of the kernels' arithmetic (for tests/test_head_ref_cpu.py only) and the operand generator of the op-level tests.

Layout: y [P, C] (the kernels' NHWC with the pixels flattened) holding values the element type represents exactly, a / b /
mean / invstd [C] float32 or None, w [K, C], bias [K], dl [P, K] float32.

    forward    z = relu(a*y + b)  (z = y without the BatchNorm prologue: the kernels apply no ReLU of their own then)
               logits = bias + z . w^T
    backward   g = dl . w          dW = dl^T . z          db = sum_p dl
    sums       s1 = sum_p g*m      s2 = sum_p g*m*xhat    m = [a*y + b > 0], xhat = (y - mean) * invstd

BOUNDS.  u = 2^-24 is the unit roundoff of float32 and gamma(n) = n u / (1 - n u) the classical constant of an n-rounding
chain: a sum of products evaluated in ANY order in which no term passes through more than n roundings (its product and the
additions above it; an fma saves one) differs from the exact sum by at most gamma(n) * sum |x_i| |y_i|.  No constant below is
fitted; n is read from the launch code (fwd_geometry / bwd_geometry restate launch_head_fwd / launch_head_bwd).

* Input error of z.  The kernels form p = fl(a*y), z = max(fl(p + b), 0): z32 - z = a y d1 + (a y + b) d2 + a y d1 d2 with
  |d1|, |d2| <= u, so |z32 - z| <= dz = u ((1 + u) |a y| + |a y + b|) where the pre-activation is positive, and 0 where it is
  negative or exactly zero: the operands keep every pre-activation away from a sign flip (ambiguous() == 0), so the float32
  mask is the float64 one.  It reaches a result through |w| (forward) or |dl| (dW); every magnitude below is taken on
  |z| + dz, which bounds |z32|.
* logits: a lane multiplies and adds its V channels in series (1 product + V - 1 additions for the first), log2(LPP) tree
  additions join the lanes, one addition brings the bias: n = V + log2(LPP) + 1.
      bound = gamma(n) (sum_c (|z| + dz) |w| + |bias|) + sum_c dz |w|
* g: o = 0; o += dl[k] * w[k] over the classes, n = ncls (the addition to 0 is exact), then ONE rounding to the element type:
      b32 = gamma(ncls) sum_k |dl| |w|;   bound = b32 + max(eps (|g| + b32), tiny)     (nothing where sum_k |dl| |w| = 0)
  eps = the type's unit roundoff (bf16 2^-8, fp16 2^-11, fp32: no store rounding), tiny = half the spacing of the fp16
  subnormals, 2^-25, for results below 2^-14 (the two agree there).
* dW, db, s1, s2: a thread adds its T = 4 * ceil(npix / (nblk * ppb * 4)) pixels in visiting order, the block adds its ppb
  LDS rows in group order, k_head_bwd_finalize / the hook's collapse add the blocks in float64 and round once to float32:
  n = T + ppb (T for the thread's first term, ppb - 1 inexact LDS additions, the last rounding; the float64 stage is far inside
  the slack of the one exact addition counted).  ppb = 256 V / C, nblk = min(2048, ceil(npix / (4 ppb))).
      dW bound = gamma(n) sum_p |dl| (|z| + dz) + sum_p |dl| dz          db bound = gamma(n) sum_p |dl|
  The sums take the UNROUNDED float32 g (error b32 above) of the unmasked elements, and xhat as fma(y, invstd, fl(-mean *
  invstd)): |xh32 - xhat| <= dxh = u ((1 + u) |mean invstd| + |xhat|).
      s1 bound = sum_p m b32 + gamma(n) sum_p m (|g| + b32)
      s2 bound = sum_p m (b32 (|xhat| + dxh) + |g| dxh) + gamma(n) sum_p m (|g| + b32) (|xhat| + dxh)

MEASURED worst ratios of the float32 restatement against these bounds (tests/test_head_ref_cpu.py prints and asserts <= 1):
see MEASURED_RESTATEMENT below.
"""
import functools

import numpy as np
import torch

from .resample_ref import worst_ratio   # noqa: F401  (the same pass rule: max |got - ref| / bound, exact where the bound is 0)

f32 = np.float32
U32 = 2.0 ** -24
HB_BLOCKS, UNROLL, THREADS, MAX_CLS = 2048, 4, 256, 8     # launch_head_bwd / launch_head_fwd / HEAD_MAX_CLS

# vec = channels per 16-byte vector; eps / tiny: see the module docstring; big = a magnitude near the top of the type's range
# whose products with |a| <= 2, |w| <= 0.75 and |dl| ~ 1 stay far inside float32
PREC = {"fp32": dict(vec=4, dt=torch.float32, eps=0.0, tiny=0.0, big=2.0 ** 120),
        "bf16": dict(vec=8, dt=torch.bfloat16, eps=2.0 ** -8, tiny=0.0, big=2.0 ** 120),
        "fp16": dict(vec=8, dt=torch.float16, eps=2.0 ** -11, tiny=2.0 ** -25, big=6.0e4)}
CLASSES = (1, 2, 3, 4, 5, 8)             # 1..4 specialised, 5 and 8 the generic instantiation
FWD_MAIN = (2, 37, 45)                   # B, H, W of the forward's main shape
FWD_SMALL = ((1, 1, 1), (1, 3, 5))       # fewer pixels than one block
BWD_NPIX = (1, 63, 1665, 4099)
CAP_NPIX = 133333                        # > 2048 * 64: every block of the capped grid makes a second, ragged trip

# worst ratio of restate_fwd / restate_bwd against the bounds over the shapes above, as test_head_ref_cpu.py printed them
MEASURED_RESTATEMENT = {
    "fp32": dict(logits=0.575, g=0.999, dw=0.187, db=0.058),
    "bf16": dict(logits=0.524, g=0.996, dw=0.242, db=0.086, s1=0.142, s2=0.158),
    "fp16": dict(logits=0.451, g=1.000, dw=0.234, db=0.086, s1=0.156, s2=0.182),
}
# (g sits at 1 by construction: with one class it is a single product, one rounding against gamma(1); in the 16-bit types the
# store rounding reaches the type's unit roundoff.)


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def widths(prec):
    """every channel count the head kernels accept in this precision: LPP = C / V in {1, 2, 4, 8, 16}"""
    return [PREC[prec]["vec"] * lpp for lpp in (1, 2, 4, 8, 16)]


def fwd_geometry(prec, C, HW):
    """launch_head_fwd: lanes per pixel, pixels per block and unroll slot, blocks per image, trips of a block, chain length"""
    vec = PREC[prec]["vec"]
    lpp = C // vec
    assert C == lpp * vec and lpp in (1, 2, 4, 8, 16)
    ppb = THREADS // lpp
    grid = -(-(-(-HW // (ppb * UNROLL))) // 2)
    trips = -(-HW // (grid * ppb * UNROLL))
    return dict(lpp=lpp, ppb=ppb, grid=grid, trips=trips, n=vec + lpp.bit_length() - 1 + 1)


def bwd_geometry(prec, C, npix):
    """launch_head_bwd: pixels per block and unroll slot, blocks, trips of a block, terms per thread T, chain length n"""
    vec = PREC[prec]["vec"]
    lpp = C // vec
    assert C == lpp * vec and lpp in (1, 2, 4, 8, 16)
    ppb = THREADS // lpp
    nblk = min(HB_BLOCKS, -(-npix // (UNROLL * ppb)))
    trips = -(-npix // (nblk * ppb * UNROLL))
    return dict(lpp=lpp, ppb=ppb, nblk=nblk, trips=trips, T=UNROLL * trips, n=UNROLL * trips + ppb)


def round_to(x, dt):
    """float32 values the element type holds exactly (round to nearest even, as the kernels' stores)"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).to(dt).float().numpy()


def _f64(*xs):
    return tuple(None if x is None else np.asarray(x, np.float64) for x in xs)


def activation(y, a, b):
    """(z, dz, m) in float64: the head's input, the bound of its float32 evaluation's error, the ReLU mask (None without BN)"""
    y, a, b = _f64(y, a, b)
    if a is None:
        return y, np.zeros_like(y), None
    ay = a * y
    pre = ay + b
    m = pre > 0
    return np.where(m, pre, 0.0), np.where(m, U32 * ((1 + U32) * np.abs(ay) + np.abs(pre)), 0.0), m


def ambiguous(y, a, b, planted_zero=None):
    """elements whose float64 pre-activation is too close to zero for a float32 evaluation to be sure of its sign:
    |a*y + b| < 2^-20 (|a*y| + |b|), except the deliberate exact zeros"""
    y, a, b = _f64(y, a, b)
    ay = a * y
    amb = np.abs(ay + b) < 2.0 ** -20 * (np.abs(ay) + np.abs(b))
    if planted_zero is not None:
        amb &= ~(planted_zero & (ay + b == 0))
    return amb


def fwd_ref(prec, y, a, b, w, bias):
    """(ref, bound) of the logits [P, K]"""
    w, bias = _f64(w, bias)
    z, dz, _ = activation(y, a, b)
    n = fwd_geometry(prec, y.shape[1], 1)["n"]
    aw = np.abs(w).T
    return z @ w.T + bias, gamma(n) * ((np.abs(z) + dz) @ aw + np.abs(bias)) + dz @ aw


def store_bound(prec, ref, mag, b32):
    """b32 plus one rounding of a float32 value within b32 of ref to the element type; exact zeros where mag == 0"""
    eps, tiny = PREC[prec]["eps"], PREC[prec]["tiny"]
    if eps == 0.0:
        return b32
    return np.where(mag > 0, b32 + np.maximum(eps * (np.abs(ref) + b32), tiny), 0.0)


def bwd_ref(prec, dl, y, a, b, w, mean=None, invstd=None):
    """{name: (ref, bound)} for g [P, C], dw [K, C], db [K] and, with mean / invstd, s1 / s2 [C]"""
    dl, w, y64 = _f64(dl, w, y)
    P, C = y64.shape
    K = w.shape[0]
    n = bwd_geometry(prec, C, P)["n"]
    z, dz, m = activation(y, a, b)
    adl = np.abs(dl)
    g, gmag = dl @ w, adl @ np.abs(w)
    b32 = gamma(K) * gmag
    out = {"g": (g, store_bound(prec, g, gmag, b32)),
           "dw": (dl.T @ z, gamma(n) * (adl.T @ (np.abs(z) + dz)) + adl.T @ dz),
           "db": (dl.sum(0), gamma(n) * adl.sum(0))}
    if mean is not None:
        assert m is not None
        mean, invstd = _f64(mean, invstd)
        xh = (y64 - mean) * invstd
        dxh = U32 * ((1 + U32) * np.abs(mean * invstd) + np.abs(xh))
        axh = np.abs(xh) + dxh
        gm, gmm, bm = g * m, (np.abs(g) + b32) * m, b32 * m
        out["s1"] = (gm.sum(0), bm.sum(0) + gamma(n) * gmm.sum(0))
        out["s2"] = ((gm * xh).sum(0), (bm * axh + np.abs(gm) * dxh).sum(0) + gamma(n) * (gmm * axh).sum(0))
    return out


def single_pixel_dw(prec, npix, dl_row, y_row, a, b):
    """(dW ref, bound) [K, C] of a gradient that is zero except dl_row at one pixel whose input row is y_row"""
    n = bwd_geometry(prec, y_row.shape[0], npix)["n"]
    z, dz, _ = activation(y_row[None, :], a, b)
    adl = np.abs(np.asarray(dl_row, np.float64))[:, None]
    return np.asarray(dl_row, np.float64)[:, None] * z, gamma(n) * adl * (np.abs(z) + dz) + adl * dz


# ---- float32 restatement of the kernels' arithmetic (CPU test only): every operation a separate float32 rounding ------------
def _act32(y, a, b):
    y = np.asarray(y, f32)
    if a is None:
        return y
    z = np.maximum((y * a).astype(f32) + b, f32(0))
    assert z.dtype == f32
    return z


def restate_fwd(prec, y, a, b, w, bias):
    """k_head_fwd: per lane V channels in series, the lanes of a pixel by a tree (largest distance first), then the bias"""
    vec = PREC[prec]["vec"]
    z = _act32(y, a, b)
    P, C = z.shape
    K = w.shape[0]
    zz, ww = z.reshape(P, 1, C // vec, vec), np.asarray(w, f32).reshape(1, K, C // vec, vec)
    d = zz[..., 0] * ww[..., 0] + zz[..., 1] * ww[..., 1]
    for j in range(2, vec):
        d = d + zz[..., j] * ww[..., j]
    while d.shape[-1] > 1:
        h = d.shape[-1] // 2
        d = d[..., h:] + d[..., :h]
    out = d[..., 0] + np.asarray(bias, f32)
    assert out.dtype == f32
    return out


def restate_bwd(prec, dl, y, a, b, w, mean=None, invstd=None):
    """k_head_bwd + k_head_bwd_finalize: thread (block, group) visits pixel ((trip * nblk + block) * 4 + u) * ppb + group"""
    dl, w = np.asarray(dl, f32), np.asarray(w, f32)
    P, C = y.shape
    K = w.shape[0]
    geo = bwd_geometry(prec, C, P)
    nblk, ppb = geo["nblk"], geo["ppb"]
    z = _act32(y, a, b)
    o = np.zeros((P, C), f32)
    for k in range(K):
        o = o + dl[:, k:k + 1] * w[k]
    out = {"g": round_to(o, PREC[prec]["dt"])}
    sums = mean is not None
    if sums:
        mi = (-np.asarray(mean, f32) * invstd).astype(f32)
        xh = (np.asarray(y, np.float64) * np.asarray(invstd, np.float64) + mi).astype(f32)     # the fma
        gm = np.where(z > 0, o, f32(0))
    dw, db = np.zeros((nblk, ppb, K, C), f32), np.zeros((nblk, ppb, K), f32)
    s1, s2 = np.zeros((nblk, ppb, C), f32), np.zeros((nblk, ppb, C), f32)
    blk, grp = np.arange(nblk)[:, None], np.arange(ppb)[None, :]
    for trip in range(geo["trips"]):
        for u in range(UNROLL):
            p = ((trip * nblk + blk) * UNROLL + u) * ppb + grp
            ok = p < P
            pp = np.where(ok, p, 0)
            d = np.where(ok[..., None], dl[pp], f32(0))
            zz = np.where(ok[..., None], z[pp], f32(0))
            dw = dw + d[..., :, None] * zz[..., None, :]
            db = db + d
            if sums:
                gq = np.where(ok[..., None], gm[pp], f32(0))
                s1 = s1 + gq
                s2 = gq * np.where(ok[..., None], xh[pp], f32(0)) + s2

    def rows(acc):          # the block's LDS rows in group order (float32), the blocks in float64, one rounding
        t = np.zeros_like(acc[:, 0])
        for q in range(ppb):
            t = t + acc[:, q]
        assert t.dtype == f32
        return t.astype(np.float64).sum(0).astype(f32)
    out["dw"], out["db"] = rows(dw), rows(db)
    if sums:
        out["s1"], out["s2"] = rows(s1), rows(s2)
    return out


# ---- operands -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)          # the callers take the few shapes of one width through every class count, then move on
def make_operands(prec, C, npix, seed=0):
    """Operands for MAX_CLS classes (take() cuts them down), float32 arrays; y holds element-type values.  Planted:
      * channel 1 has a = 2, b = -1 and y = 0.5 at every 7th pixel: a pre-activation that is exactly 0 in float32 and float64
        (masked: the mask is a strict > 0);
      * every 11th pixel has all its pre-activations near -1 (a whole masked pixel); channel 2 has a negative a;
      * two elements of the last channel carry +-big, near the top of the element type's range, unmasked;
      * dl: a run of rows of exact zeros, a row of 1e-6 (g in fp16's subnormals), a row of +-4000 (g in fp16's top binades).
    Every other pre-activation that a float32 evaluation could get on the wrong side of zero is replaced by one near +1."""
    P = PREC[prec]
    gen = torch.Generator().manual_seed(1000 * seed + 7 * C + npix % 997)
    y = torch.randn(npix, C, generator=gen).numpy()
    a = (torch.rand(C, generator=gen) + 0.5).numpy()
    b = (torch.randn(C, generator=gen) * 0.3).numpy()
    mean = (torch.randn(C, generator=gen) * 0.1).numpy()
    invstd = (torch.rand(C, generator=gen) + 0.5).numpy()
    w = np.clip((torch.randn(MAX_CLS, C, generator=gen) * 0.2).numpy(), -0.75, 0.75)
    bias = (torch.randn(MAX_CLS, generator=gen) * 0.1).numpy()
    dl = torch.randn(npix, MAX_CLS, generator=gen).numpy()
    a[1], b[1], a[2] = 2.0, -1.0, -a[2]
    pix = np.arange(npix)
    zero_pre, dead = pix[pix % 7 == 3], pix[pix % 11 == 5]
    y[dead] = (-1.0 - b) / a
    y[zero_pre, 1] = 0.5
    bigp = np.unique([npix // 2, npix - 1])
    y[bigp, C - 1] = P["big"] * np.sign(a[C - 1])
    y = round_to(y, P["dt"])
    planted = np.zeros((npix, C), bool)
    planted[zero_pre, 1] = True
    amb = ambiguous(y, a, b, planted)
    if amb.any():
        y = np.where(amb, round_to(np.broadcast_to((1.0 - b) / a, y.shape), P["dt"]), y)
    dl[npix // 5] *= 1e-6
    if (2 * npix) // 5 not in bigp:        # 4000 * big would leave float32
        dl[(2 * npix) // 5] = np.where(dl[(2 * npix) // 5] < 0, -4000.0, 4000.0)
    dl[npix // 3:npix // 3 + 5] = 0.0
    return dict(prec=prec, C=C, npix=npix, y=y, a=a.astype(f32), b=b.astype(f32), mean=mean.astype(f32),
                invstd=invstd.astype(f32), w=w.astype(f32), bias=bias.astype(f32), dl=dl.astype(f32), planted_zero=planted,
                zero_pre=zero_pre, dead=dead, big=bigp)


def take(ops, ncls):
    """the same operands with the first ncls classes"""
    out = dict(ops)
    out.update(w=np.ascontiguousarray(ops["w"][:ncls]), bias=np.ascontiguousarray(ops["bias"][:ncls]),
               dl=np.ascontiguousarray(ops["dl"][:, :ncls]), ncls=ncls)
    return out


def check_plants(ops):
    """what the generator promises, asserted: no ambiguous pre-activation left, the planted ones are what they claim"""
    y, a, b = ops["y"], ops["a"], ops["b"]
    assert not ambiguous(y, a, b, ops["planted_zero"]).any()
    pre32 = (y * a).astype(f32) + b
    pre64 = a.astype(np.float64) * y + b
    assert ((pre32 > 0) == (pre64 > 0)).all()
    if len(ops["zero_pre"]):
        assert (pre32[ops["zero_pre"], 1] == 0).all() and (pre64[ops["zero_pre"], 1] == 0).all()
    only_dead = np.setdiff1d(ops["dead"], ops["big"])
    if len(only_dead):
        assert (pre64[only_dead][~ops["planted_zero"][only_dead]] < -0.5).all()
    assert (pre64[ops["big"], ops["C"] - 1] > 0).all() and np.isfinite(pre32).all()
    assert (np.abs(y[ops["big"], ops["C"] - 1]) >= PREC[ops["prec"]]["big"] * 0.99).all()
    n = ops["npix"]
    if n >= 16:
        assert (ops["dl"][n // 3:n // 3 + 5] == 0).all()
