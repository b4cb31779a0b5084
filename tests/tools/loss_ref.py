"""The specification of the loss kernels (fu_loss_ce, fu_loss_ce_weighted, fu_loss_ce_focal, fu_loss_bce_dice) for the
op-level tests: loss, closed-form dL/dlogits, valid count, summed weight D and confusion matrix, in NumPy float64, written
from the formulas of include/floodunet.h / the header comment of fu_loss.hip and from oracle.bce_dice_loss -- not from the
kernel bodies.  tests/test_loss_ref_cpu.py pins every closed form to fp64 autograd (F.cross_entropy, focal_ref.focal_loss,
oracle.bce_dice_loss) at 1e-12.  The focal form is tools/focal_ref.py's; this file only changes its layout.

Layout: logits z [P, C] (the kernels' NHWC with the pixels flattened), target t int64 [P].  A pixel is valid when
t != ignore_index and 0 <= t < C.  N = the valid pixels, D = the sum of w[t] over them; N == 0 or D == 0 gives loss 0 and a
zero gradient (the project's rule for the all-ignored batch).  argmax = the first maximal index, as torch.argmax on the CPU.

The per-element bound of an fp32 evaluation (grad_bound)
---------------------------------------------------------
With m = max_j z_j of the pixel and S_i the magnitude of the pixel's scalar factor,

    bound_ik = 2^-24 * (K * (1 + |z_ik - m| + max_j |z_ij - m|) * S_i + R_i)

  * 1 + |z_k - m| + max_j |z_j - m|: exp(z_k - m) carries the rounding of its argument (|z_k - m| * 2^-24 relative), the
    normaliser that of its largest argument, and the 1 stands for the handful of roundings every element has anyway.  The
    bound is ABSOLUTE in S_i: p_k - [k == t] may cancel to nothing (a target ahead by 20 has p_t = 1 in fp32), and its
    error is still a rounding of p_k, which is at most 1.
  * S_i: 1/N (plain), (c_nll w[t] + c_smooth W)/D (weighted and smoothed: the smoothing term of a zero-weight target is
    not 0, so w[t]/D alone would not do), w[t] mf/D (focal), (1 + dice_w |dDice/dp|)/N (BCE + Dice).
  * R_i, the fp32 rounding of N, D and the Dice sums, which reach every element as one common factor: N is an exact
    integer below 2^24 and 1/N rounds once -> R = 2 S_i.  D is a sum of non-negative fp32 terms that the kernels add as:
    `trips` terms per thread in series, 6 levels of a wave tree, 4 waves, the rest in fp64 -- at most trips + 9 roundings,
    one more for the fp32 copy of D and one for 1/D -> R = (trips + 12) S_i with a spare.  The Dice factor
    -(2 t Dd - Nn)/Dd^2 takes Dd and Nn from sums of the same kind (relative error d = (trips + 12) 2^-24 each); 2 t Dd - Nn
    >= Dd for t = 1, so nothing cancels and the factor is within 5 d -> R = 2/N + 5 (trips + 12) dice_w |dDice/dp| / N.
    `trips` = ceil(P / (cap * 256)) comes from the caller (the documented caps of the loss kernels' grids).
  * K is MEASURED, never taken from a kernel: restate_f32 evaluates the same stable formulas in NumPy float32 (per-pixel
    arithmetic in float32, the sums over pixels in float64, N / D / Dice sums rounded to float32), and K is the smallest
    power of two that puts its worst ratio against the fp64 reference at or below 1/4 over every input set of the tests
    (constructed_inputs for every C, ignore_index and form of test_gpu_loss_ops.py; big_inputs in all its layouts).  The
    factor 4 that is left is for the device's expf / logf / powf (a few ulp where NumPy's are below one) and for another
    summation order.  One K serves all four forms.  Measured worst ratios of the restatement (tests/test_loss_ref_cpu.py
    prints them and asserts the 1/4):

        K      plain CE   weighted / smoothed CE   focal   BCE + Dice
        8      0.153      0.121                    0.153   0.288        <- above 1/4
        16     0.083      0.088                    0.105   0.159        ->  K = 16

    (at K = 1: 0.561, 0.238, 0.448, 1.005; the ratio does not halve with K because R does not scale with it.)"""
import numpy as np
import torch

from . import focal_ref

EPS32 = 2.0 ** -24
# measured, see the module docstring: the worst float32-restatement ratio per form at K / 2 and at K
K = 16.0
MEASURED = {8.0: {"ce": 0.153, "weighted": 0.121, "focal": 0.153, "bce_dice": 0.288},
            16.0: {"ce": 0.083, "weighted": 0.088, "focal": 0.105, "bce_dice": 0.159}}

SHAPE_A = (2, 37, 45)                        # 3330 pixels: 13 full blocks of 256 and a ragged one
MARGINS = (20.0, 60.0, 88.0, 104.0, 137.5)   # fp32 exp: denormal below -87.3, zero below -104
WEIGHTS = [2.5, 0.7, 1.3, 0.25, 3.0, 0.5, 1.7, 0.9]
SHAPE_B = (592, 592)                         # one sample = 350 464 pixels; three = 1 051 392
CE_LOSS_CAP, BD_LOSS_CAP, GRAD_CAP = 1024, 400, 4096   # blocks of 256: the grids' caps (fu_loss.hip)


def sum_trips(P, cap_blocks):
    """terms one thread adds in series when P pixels go over at most cap_blocks blocks of 256"""
    return -(-int(P) // (256 * min(cap_blocks, -(-int(P) // 256))))


def valid_mask(t, ignore_index, C):
    return (t != ignore_index) & (t >= 0) & (t < C)


def class_weights(C, ignore_index):
    """C weights with a ZERO on a live class -- wherever a second live class keeps the summed weight positive"""
    w = list(WEIGHTS[:C])
    live = [c for c in range(C) if c != ignore_index]
    if len(live) >= 2:
        w[live[0]] = 0.0
    return w


def confusion(z, t, ignore_index):
    """int64 [C, C], M[t, argmax] over the valid pixels; the first maximal index wins"""
    C = z.shape[1]
    v = valid_mask(t, ignore_index, C)
    am = np.argmax(z, axis=1)
    return np.bincount(t[v] * C + am[v], minlength=C * C).reshape(C, C).astype(np.int64)


def _w(weight, C, dt):
    return np.ones(C, dt) if weight is None else np.asarray(weight, np.float32).astype(dt)


def _onehot(idx, C, dt):
    return (idx[:, None] == np.arange(C)[None, :]).astype(dt)


def _result(loss, grad, N, D, z, t, ignore_index):
    return {"loss": float(loss), "grad": grad, "n_valid": int(N), "D": float(D), "confusion": confusion(z, t, ignore_index)}


def _softmax_parts(z):
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    return m, e, e.sum(axis=1, keepdims=True)


def _cross_entropy(z32, t, ignore_index, weight, eps, dt):
    """loss = [c_nll sum_i w[t] (lse - z[t]) + c_smooth sum_i sum_c w[c] (lse - z[c])] / D,  c_nll = 1 - eps, c_smooth = eps / C
    dz_k = [c_nll w[t] (p_k - [k == t]) + c_smooth (p_k W - w[k])] / D;  w = 1, eps = 0 is the plain form (D = N)."""
    P, C = z32.shape
    z = z32.astype(dt)
    v = valid_mask(t, ignore_index, C)
    tt = np.where(v, t, 0)
    w = _w(weight, C, dt)
    c_nll, c_s = dt(1.0 - eps), dt(eps / C)
    m, e, se = _softmax_parts(z)
    nll = (m + np.log(se)) - z                                              # lse - z[c], [P, C]
    wt = w[tt] * v
    N, D = int(v.sum()), float(wt.astype(np.float64).sum())
    if N == 0 or D == 0.0:
        return 0.0, np.zeros((P, C), dt), N, D
    num = float(c_nll) * float((wt * np.take_along_axis(nll, tt[:, None], 1)[:, 0]).astype(np.float64).sum())
    if eps != 0.0:
        num += float(c_s) * float(((nll * w[None, :]).sum(axis=1) * v).astype(np.float64).sum())
    p = e / se
    g = c_nll * wt[:, None] * (p - _onehot(tt, C, dt))
    if eps != 0.0:
        g = g + c_s * (p * w.sum() - w[None, :]) * v[:, None]
    return num / D, g / dt(D), N, D


def _focal(z32, t, ignore_index, gamma, weight, dt):
    """loss = sum_i w[t] u^gamma (-log q) / D,  dz_k = w[t] (p_k - [k == t]) mf / D,  mf = u^gamma - gamma q u^(gamma-1) log q,
    with u the other classes' share of the sum (not 1 - q), -log q = log(sum) - (z_t - max), log1p of the others' sum where the
    target holds the maximum, and mf as u^gamma (1 + gamma q (-log q) / u); u == 0: the pixel drops out (floodunet.h).
    Returns mf as well (grad_bound's scalar factor)."""
    P, C = z32.shape
    z = z32.astype(dt)
    v = valid_mask(t, ignore_index, C)
    tt = np.where(v, t, 0)
    w = _w(weight, C, dt)
    oh = _onehot(tt, C, dt)
    m, e, se = _softmax_parts(z)
    se, m = se[:, 0], m[:, 0]
    et = (e * oh).sum(axis=1)
    so = (e * (1 - oh)).sum(axis=1)
    zt = (z * oh).sum(axis=1)
    u, q = so / se, et / se
    nlq = np.where(zt == m, np.log1p(so), np.log(se) - (zt - m))
    pos = u > 0
    us = np.where(pos, u, dt(1.0))
    ug = np.where(pos, us ** dt(gamma), dt(0.0))
    mf = np.where(pos, ug * (1 + dt(gamma) * q * (nlq / us)), dt(0.0))
    wt = w[tt] * v
    N, D = int(v.sum()), float(wt.astype(np.float64).sum())
    if N == 0 or D == 0.0:
        return 0.0, np.zeros((P, C), dt), N, D, np.zeros(P, dt)
    loss = float((wt * (ug * nlq)).astype(np.float64).sum()) / D
    pk = np.where(oh > 0, -u[:, None], e / se[:, None])                     # p_t - 1 = -u
    return loss, (wt * mf / dt(D))[:, None] * pk, N, D, mf


def _lse(x):
    m = x.max(axis=1)
    return m + np.log(np.exp(x - m[:, None]).sum(axis=1))


def _bce_dice(z32, t, ignore_index, dice_weight, dt, naive_log1mp=False):
    """BCE = -(1/N) sum [tb log p + (1 - tb) log(1 - p)],  Dice = 1 - (2 sum p tb + 1) / (sum p + sum tb + 1),  p = softmax(z)[1],
    tb = [t == 1], loss = BCE + dice_weight Dice (oracle.bce_dice_loss).  log(1 - p) = logsumexp(z[others]) - logsumexp(z);
        dz_k = (s_k - tb [k == 1] - (1 - tb) s1_k) / N + dice_weight dDice/dp p ([k == 1] - s_k),
    s = softmax(z), s1 = softmax over the other classes (0 at k = 1), dDice/dp = -(2 tb Dd - Nn) / Dd^2.
    naive_log1mp: the form the kernel had, log(sum_{k != 1} exp(z_k - m)) - log(sum_k exp(z_k - m)) with ONE maximum m over all
    classes and s1 from the same sum -- the negative control of tests/test_loss_ref_cpu.py.
    Returns |dDice/dp| as well (grad_bound's scalar factor)."""
    P, C = z32.shape
    assert C >= 2, "bce_dice needs class 1"
    z = z32.astype(dt)
    v = valid_mask(t, ignore_index, C)
    N = int(v.sum())
    if N == 0:
        return 0.0, np.zeros((P, C), dt), N, 0.0, np.zeros(P, dt)
    others = np.delete(z, 1, axis=1)
    m, e, se = _softmax_parts(z)
    s = e / se
    if naive_log1mp:
        with np.errstate(divide="ignore", invalid="ignore"):
            eo = np.delete(e, 1, axis=1)
            se1 = eo.sum(axis=1)
            log1mp = np.log(se1) - np.log(se[:, 0])
            s1o = np.where(se1[:, None] > 0, eo / np.where(se1 > 0, se1, dt(1.0))[:, None], dt(0.0))
    else:
        log1mp = _lse(others) - _lse(z)
        fo = np.exp(others - others.max(axis=1, keepdims=True))
        s1o = fo / fo.sum(axis=1, keepdims=True)
    s1 = np.insert(s1o, 1, 0, axis=1)
    logp = z[:, 1] - _lse(z)
    p = s[:, 1]
    tb = ((t == 1) & v).astype(dt)
    vf = v.astype(dt)
    bce = -float(np.where(tb > 0, logp, log1mp)[v].astype(np.float64).sum())
    inter = float((p * tb).astype(np.float64).sum())
    Sp, St = float((p * vf).astype(np.float64).sum()), float(tb.astype(np.float64).sum())
    Dd, Nn = Sp + St + 1.0, 2.0 * inter + 1.0
    loss = bce / N + dice_weight * (1.0 - Nn / Dd)
    invN, Dd, Nn = dt(1.0 / N), dt(Dd), dt(Nn)
    ddice = -(2 * tb * Dd - Nn) / (Dd * Dd)
    d1 = _onehot(np.ones(P, np.int64), C, dt)
    gb = (s - tb[:, None] * d1 - (1 - tb)[:, None] * s1) * invN
    gd = dt(dice_weight) * (ddice * p)[:, None] * (d1 - s)
    return loss, (gb + gd) * vf[:, None], N, float(N), np.abs(ddice)


# ---------------------------------------------------------------------------------------------------- the reference
def reference(form, z, t, ignore_index, weight=None, eps=0.0, gamma=0.0, dice_weight=1.0):
    """form: 'ce' | 'weighted' | 'focal' | 'bce_dice'.  z float32 [P, C], t int64 [P] -> dict(loss, grad fp64 [P, C], n_valid,
    D, confusion).  D is N for 'ce' and 'bce_dice'."""
    if form == "ce":
        loss, g, N, D = _cross_entropy(z, t, ignore_index, None, 0.0, np.float64)
    elif form == "weighted":
        loss, g, N, D = _cross_entropy(z, t, ignore_index, weight, eps, np.float64)
    elif form == "focal":                                                   # tools/focal_ref.py, in its [B, C, H, W] layout
        P, C = z.shape
        zz = torch.from_numpy(np.ascontiguousarray(z.T)).double().reshape(1, C, P, 1)
        tt = torch.from_numpy(t).reshape(1, P, 1)
        loss = float(focal_ref.focal_loss(zz, tt, gamma, weight, ignore_index))
        g = focal_ref.focal_dlogits_closed_form(zz, tt, gamma, weight, ignore_index).reshape(C, P).numpy().T.copy()
        v = valid_mask(t, ignore_index, C)
        N, D = int(v.sum()), float((_w(weight, C, np.float64)[np.where(v, t, 0)] * v).sum())
    elif form == "bce_dice":
        loss, g, N, D, _ = _bce_dice(z, t, ignore_index, dice_weight, np.float64)
    else:
        raise ValueError(form)
    return _result(loss, g, N, D, z, t, ignore_index)


def restate_f32(form, z, t, ignore_index, weight=None, eps=0.0, gamma=0.0, dice_weight=1.0, naive_log1mp=False):
    """The same stable formulas in NumPy float32 -> (loss, grad float32 [P, C]): what K is measured with."""
    if form in ("ce", "weighted"):
        loss, g, _, _ = _cross_entropy(z, t, ignore_index, weight if form == "weighted" else None,
                                       eps if form == "weighted" else 0.0, np.float32)
    elif form == "focal":
        loss, g, _, _, _ = _focal(z, t, ignore_index, gamma, weight, np.float32)
    elif form == "bce_dice":
        loss, g, _, _, _ = _bce_dice(z, t, ignore_index, dice_weight, np.float32, naive_log1mp)
    else:
        raise ValueError(form)
    return float(loss), g


def grad_bound(form, z, t, ignore_index, trips, weight=None, eps=0.0, gamma=0.0, dice_weight=1.0, k=None):
    """fp64 [P, C]: the per-element bound of an fp32 evaluation of the form's gradient (module docstring); 0 on invalid pixels
    and everywhere when N or D is 0 -- those elements must be exactly 0."""
    a, r = grad_bound_parts(form, z, t, ignore_index, trips, weight, eps, gamma, dice_weight)
    return EPS32 * ((K if k is None else k) * a + r)


def grad_bound_parts(form, z, t, ignore_index, trips, weight=None, eps=0.0, gamma=0.0, dice_weight=1.0):
    """(A [P, C], R [P, 1]) of bound = 2^-24 (K A + R): A = (1 + |z_k - m| + max_j |z_j - m|) S_i"""
    P, C = z.shape
    z64 = z.astype(np.float64)
    v = valid_mask(t, ignore_index, C)
    tt = np.where(v, t, 0)
    dev = np.abs(z64 - z64.max(axis=1, keepdims=True))
    shape = 1.0 + dev + dev.max(axis=1, keepdims=True)
    w = _w(weight if form in ("weighted", "focal") else None, C, np.float64)
    N, D = int(v.sum()), float((w[tt] * v).sum())
    if N == 0 or D == 0.0:
        return np.zeros((P, C)), np.zeros((P, 1))
    sum_roundings = trips + 12.0
    if form == "ce":
        S = v / N
        R = 2.0 * S
    elif form == "weighted":
        S = ((1.0 - eps) * w[tt] + (eps / C) * w.sum()) * v / D
        R = sum_roundings * S
    elif form == "focal":
        mf = _focal(z, t, ignore_index, gamma, weight, np.float64)[4]
        S = w[tt] * np.abs(mf) * v / D
        R = sum_roundings * S
    elif form == "bce_dice":
        dd = _bce_dice(z, t, ignore_index, dice_weight, np.float64)[4]
        S = (1.0 + dice_weight * dd) * v / N
        R = (2.0 + 5.0 * sum_roundings * dice_weight * dd) * v / N
    else:
        raise ValueError(form)
    return shape * S[:, None], R[:, None]


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements; inf if got is not finite or differs where the bound is 0 (invalid pixels,
    N or D == 0: exact zeros).  An evaluation passes with a ratio <= 1."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    if (err[bound == 0] != 0).any():
        return float("inf")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def loss_ok(got, spec):
    """the project's loss bound: |loss - spec| <= 1e-5 max(1, |spec|)"""
    return bool(np.isfinite(got)) and abs(got - spec) <= 1e-5 * max(1.0, abs(spec))


# ---------------------------------------------------------------------------------------------------- the inputs
def form_cases(C):
    """(label, form, keyword arguments but the weights) of section a; BCE + Dice needs class 1"""
    cases = [("ce", "ce", {}), ("weighted eps=0", "weighted", {"eps": 0.0}), ("weighted eps=0.1", "weighted", {"eps": 0.1}),
             ("focal 0.5", "focal", {"gamma": 0.5}), ("focal 2", "focal", {"gamma": 2.0})]
    if C >= 2:
        cases += [("bce_dice 0", "bce_dice", {"dice_weight": 0.0}), ("bce_dice 0.7", "bce_dice", {"dice_weight": 0.7})]
    return cases


def form_kwargs(form, kw, C, ignore_index):
    """the keyword arguments reference / restate_f32 / grad_bound take for one case"""
    kw = dict(kw)
    if form in ("weighted", "focal"):
        kw["weight"] = class_weights(C, ignore_index)
    return kw


def constructed_inputs(C, ignore_index, seed=0):
    """Section a: 2 x 37 x 45 pixels of N(0, 3) logits and uniform targets, with planted pixels: the target ahead of / behind
    the best other class by each of MARGINS (two per target class: one whose rival is class 1 -- class 0 for target 1 -- with
    every other class behind the rival by the margin as well, the confidently wrong pixel of BCE + Dice; one whose rival is
    the next class, in the company of the rest), exact two- and three-way ties for the maximum, all-equal rows, and targets
    -1, C, 255 and the ignore value.  The last two pixels -- the ragged block -- are planted ones.
    -> z float32 [P, C], t int64 [P]"""
    rng = np.random.default_rng(1000 * C + 10 * (ignore_index % 7) + seed)
    P = SHAPE_A[0] * SHAPE_A[1] * SHAPE_A[2]
    z = (3.0 * rng.standard_normal((P, C))).astype(np.float32)
    t = rng.integers(0, C, P).astype(np.int64)
    spots = iter([P - 1, P - 2] + [int(i) for i in rng.permutation(P - 2)])
    if C >= 2:
        for M in MARGINS:
            for sign in (1.0, -1.0):
                for rep in (0, 1):
                    for tc in range(C):
                        i = next(spots)
                        rival = (1 if tc != 1 else 0) if rep == 0 else (tc + 1) % C
                        rest = [c for c in range(C) if c not in (tc, rival)]
                        vals = np.sort(z[i, [c for c in range(C) if c != tc]])
                        z[i, rival] = vals[-1]
                        z[i, rest] = vals[:-1] - (np.float32(M) if rep == 0 else np.float32(0.0))
                        z[i, tc] = vals[-1] + np.float32(sign * M)
                        t[i] = tc
        for width in (2, 3):
            if C < width:
                continue
            for first in range(min(C - width + 1, 2)):
                tied = list(range(first, first + width))
                for rep in (0, 1):
                    for tc in range(C):                                     # every class as the target: some are valid
                        i = next(spots)
                        z[i, tied] = z[i].max() + np.float32(1.0 + rep)
                        t[i] = tc
    for value in (0.75, -2.5):
        for tc in range(C):
            i = next(spots)
            z[i, :] = np.float32(value)
            t[i] = tc
    for bad in (-1, C, 255, ignore_index):
        for _ in range(8):
            t[next(spots)] = bad
    return z, t


def planted_census(z, t, ignore_index):
    """What constructed_inputs planted, counted from the data over the VALID pixels: {('ahead', M) / ('behind', M) / 'tie2' /
    'tie3' / 'equal' / ('target', value): pixels}.  Margins: target against the best other class, within 1e-3."""
    P, C = z.shape
    v = valid_mask(t, ignore_index, C)
    z64 = z.astype(np.float64)
    out = {}
    if C >= 2:
        tt = np.where(v, t, 0)
        zt = np.take_along_axis(z64, tt[:, None], 1)[:, 0]
        oth = z64.copy()
        oth[np.arange(P), tt] = -np.inf
        margin = zt - oth.max(axis=1)
        for M in MARGINS:
            out[("ahead", M)] = int((v & (np.abs(margin - M) <= 1e-3)).sum())
            out[("behind", M)] = int((v & (np.abs(margin + M) <= 1e-3)).sum())
    n_max = (z == z.max(axis=1, keepdims=True)).sum(axis=1)
    out["tie2"] = int((v & (n_max == 2)).sum())
    out["tie3"] = int((v & (n_max == 3)).sum())
    out["equal"] = int((v & (n_max == C)).sum())
    for bad in (-1, C, 255, ignore_index):
        out[("target", bad)] = int((t == bad).sum())
    return out


def expected_kinds(C, ignore_index):
    """the planted kinds that exist for this class count (none where no class is live)"""
    if not [c for c in range(C) if c != ignore_index]:
        return []
    kinds = ["equal"]
    if C >= 2:
        kinds += [(side, M) for M in MARGINS for side in ("ahead", "behind")] + ["tie2"]
    if C >= 3:
        kinds.append("tie3")
    return kinds


_BIG = {}


def big_inputs():
    """Section b, C = 3: N(0, 3) logits and uniform targets for three samples of 592 x 592 (one sample = the first 350 464
    rows), with a pixel whose target 0 is behind class 1 by 120 and one whose target is ahead by 120 next to every trip
    boundary of the grids.  Built once per process.  -> z float32 [P, 3], t int64 [P]"""
    if "z" not in _BIG:
        rng = np.random.default_rng(592)
        P = 3 * SHAPE_B[0] * SHAPE_B[1]
        z = (3.0 * rng.standard_normal((P, 3), dtype=np.float32)).astype(np.float32)
        t = rng.integers(0, 3, P).astype(np.int64)
        for start in (0, 256 * BD_LOSS_CAP, 256 * CE_LOSS_CAP, SHAPE_B[0] * SHAPE_B[1] - 300, 256 * GRAD_CAP, P - 300):
            z[start + 5] = (-2.0, 118.0, -1.0)
            t[start + 5] = 0
            z[start + 261] = (121.0, 1.0, -3.0)
            t[start + 261] = 0
        _BIG["z"], _BIG["t"] = z, t
    return _BIG["z"], _BIG["t"]


def big_case(batch, valid_from):
    """One layout of section b: `batch` samples, the pixels before `valid_from` set to the ignore value -100"""
    z, t = big_inputs()
    P = batch * SHAPE_B[0] * SHAPE_B[1]
    t = t[:P].copy()
    t[:valid_from] = -100
    return z[:P], t


def big_layouts(form):
    """(batch, valid_from) of section b for one form: every pixel valid; only the pixels at or beyond cap * 256 valid, for the
    cap of the form's loss kernel (one sample crosses it) and for the gradient kernels' (three samples cross it)"""
    loss_cap = BD_LOSS_CAP if form == "bce_dice" else CE_LOSS_CAP
    return [(1, 0), (1, 256 * loss_cap), (3, 0), (3, 256 * loss_cap), (3, 256 * GRAD_CAP)]


BIG_FORMS = [("ce", "ce", {}), ("weighted eps=0.1", "weighted", {"eps": 0.1, "weight": [0.0, 0.7, 1.3]}),
             ("bce_dice 0.7", "bce_dice", {"dice_weight": 0.7})]
