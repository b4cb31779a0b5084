"""The specification of fu_loss_ce_region: a cross entropy (plain, class-weighted / label-smoothed or focal: tools/loss_ref.py)
plus lambda times the soft Tversky region term over all classes, in NumPy float64, written from the formulas of
include/floodunet.h -- not from the kernel bodies.  tests/test_region_loss_cpu.py pins the closed form to fp64 autograd of the
definition at 1e-12.

Layout as loss_ref: logits z [P, C], target t int64 [P]; a pixel is valid when t != ignore_index and 0 <= t < C.  With
p = softmax(z), y_ik = [t_i == k] and every sum over the valid pixels:

    I_k = sum_i p_ik y_ik      P_k = sum_i p_ik      T_k = sum_i y_ik
    Num_k = I_k + s            Den_k = I_k + alpha (P_k - I_k) + beta (T_k - I_k) + s            TI_k = Num_k / Den_k
    R = sum_{k in K} (1 - TI_k) / |K|,   K = {0..C-1} without ignore_index;       loss = CE + lambda R
    d(lambda R)/dz_ij = lambda p_ij (g_ij - sum_k g_ik p_ik),   g_ik = A_k if y_ik else B_k
    A_k = -(alpha (P_k - I_k) + beta (T_k + s)) / (|K| Den_k^2),   B_k = alpha Num_k / (|K| Den_k^2)      (0 outside K)

The numerator of A_k is the sum of non-negative terms, not Den - (1 - beta) Num, which cancels.  Invalid pixels get exactly 0;
no valid pixel gives R = 0 exactly (TI_k = s / s).  The region term follows pixel validity, not the CE's summed weight D.

The per-element bound of an fp32 evaluation (grad_bound)
---------------------------------------------------------
    bound = loss_ref.grad_bound(CE form) + 2^-24 (K shape_i S_i + 6 (trips + 12) S_i) + 2^-24 |spec|

  * shape_i = 1 + |z_k - m| + max_j |z_j - m| and K = loss_ref.K, as there: p_ij and the p_ik inside sum_k g_ik p_ik carry the
    rounding of their exponentials' arguments.
  * S_i = lambda max_k 1 / (|K| Den_k) on valid pixels, the scale of the coefficients: Den_k - Num_k = alpha (P_k - I_k) +
    beta (T_k - I_k) >= 0, so |B_k| <= alpha / (|K| Den_k) and |A_k| <= (2 + beta) / (|K| Den_k); the small factors that are
    left (alpha, 2 + beta, the 2 of g_ij - sum_k g_ik p_ik) are in the measured ratio, not in the formula.
    The bound is ABSOLUTE in S_i, as the project's bounds are: one relative to p_ik does not hold in fp32 for a denormal p.
  * 6 (trips + 12) S_i: I_k, P_k and T_k are sums of non-negative fp32 terms with at most trips + 12 roundings each
    (loss_ref), relative error d = (trips + 12) 2^-24; A_k and B_k take Num, Den^2 and P - I from them (P - I is within
    max(alpha, 1) P d / Den of Den), within 6 d together.  `trips` = ceil(P / (region_cap(C) * 256)).
  * 2^-24 |spec|: the final add of the region gradient to the stored CE gradient rounds once.
  * The restatement (restate_f32: per-pixel arithmetic in float32, the sums over pixels in float64 and then rounded to float32)
    stays within 1/4 of the bound; tests/test_region_loss_cpu.py prints the worst ratios and asserts the 1/4.  Measured worst
    ratios at K = 16 over constructed_inputs (C in {2, 3, 4, 5, 8}, three ignore values) and the big_case layouts, the
    parameter sets PARAM_SETS, each CE form: see MEASURED below (filled from that test's output)."""
import numpy as np

from . import loss_ref as L

def region_cap(C):
    """blocks of 256 pixels per trip of k_region_sums (fu_loss.hip: region_max_blocks = LOSS_PART_FLOATS / (3 KMAX), KMAX = C up
    to 4 classes, else HEAD_MAX_CLS = 8): 682 / 455 / 341 / 170.  The cap sets the summation order and the `trips` of the bound"""
    return 4096 // (3 * (C if C <= 4 else 8))


# (alpha, beta, s): Dice with the smoothing of fu_loss_bce_dice, Jaccard, a Tversky that tells alpha from beta, a small s
PARAM_SETS = [(0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (0.3, 0.7, 1.0), (0.5, 0.5, 1e-3)]
# the worst float32-restatement ratio against grad_bound per CE form (tests/test_region_loss_cpu.py prints them)
MEASURED = {"constructed": {"ce": 0.029, "weighted": 0.064, "focal": 0.062}, "big": {"ce": 0.020, "weighted": 0.027}}


def trips(P, C):
    return L.sum_trips(P, region_cap(C))


def included(C, ignore_index):
    """bool [C]: the classes of K"""
    return np.arange(C) != ignore_index


def _region(z32, t, ignore_index, lam, alpha, beta, s, dt, swap=False, flip_b=False):
    """(lambda R, gradient [P, C], TI [C] (1 outside K), R, 1 / (|K| Den_k) [C] (0 outside K)) in the arithmetic of dt; the sums
    over pixels in float64, then rounded to dt.  swap / flip_b: the comparator controls (alpha and beta exchanged in the
    gradient's coefficients; the sign of B_k flipped)."""
    P, C = z32.shape
    z = z32.astype(dt)
    v = L.valid_mask(t, ignore_index, C)
    tt = np.where(v, t, 0)
    m, e, se = L._softmax_parts(z)
    p = e * (dt(1.0) / se)
    y = (L._onehot(tt, C, dt) > 0) & v[:, None]
    inc = included(C, ignore_index)
    nk = int(inc.sum())
    I = (p * y).astype(np.float64).sum(axis=0).astype(dt)
    Pk = (p * v[:, None]).astype(np.float64).sum(axis=0).astype(dt)
    T = y.astype(np.float64).sum(axis=0).astype(dt)
    a, b, s_ = dt(alpha), dt(beta), dt(s)
    fp, fn = np.maximum(Pk - I, dt(0.0)), np.maximum(T - I, dt(0.0))
    num = I + s_
    den = I + a * fp + b * fn + s_
    ti = np.where(inc, num / den, dt(1.0))
    if nk == 0 or not v.any():
        return 0.0, np.zeros((P, C), dt), ti, 0.0, np.zeros(C)
    R = float(((1.0 - ti.astype(np.float64)) * inc).sum() / nk)
    ga, gb = (b, a) if swap else (a, b)
    q = np.where(inc, dt(1.0) / (dt(nk) * den * den), dt(0.0))
    A = -(ga * fp + gb * (T + s_)) * q
    B = (-ga if flip_b else ga) * num * q
    g = np.where(y, A[None, :], B[None, :])
    gp = (g * p).sum(axis=1, keepdims=True)
    dz = (dt(lam) * p * (g - gp)) * v[:, None]
    G = np.where(inc, 1.0 / (nk * den.astype(np.float64)), 0.0)
    return lam * R, dz, ti, R, G


def _ce_form(form):
    if form not in ("ce", "weighted", "focal"):
        raise ValueError(f"the region term goes with a cross entropy form, not {form!r}")
    return form


def reference(form, z, t, ignore_index, lam, alpha, beta, s, **kw):
    """CE form + lambda R -> loss_ref.reference's dict (loss, grad fp64 [P, C], n_valid, D, confusion) with the region term in
    loss and grad, plus 'TI' [C], 'R', 'ce_loss' and 'region_grad'.  kw: the CE form's (weight, eps, gamma)."""
    out = dict(L.reference(_ce_form(form), z, t, ignore_index, **kw))
    lr, dz, ti, R, _ = _region(z, t, ignore_index, lam, alpha, beta, s, np.float64)
    out["ce_loss"] = out["loss"]
    out["loss"] = out["loss"] + lr
    out["region_grad"] = dz
    out["grad"] = out["grad"] + dz
    out["TI"], out["R"] = ti, R
    return out


def restate_f32(form, z, t, ignore_index, lam, alpha, beta, s, swap=False, flip_b=False, **kw):
    """The same stable formulas in NumPy float32 -> (loss, grad float32 [P, C]); the final add in float32"""
    loss, g = L.restate_f32(_ce_form(form), z, t, ignore_index, **kw)
    lr, dz, _, _, _ = _region(z, t, ignore_index, lam, alpha, beta, s, np.float32, swap, flip_b)
    return float(np.float32(loss) + np.float32(lr)), (g.astype(np.float32) + dz.astype(np.float32)).astype(np.float32)


def region_bound(z, t, ignore_index, lam, alpha, beta, s, k=None):
    """fp64 [P, C]: 2^-24 (K shape_i S_i + 6 (trips + 12) S_i), 0 on invalid pixels"""
    P, C = z.shape
    z64 = z.astype(np.float64)
    v = L.valid_mask(t, ignore_index, C)
    dev = np.abs(z64 - z64.max(axis=1, keepdims=True))
    shape = 1.0 + dev + dev.max(axis=1, keepdims=True)
    G = _region(z, t, ignore_index, lam, alpha, beta, s, np.float64)[4]
    S = (lam * G.max() * v)[:, None]
    return L.EPS32 * ((L.K if k is None else k) * shape * S + 6.0 * (trips(P, C) + 12.0) * S)


def grad_bound(form, z, t, ignore_index, lam, alpha, beta, s, ce_trips=None, k=None, spec=None, **kw):
    """the CE form's loss_ref.grad_bound + the region bound + 2^-24 |spec| for the final add (spec: reference(...)['grad'],
    computed here when the caller has none)"""
    P = z.shape[0]
    ce_trips = L.sum_trips(P, L.CE_LOSS_CAP) if ce_trips is None else ce_trips
    if spec is None:
        spec = reference(form, z, t, ignore_index, lam, alpha, beta, s, **kw)["grad"]
    return (L.grad_bound(_ce_form(form), z, t, ignore_index, ce_trips, k=k, **kw)
            + region_bound(z, t, ignore_index, lam, alpha, beta, s, k) + L.EPS32 * np.abs(spec))


def big_layouts():
    """(batch, valid_from) on loss_ref.big_case: every pixel valid; only the pixels at or beyond a cap valid, for the cap of
    k_region_sums (one sample crosses it many times over), of the CE loss kernel and of the gradient passes"""
    return [(1, 0), (1, 256 * region_cap(3)), (1, 256 * L.CE_LOSS_CAP), (3, 0), (3, 256 * L.GRAD_CAP)]
