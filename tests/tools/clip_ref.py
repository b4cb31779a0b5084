"""The specification of the global-norm gradient clipping ahead of the Adam step (fu_set_grad_clip) and of fu_grad_norms, in
numpy fp64.  With g the flat fp32 gradient buffer, gscale_in = float32(grad_scale) (slot 6 of the Adam scalars):

    total  = sum_i (double)g_i ^ 2                    every square is exact in fp64
    N      = sqrt(total) * |(double)gscale_in|        the norm of the gradients as Adam consumes them
    finite = isfinite(N)
    coef   = float32(max_norm / (N + 1e-6))  if max_norm > 0 and finite and max_norm / (N + 1e-6) < 1  else  float32(1)
    gscale_out = gscale_in * coef                     one fp32 multiply

A step whose N is not finite is skipped.  REL is the bound the device values are held to: the device sums n non-negative
doubles in some fixed order (<= n * 2^-53 relative, 2e-9 at 17 M elements) and rounds to float once (2^-24); 2^-23 covers both
and the rounding of sqrt and of the division."""
import math

import numpy as np

REL = 2.0 ** -23


def sq_total(g) -> float:
    """The sum of squares of an fp32 array in fp64: exact squares, numpy's pairwise sum (<= log2(n) * 2^-53 relative)."""
    x = np.asarray(g, dtype=np.float32).astype(np.float64).ravel()
    return float(np.sum(x * x))


def norm(g, grad_scale=1.0) -> float:
    """N as above (fp64)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return math.sqrt(sq_total(g)) * abs(float(np.float32(grad_scale)))


def clip(g, max_norm, grad_scale=1.0):
    """(N, coef, gscale_out, skip): N fp64, coef and gscale_out np.float32, skip = the norm is not finite."""
    gs = np.float32(grad_scale)
    x = np.asarray(g, dtype=np.float32)
    if not np.isfinite(x).all():
        n = float("nan") if np.isnan(x).any() else float("inf")
    else:
        n = norm(x, grad_scale)
    finite = math.isfinite(n)
    r = max_norm / (n + 1e-6) if finite else float("nan")
    coef = np.float32(r) if (max_norm > 0 and finite and r < 1.0) else np.float32(1.0)
    return n, coef, np.float32(gs * coef), not finite


def tensor_norms(g, table, grad_scale=1.0):
    """fu_grad_norms: per-tensor numpy.linalg.norm of the fp64 slice times |grad_scale|, then the total, as fp64.
    table: (offset, numel) per parameter."""
    x = np.asarray(g, dtype=np.float32).astype(np.float64).ravel()
    s = abs(float(grad_scale))
    per = [float(np.linalg.norm(x[o:o + n])) * s for o, n in table]
    return np.array(per + [math.sqrt(sq_total(g)) * s])


def rel_err(got, want) -> float:
    got, want = float(got), float(want)
    return abs(got - want) / abs(want) if want != 0.0 else abs(got)
