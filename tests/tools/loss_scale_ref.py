"""The specification of the fp16 loss scale and overflow guard (k_absmax_partial + k_loss_grad_eff in fu_loss.hip,
k_grad_finite_check + k_guard_book in fu_optim.hip), in plain numpy: float32 where the kernels are float32.

The rule both kernels share:  x is BAD  <=>  not (|x| <= float32(3.0e38)).  So +-inf, NaN and the finite floats above
3.0e38 (the next one is 3.0000002e38) are bad, and 3.0e38 itself is not.

The scale of one backward, from the stored loss gradient dl, the upstream factor `up` (1 when absent) and the guard's
back-off exponent:

    m = max |dl_i| over the entries that are not bad (0 if there is none), times |float32(up)|, one float32 multiply
    e = 6 - frexp(m).exponent   if 0 < m <= 3.0e38  (m = f * 2^e', f in [0.5, 1): m * 2^e lies in [32, 64))   else 0
    e = clamp(e - backoff, -60, 60)
    S = 2^e,  scale = (S, 1 / S) = (2^e, 2^-e), both exact floats
    out_i = dl_i * (float32(up) * S)        one rounding per element (the factor is float32(up) times a power of two)

Without a scale (fp32 / bf16 contexts with an upstream factor): out_i = dl_i * float32(up).

The guard, four integers {flag, skipped, backoff, clean}: the finite check ORs 1 into flag when an element of the
gradient buffer is bad; the book, once per optimiser step, then does

    flag set:     skipped += 1, backoff = min(backoff + 1, 14), clean = 0, flag = 0
    flag clear:   clean += 1; at clean == 64: clean = 0, backoff = max(backoff - 1, 0)"""
import numpy as np

BAD_ABOVE = np.float32(3.0e38)
E_MIN, E_MAX = -60, 60
BACKOFF_MAX = 14
CLEAN_STEPS = 64


def is_bad(x):
    """not (|x| <= float32(3.0e38)), elementwise: inf, NaN and the finite floats above 3.0e38 are bad; 3.0e38 is not."""
    with np.errstate(invalid="ignore"):
        return ~(np.abs(np.asarray(x, dtype=np.float32)) <= BAD_ABOVE)


def absmax(dl, up=None) -> np.float32:
    """m as above (float32)."""
    a = np.abs(np.asarray(dl, dtype=np.float32).ravel())
    a = a[~is_bad(a)]
    m = a.max() if a.size else np.float32(0)
    upv = np.float32(1.0 if up is None else up)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(m * np.abs(upv))


def scale_exponent(dl, up=None, backoff=0) -> int:
    m = absmax(dl, up)
    e = 0
    if m > 0 and m <= BAD_ABOVE:
        e = 6 - int(np.frexp(m)[1])
    e -= int(backoff)
    return min(max(e, E_MIN), E_MAX)


def loss_grad_eff_ref(dl, up=None, backoff=0, scaled=True):
    """(out, S, 1 / S) with a scale, (out, None, None) without: out float32 of dl's shape, S and 1 / S np.float32."""
    x = np.asarray(dl, dtype=np.float32)
    f = np.float32(1.0 if up is None else up)
    S = inv = None
    if scaled:
        e = scale_exponent(x, up, backoff)
        S, inv = np.float32(np.ldexp(1.0, e)), np.float32(np.ldexp(1.0, -e))
        with np.errstate(over="ignore", invalid="ignore"):
            f = np.float32(f * S)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        out = (x * f).astype(np.float32)
    return out, S, inv


def guard_book_ref(state, bad):
    """One optimiser step's guard: `bad` (the finite check's verdict) is ORed into the flag, then the book runs.
    state = [flag, skipped, backoff, clean] -> the four integers afterwards (a new list)."""
    flag, skipped, backoff, clean = (int(v) for v in state)
    if flag or bad:
        return [0, skipped + 1, min(backoff + 1, BACKOFF_MAX), 0]
    clean += 1
    if clean >= CLEAN_STEPS:
        clean, backoff = 0, max(backoff - 1, 0)
    return [0, skipped, backoff, clean]


def book_script():
    """The scripted sequence the CPU and the GPU test both run: (bad, note) per step, about 220 steps.
    15 bad steps (the exponent stops at 14); 63 clean, one bad, 64 clean (14 -> 15 capped at 14 -> 13: back by exactly one
    only after 64 clean steps IN A ROW); then bad / clean alternation and a final clean run."""
    seq = [True] * 15 + [False] * 63 + [True] + [False] * 64
    seq += [True, False, True, False, False] + [False] * 70
    return seq
