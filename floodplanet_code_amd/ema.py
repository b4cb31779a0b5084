"""Exponential moving average (EMA) of the weights: the host-side arithmetic.  Torch-free, so that constructors and command
lines can validate their arguments before anything touches the GPU.

The average itself lives in three flat device buffers beside the Adam moments (HipUNet.enable_ema) and is updated inside the
fused Adam launch (fu_adam_ema_step): ema = lerp(ema, p_new, w) with w = ema_weight(decay, n).  Warm-up: the effective decay
of update n is min(decay, (1 + n) / (10 + n)), so the first updates follow the weights closely (w = 9/11 at n = 1, below 0.5
from n = 9 on) instead of averaging in the random initialisation with weight `decay`."""
from __future__ import annotations


def check_decay(decay) -> float:
    """decay as a Python float; ValueError unless it lies in [0, 1)."""
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError(f"ema decay must be a number in [0, 1), got {decay!r}") from None
    if not 0.0 <= d < 1.0:            # (NaN fails both comparisons)
        raise ValueError(f"ema decay must lie in [0, 1), got {decay!r}")
    return d


def ema_weight(decay, n_update: int, warmup: bool = True) -> float:
    """The lerp weight 1 - d of the n_update-th update (1-based): d = min(decay, (1 + n) / (10 + n)) with warm-up, else
    decay.  A Python double; the kernel rounds it to float once."""
    d = check_decay(decay)
    n = int(n_update)
    if n < 1:
        raise ValueError(f"ema_weight: n_update is 1-based, got {n_update!r}")
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return 1.0 - d
