"""Learning-rate schedules for the fit loop: linear warm-up, then constant / linear / cosine / polynomial decay.

The optimiser step takes its lr afresh on every call (HipAdam.param_groups[0]["lr"], DataParallelTrainer.lr; the captured
step refreshes its scalars per replay), so a schedule is one number per step, formed on the host in double:

    step <= warmup_steps:  base_lr * step / warmup_steps                                   (step is 1-based)
    afterwards, t = (step - warmup_steps) / max(1, total_steps - warmup_steps) clamped to [0, 1]:
        constant   base_lr
        linear     min_lr + (base_lr - min_lr) (1 - t)
        cosine     min_lr + (base_lr - min_lr) (1 + cos(pi t)) / 2
        poly       min_lr + (base_lr - min_lr) (1 - t)^0.9
"""
from __future__ import annotations

import math

KINDS = ("constant", "linear", "cosine", "poly")
POLY_POWER = 0.9


def check_schedule(base_lr: float, kind: str, warmup_steps: int = 0, min_lr: float = 0.0):
    """The schedule's options, checked: (kind, warmup_steps, min_lr).  min_lr lies in [0, base_lr]."""
    if kind not in KINDS:
        raise ValueError(f"unknown lr schedule {kind!r}: one of {', '.join(KINDS)}")
    warmup_steps = int(warmup_steps)
    if warmup_steps < 0:
        raise ValueError(f"warmup_steps must be >= 0, got {warmup_steps}")
    min_lr = float(min_lr)
    if not math.isfinite(min_lr) or min_lr < 0.0:
        raise ValueError(f"min_lr must be finite and >= 0, got {min_lr}")
    if min_lr > float(base_lr):
        raise ValueError(f"min_lr {min_lr} is above the learning rate {base_lr}")
    return kind, warmup_steps, min_lr


def lr_at(step: int, base_lr: float, kind: str, total_steps: int, warmup_steps: int = 0, min_lr: float = 0.0) -> float:
    """The learning rate of optimiser step `step` (1-based) out of total_steps."""
    if kind not in KINDS:
        raise ValueError(f"unknown lr schedule {kind!r}: one of {', '.join(KINDS)}")
    step, total_steps, warmup_steps = int(step), int(total_steps), int(warmup_steps)
    if step < 1:
        raise ValueError(f"step is 1-based, got {step}")
    base_lr, min_lr = float(base_lr), float(min_lr)
    if step <= warmup_steps:
        return base_lr * step / warmup_steps
    t = (step - warmup_steps) / max(1, total_steps - warmup_steps)
    t = min(1.0, max(0.0, t))
    if kind == "constant":
        return base_lr
    if kind == "linear":
        return min_lr + (base_lr - min_lr) * (1.0 - t)
    if kind == "cosine":
        return min_lr + (base_lr - min_lr) * (1.0 + math.cos(math.pi * t)) / 2.0
    return min_lr + (base_lr - min_lr) * (1.0 - t) ** POLY_POWER
