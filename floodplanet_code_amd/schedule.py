"""Learning-rate schedules for the fit loop: linear warm-up, then constant / linear / cosine / polynomial decay.

The optimiser step takes its lr afresh on every call (HipAdam.param_groups[0]["lr"], DataParallelTrainer.lr; the captured
step refreshes its scalars per replay), so a schedule is one number per step, formed on the host in double:

    step <= warmup_steps:  base_lr * step / warmup_steps                                   (step is 1-based)
    afterwards, t = (step - warmup_steps) / max(1, total_steps - warmup_steps) clamped to [0, 1]:
        constant   base_lr
        linear     min_lr + (base_lr - min_lr) (1 - t)
        cosine     min_lr + (base_lr - min_lr) (1 + cos(pi t)) / 2
        poly       min_lr + (base_lr - min_lr) (1 - t)^0.9

LrSchedule is a run's schedule as one checked value: from_args reads the fit command line, from_cfg a fit config plus the
loader's length, .lr(step) is lr_at.  A new schedule option is one field there, its check in check_schedule, its key in
CFG_KEYS and its flag in fit.build_parser.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

KINDS = ("constant", "linear", "cosine", "poly")
POLY_POWER = 0.9
CFG_KEYS = ("lr_schedule", "warmup_steps", "min_lr")      # of a fit config, present only when the command line gave them


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


@dataclasses.dataclass(frozen=True)
class LrSchedule:
    """One run's schedule, checked (check_schedule).  given: which of CFG_KEYS stated it, which is what a config records
    (not compared)."""
    kind: str
    base_lr: float
    warmup_steps: int = 0
    min_lr: float = 0.0
    total_steps: Optional[int] = None
    given: Tuple[str, ...] = dataclasses.field(default=(), compare=False)

    @classmethod
    def _of(cls, stated: dict, base_lr, total_steps) -> Optional["LrSchedule"]:
        """stated: whichever of CFG_KEYS were given, with their values; None for none of them."""
        if not stated:
            return None
        kind, warmup, min_lr = check_schedule(base_lr, stated.get("lr_schedule", "constant"), stated.get("warmup_steps", 0),
                                              stated.get("min_lr", 0.0))
        return cls(kind, float(base_lr), warmup, min_lr, total_steps, tuple(stated))

    @classmethod
    def from_cfg(cls, cfg: dict, steps_per_epoch: int) -> Optional["LrSchedule"]:
        """The schedule of a fit config over n_epochs x steps_per_epoch steps (limit_train_batches caps the latter); None when
        the config has none of CFG_KEYS."""
        if cfg.get("limit_train_batches") is not None:
            steps_per_epoch = min(steps_per_epoch, int(cfg["limit_train_batches"]))
        return cls._of({k: cfg[k] for k in CFG_KEYS if k in cfg}, cfg["lr"], steps_per_epoch * int(cfg["n_epochs"]))

    @classmethod
    def from_args(cls, args) -> Optional["LrSchedule"]:
        """The schedule a fit command line gave (--lr_schedule, --warmup_steps, --min_lr against --lr); None for none.  Its
        total_steps is None: the loader's length is not known yet."""
        stated = {k: getattr(args, k, None) for k in CFG_KEYS}
        return cls._of({k: v for k, v in stated.items() if v is not None}, args.lr, None)

    def given_cfg(self) -> dict:
        """The top-level config keys of what was stated, as stated."""
        return {k: v for k, v in zip(CFG_KEYS, (self.kind, self.warmup_steps, self.min_lr)) if k in self.given}

    def lr(self, step: int) -> float:
        """lr_at of optimiser step `step` (1-based)."""
        return lr_at(step, self.base_lr, self.kind, self.total_steps, self.warmup_steps, self.min_lr)


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
