"""OptimOptions: the options of the fused optimiser step -- weight EMA, gradient clipping, decoupled weight decay -- as one
checked value.

The command line (from_args), the models, the data-parallel trainer and HipAdam all build one through OptimOptions.make and
hand that single object to HipUNet.apply_optim_options, the one place that arms the net.  A new option is one field here,
its keyword and check in make, and one line where the net arms it.  Host arithmetic only: neither torch nor the GPU library
is imported.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple, Union

from .ema import check_decay

# the constructor keywords of WaterSegmentationModel and DataParallelTrainer, in the order cfg_from_args emits them
KEYWORDS = ("ema_decay", "ema_warmup", "grad_clip_norm", "weight_decay", "decay_all")


def check_weight_decay(weight_decay) -> float:
    """None -> 0.0 (off); a finite weight_decay >= 0 -> float; anything else raises."""
    if weight_decay is None:
        return 0.0
    v = float(weight_decay)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"the weight decay must be finite and >= 0, got {weight_decay!r}")
    return v


def check_grad_clip(max_norm) -> Optional[float]:
    """None / 0 -> None (off); a finite max_norm > 0 -> float; anything else raises."""
    if max_norm is None:
        return None
    v = float(max_norm)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"the gradient clipping norm must be finite and >= 0, got {max_norm!r}")
    return v if v > 0.0 else None


@dataclasses.dataclass(frozen=True)
class OptimOptions:
    """ema_decay None, grad_clip_norm None and weight_decay 0.0 mean "off".  decay_params: "weights" (every tensor with
    ndim >= 2), "all", or a tuple of state-dict names; names are checked against the net where the decay is armed
    (HipUNet.set_weight_decay)."""
    ema_decay: Optional[float] = None
    ema_warmup: bool = True
    grad_clip_norm: Optional[float] = None
    weight_decay: float = 0.0
    decay_params: Union[str, Tuple[str, ...]] = "weights"

    @classmethod
    def make(cls, *, ema_decay=None, ema_warmup=True, grad_clip_norm=None, weight_decay=0.0, decay_all=False,
             decay_params=None) -> "OptimOptions":
        """The options checked (ema.check_decay, check_grad_clip, check_weight_decay).  decay_all=True means
        decay_params="all"; decay_params may also be given itself, as HipAdam takes it."""
        if decay_all and decay_params is not None:
            raise TypeError("OptimOptions.make(): decay_all together with decay_params; give one or the other")
        if decay_params is None:
            decay_params = "all" if decay_all else "weights"
        elif not isinstance(decay_params, str):
            decay_params = tuple(str(k) for k in decay_params)
        return cls(None if ema_decay is None else check_decay(ema_decay), bool(ema_warmup), check_grad_clip(grad_clip_norm),
                   check_weight_decay(weight_decay), decay_params)

    @classmethod
    def from_args(cls, args) -> "OptimOptions":
        """The options a fit command line gave.  On top of make's checks, the rules that hold on the command line only: a
        flag that is given switches its option on, and a modifier needs the option it modifies."""
        ema_decay, clip, decay = (getattr(args, k, None) for k in ("ema_decay", "grad_clip", "weight_decay"))
        no_warmup, decay_all = bool(getattr(args, "no_ema_warmup", False)), bool(getattr(args, "decay_all", False))
        if ema_decay is not None:
            check_decay(ema_decay)
        elif no_warmup:
            raise ValueError("--no_ema_warmup needs --ema_decay")
        if clip is not None and check_grad_clip(clip) is None:
            raise ValueError("--grad_clip must be > 0 (leave the option out for no clipping)")
        if decay is not None:
            if check_weight_decay(decay) == 0.0:
                raise ValueError("--weight_decay must be > 0 (leave the option out for no decay)")
        elif decay_all:
            raise ValueError("--decay_all needs --weight_decay")
        return cls.make(ema_decay=ema_decay, ema_warmup=not no_warmup, grad_clip_norm=clip, weight_decay=decay,
                        decay_all=decay_all)

    @property
    def decay_all(self) -> bool:
        return self.decay_params == "all"

    @property
    def set_fields(self) -> Tuple[str, ...]:
        """Which of ("ema_decay", "grad_clip_norm", "weight_decay") are switched on."""
        on = (self.ema_decay is not None, self.grad_clip_norm is not None, self.weight_decay > 0.0)
        return tuple(k for k, f in zip(("ema_decay", "grad_clip_norm", "weight_decay"), on) if f)

    def as_kwargs(self) -> dict:
        """The five constructor keywords (KEYWORDS); a decay_params of names has no keyword there and is not carried."""
        return {name: getattr(self, name) for name in KEYWORDS}

    def given_kwargs(self) -> dict:
        """as_kwargs without what is "off", in KEYWORDS' order: what a command line puts into model_kwargs (ema_warmup
        goes with ema_decay)."""
        off = dict(ema_decay=None, ema_warmup=None if self.ema_decay is not None else self.ema_warmup, grad_clip_norm=None,
                   weight_decay=0.0, decay_all=False)
        return {k: v for k, v in self.as_kwargs().items() if v != off[k]}


def option_properties(cls):
    """Class decorator: KEYWORDS as read-only properties of the instance's optim_options (the models, the trainer)."""
    for name in KEYWORDS:
        setattr(cls, name, property(lambda self, _name=name: getattr(self.optim_options, _name)))
    return cls
