"""LossOptions: the options of the fused cross entropy (HipUNet.loss) as one checked value.

The command line (from_args), the models, the data-parallel trainer and HipUNet.loss / train_step all build one through
LossOptions.make and hand that single object down to HipUNet._loss_raw, which picks the C entry point from it.  A new
option is one field here, its keyword and check in make, its flag in from_args and its keyword in given_kwargs (what a
fit config records), and one argument at the library call.  Host arithmetic only: neither torch nor the GPU library is
imported.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Any, Optional, Tuple


def check_label_smoothing(label_smoothing) -> float:
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:          # (NaN fails both comparisons)
        raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing!r}")
    return eps


def check_focal_gamma(focal_gamma, label_smoothing=0.0) -> float:
    """The focal exponent as a float.  ValueError unless it is finite and >= 0, and 0 wherever label smoothing is set: a
    smoothed focal loss has no agreed definition."""
    gamma = float(focal_gamma)
    if not (math.isfinite(gamma) and gamma >= 0.0):
        raise ValueError(f"focal_gamma must be finite and >= 0, got {focal_gamma!r}")
    if gamma != 0.0 and float(label_smoothing) != 0.0:
        raise ValueError(f"focal_gamma={gamma} together with label_smoothing={label_smoothing!r}: a smoothed focal loss "
                         "is not defined here, set one of them to 0")
    return gamma


def check_region_loss(weight=0.0, alpha=0.5, beta=0.5, smooth=1.0):
    """The region term's options as floats (weight, alpha, beta, smooth).  ValueError unless weight is finite and >= 0, alpha
    and beta are finite and >= 0 with alpha + beta > 0, and smooth is finite and > 0 (the rules of fu_loss_ce_region)."""
    w, a, b, s = float(weight), float(alpha), float(beta), float(smooth)
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError(f"region_weight must be finite and >= 0, got {weight!r}")
    if not (math.isfinite(a) and math.isfinite(b) and a >= 0.0 and b >= 0.0 and a + b > 0.0):
        raise ValueError(f"region_alpha, region_beta must be finite and >= 0 with alpha + beta > 0, got {alpha!r}, {beta!r}")
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"region_smooth must be finite and > 0, got {smooth!r}")
    return w, a, b, s


REGION_KINDS = {"dice": (0.5, 0.5), "jaccard": (1.0, 1.0)}      # --region_loss -> (alpha, beta); tversky takes its own
BALANCED = "balanced"                                           # --class_weights balanced, until the data resolves it


def parse_class_weights(values, n_classes: Optional[int] = None):
    """--class_weights -> None, the word 'balanced' or a list of floats (n_classes of them when n_classes is known)."""
    if values is None:
        return None
    if len(values) == 1 and values[0] == BALANCED:
        return BALANCED
    try:
        w = [float(v) for v in values]
    except ValueError:
        raise ValueError(f"--class_weights takes 'balanced' or one number per class, got {list(values)}") from None
    if n_classes is not None and len(w) != int(n_classes):
        raise ValueError(f"--class_weights: {len(w)} weights for {n_classes} classes")
    return w


@dataclasses.dataclass(frozen=True)
class LossOptions:
    """class_weight is kept as the object it was given (None, a sequence or a tensor): HipUNet._class_weight_dev checks and
    uploads it once per object.  The scalars are Python floats once they went through make."""
    class_weight: Any = None
    label_smoothing: float = 0.0
    focal_gamma: float = 0.0
    region_weight: float = 0.0
    region_alpha: float = 0.5
    region_beta: float = 0.5
    region_smooth: float = 1.0

    @classmethod
    def make(cls, n_classes: Optional[int] = None, kind: str = "ce", *, class_weight=None, label_smoothing=0.0,
             focal_gamma=0.0, region_weight=0.0, region_alpha=0.5, region_beta=0.5, region_smooth=1.0) -> "LossOptions":
        """The options checked for a loss of `kind` on a net of n_classes classes (None: not known here).  label_smoothing's
        range is checked where it is used, on the weighted and region routes of HipUNet._loss_raw."""
        gamma = check_focal_gamma(focal_gamma, label_smoothing)
        if gamma != 0.0 and kind != "ce":
            raise ValueError(f"focal_gamma belongs to kind='ce'; kind={kind!r} does not take it")
        region = check_region_loss(region_weight, region_alpha, region_beta, region_smooth)
        if region[0] != 0.0 and kind != "ce":
            raise ValueError(f"region_weight belongs to kind='ce'; kind={kind!r} does not take it")
        if region[0] != 0.0 and n_classes is not None and n_classes < 2:
            raise ValueError("a region term needs n_classes >= 2")
        eps = float(label_smoothing)
        if kind != "ce" and (class_weight is not None or eps != 0.0):
            raise ValueError(f"class_weight / label_smoothing belong to kind='ce'; kind={kind!r} takes neither")
        if kind != "ce" and region[1:] != (cls.region_alpha, cls.region_beta, cls.region_smooth):      # (the defaults)
            raise ValueError(f"region_alpha / region_beta / region_smooth belong to kind='ce'; kind={kind!r} takes none")
        return cls(class_weight, eps, gamma, *region)

    @classmethod
    def from_args(cls, args, n_classes: Optional[int] = None) -> "LossOptions":
        """The options a fit command line gave.  On top of make's checks, the rules that hold on the command line only:
        --region_weight, --tversky and --region_smooth need --region_loss, and --tversky goes with `tversky` and only with
        it.  --class_weights balanced stays the word BALANCED in class_weight: the data decides it, so the caller does."""
        weights = parse_class_weights(getattr(args, "class_weights", None), n_classes)       # reported first, as ever;
        smoothing = getattr(args, "label_smoothing", 0.0)
        gamma = check_focal_gamma(getattr(args, "focal_gamma", 0.0), smoothing)              # then the focal exponent
        kind = getattr(args, "region_loss", None)
        weight, tversky, smooth = (getattr(args, k, None) for k in ("region_weight", "tversky", "region_smooth"))
        region = {}
        if kind is None:
            given = [n for n, v in (("region_weight", weight), ("tversky", tversky), ("region_smooth", smooth)) if v is not None]
            if given:
                raise ValueError("--" + ", --".join(given) + " need --region_loss")
        else:
            if (kind == "tversky") != (tversky is not None):
                raise ValueError("--region_loss tversky and --tversky A B go together")
            alpha, beta = tversky if kind == "tversky" else REGION_KINDS[kind]
            region = dict(region_weight=1.0 if weight is None else weight, region_alpha=alpha, region_beta=beta,
                          region_smooth=1.0 if smooth is None else smooth)
        return cls.make(n_classes, class_weight=weights, label_smoothing=smoothing, focal_gamma=gamma, **region)

    def given_kwargs(self, region: Optional[bool] = None) -> dict:
        """The model keywords of what is switched on, in the order a fit config lists them: class_weights (the model's
        plural; not while it is still BALANCED), label_smoothing, focal_gamma, then the four region_* together.  region:
        whether the region term was named -- a command line that names --region_loss records its four numbers whatever
        they are, a weight of 0 included; None: when they are not the defaults."""
        out = {}
        if self.class_weight is not None and not isinstance(self.class_weight, str):
            out["class_weights"] = [float(v) for v in self.class_weight]
        if self.label_smoothing != 0.0:
            out["label_smoothing"] = self.label_smoothing
        if self.focal_gamma != 0.0:
            out["focal_gamma"] = self.focal_gamma
        if self.region != LossOptions().region if region is None else region:
            out.update(zip(("region_weight", "region_alpha", "region_beta", "region_smooth"), self.region))
        return out

    @property
    def region(self) -> Tuple[float, float, float, float]:
        """(weight, alpha, beta, smooth), the fields of FuRegionLoss in their order."""
        return self.region_weight, self.region_alpha, self.region_beta, self.region_smooth

    def as_kwargs(self) -> dict:
        """The seven options under their keyword names (the keywords of HipUNet.loss); class_weight is not copied."""
        return {name: getattr(self, name) for name in self.__dataclass_fields__}

