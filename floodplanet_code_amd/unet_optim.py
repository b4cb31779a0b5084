"""The optimiser half of HipUNet: the Adam moments, the weight EMA, gradient clipping and decoupled weight decay as flat
caller-owned buffers and module settings that every device context is armed with (_OptimMixin, which HipUNet inherits), and
HipAdam, the torch.optim.Adam whose step is the one fused launch.

The layers above (the models, the trainer, HipAdam) hand the net one OptimOptions (HipUNet.apply_optim_options); a new
context takes the module's settings through _arm_optim.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import check, ptr
from .ema import check_decay, ema_weight
from .optim_options import OptimOptions, check_grad_clip, check_weight_decay


class _OptimMixin:
    """Mixed into HipUNet, which owns the parameter table (_table, _bn), the flat parameter / gradient / running-statistics
    buffers and the device context (_ctx)."""

    def _init_optim_state(self):
        # Adam moments (torch.optim.Adam's exp_avg / exp_avg_sq) as flat caller-owned buffers: bound into every context
        # (fu_bind_adam_state), so they survive context re-creation (another tile size, a larger batch, .to(device))
        self._flat_m: Optional[torch.Tensor] = None
        self._flat_v: Optional[torch.Tensor] = None
        # weight EMA (enable_ema): (decay, warmup) and three more flat caller-owned buffers -- the average of the parameters
        # and of the BatchNorm running statistics -- bound beside the moments (fu_bind_ema_state)
        self._ema: Optional[Tuple[float, bool]] = None
        self._ema_p = self._ema_rm = self._ema_rv = None
        self._ema_pending: Optional[dict] = None      # load_ema_state_dict before the module reached its device
        self._ema_swapped = False                     # inside ema_weights(): the context reads the EMA buffers
        self._grad_clip: Optional[float] = None       # set_grad_clip: max global gradient norm of the optimiser step
        self._clip_carry = (0.0, 0.0, 0, 0, 0)        # last norm / coefficient and the counters of the contexts before this one
        self._weight_decay = 0.0                      # set_weight_decay: AdamW's decoupled decay inside the optimiser step ...
        self._decay_mask: Optional[List[bool]] = None     # ... and which tensors of the parameter table it acts on

    def _flatten_optim(self, device: torch.device):
        """_flatten's part: the moments and the EMA buffers move with the module, or are made beside the new flat buffers."""
        if self._flat_m is not None and self._flat_m.numel() == self._total:
            self._flat_m = self._flat_m.to(device)      # the optimiser state moves with the module, never resets
            self._flat_v = self._flat_v.to(device)
        else:
            self._flat_m = torch.zeros(self._total, dtype=torch.float32, device=device)
            self._flat_v = torch.zeros(self._total, dtype=torch.float32, device=device)
        if self._ema is not None:
            if self._ema_p is not None and self._ema_p.numel() == self._total:
                self._ema_p, self._ema_rm, self._ema_rv = (t.to(device) for t in (self._ema_p, self._ema_rm, self._ema_rv))
            else:                                       # the average starts at the live values
                self._ema_p, self._ema_rm, self._ema_rv = self._flat.clone(), self._flat_rm.clone(), self._flat_rv.clone()

    def adam_state(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(exp_avg, exp_avg_sq) flat fp32 buffers in parameter order (torch.optim.Adam's state, for checkpoints)."""
        return self._flat_m, self._flat_v

    def reset_adam_state(self):
        if self._flat_m is not None:
            self._flat_m.zero_()
            self._flat_v.zero_()

    # ---------------------------------------------------------------- the options as one value
    def apply_optim_options(self, options: OptimOptions, *, ema: bool = True, step: bool = True):
        """Arm the net with an OptimOptions: the one call the models, the trainer and HipAdam make.  A field left at "off"
        leaves the net's setting alone.  ema / step: which part to arm now -- the weight EMA, or what belongs to the
        optimiser step (clipping, decay); WaterSegmentationModel arms the first at construction and the second with its
        optimiser."""
        if ema and options.ema_decay is not None:
            self.enable_ema(options.ema_decay, options.ema_warmup)
        if step and options.grad_clip_norm is not None:
            self.set_grad_clip(options.grad_clip_norm)
        if step and (options.weight_decay > 0.0 or options.decay_params != "weights"):
            self.set_weight_decay(options.weight_decay, options.decay_params)
        return self

    def _arm_optim(self, h):
        """Everything a new context h takes from the module: the buffers, then the clip norm and the decay where set."""
        self._bind(h)
        if self._grad_clip is not None:               # the setting belongs to the module: every new context takes it
            check(_lib.load().fu_set_grad_clip(h, self._grad_clip))
        if self._weight_decay > 0.0:                  # likewise
            self._arm_weight_decay(h)

    def optim_key(self):
        """What a captured step depends on: which optimiser launch it holds (with the EMA or not), whether the two norm
        launches go ahead of it, and whether it is the decay-aware one."""
        return self.ema_enabled, self.grad_clip, self._decay_key()

    # ---------------------------------------------------------------- weight EMA
    def enable_ema(self, decay: float, warmup: bool = True):
        """Keep an exponential moving average of the parameters and of the BatchNorm running statistics, updated inside the
        fused Adam launch (adam_step / HipAdam.step then call fu_adam_ema_step with ema.ema_weight(decay, step, warmup)).
        The three flat buffers live on the module's device and start as copies of the live values; on a module that has not
        reached its device yet they are made when it does.  Enabling again keeps the running average and takes the new
        decay."""
        self._ema = (check_decay(decay), bool(warmup))
        if self._flat_valid and self._flat is not None and self._ema_p is None:
            with torch.no_grad():
                self._ema_p, self._ema_rm, self._ema_rv = self._flat.clone(), self._flat_rm.clone(), self._flat_rv.clone()
        if self._ctx is not None:
            self._bind(self._ctx)
        return self

    def disable_ema(self):
        """Drop the average and its buffers; adam_step launches the plain Adam kernel again."""
        if self._ema_swapped:
            raise RuntimeError("disable_ema() inside ema_weights()")
        self._ema = None
        self._ema_p = self._ema_rm = self._ema_rv = None
        self._ema_pending = None
        if self._ctx is not None:
            self._bind(self._ctx)
        return self

    @property
    def ema_enabled(self) -> bool:
        return self._ema is not None

    @property
    def ema_serving(self) -> bool:
        """True inside ema_weights(): eval forwards read the averaged weights."""
        return self._ema_swapped

    def ema_buffers(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(EMA of the flat parameters, of running_mean, of running_var): the flat fp32 buffers the kernel updates."""
        if self._ema is None or self._ema_p is None:
            raise RuntimeError("no EMA buffers: call enable_ema() and move the module to its device first")
        return self._ema_p, self._ema_rm, self._ema_rv

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The averaged model under exactly the keys and shapes of state_dict(): parameters and running statistics from the
        EMA buffers, num_batches_tracked from the live model.  Copies."""
        ep, erm, erv = self.ema_buffers()
        src = {}
        for name, p, off, n in self._table:
            src[name] = ep[off:off + n].view(p.shape)
        for name, m, off in self._bn:
            c = m.weight.numel()
            src[name + ".running_mean"] = erm[off:off + c]
            src[name + ".running_var"] = erv[off:off + c]
        return {k: (src[k] if k in src else v).detach().clone() for k, v in self.state_dict().items()}

    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Fill the EMA buffers from a dict shaped like state_dict() (num_batches_tracked is ignored: it follows the live
        model).  Needs enable_ema(); before the module has reached its device the values wait until it has."""
        if self._ema is None:
            raise RuntimeError("load_ema_state_dict(): call enable_ema() first")
        want = [k for k in self.state_dict().keys() if not k.endswith("num_batches_tracked")]
        missing = [k for k in want if k not in sd]
        if missing:
            raise KeyError(f"load_ema_state_dict(): missing keys {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        if not self._flat_valid or self._ema_p is None:
            self._ema_pending = {k: sd[k].detach().clone() for k in want}
            return
        with torch.no_grad():
            for name, p, off, n in self._table:
                if tuple(sd[name].shape) != tuple(p.shape):
                    raise ValueError(f"load_ema_state_dict(): {name} has shape {tuple(sd[name].shape)}, expected {tuple(p.shape)}")
                self._ema_p[off:off + n].copy_(sd[name].reshape(-1))
            for name, m, off in self._bn:
                c = m.weight.numel()
                self._ema_rm[off:off + c].copy_(sd[name + ".running_mean"])
                self._ema_rv[off:off + c].copy_(sd[name + ".running_var"])
        if self._ema_swapped:                 # the context reads these buffers now: the next eval forward, on whichever
            self._mark_dirty()                # context serves it, calls fu_params_changed first (as after load_state_dict)

    @contextlib.contextmanager
    def ema_weights(self):
        """Eval forwards inside the block read the EMA parameters and EMA running statistics: the context is re-bound to the
        EMA buffers (fu_bind_buffers + fu_params_changed) and back on exit -- the live buffers are never written, so they
        come back bitwise unchanged.  A training forward or an optimiser step inside the block raises."""
        if self._ema is None:
            raise RuntimeError("ema_weights(): call enable_ema() first")
        if self._ema_swapped:
            raise RuntimeError("ema_weights() does not nest")
        self._ema_swapped = True
        try:
            if self._ctx is not None:
                self._bind(self._ctx)
            yield self
        finally:
            self._ema_swapped = False
            if self._ctx is not None:
                self._bind(self._ctx)

    def _bind(self, h):
        """Bind the flat buffers into context h: the live ones, or inside ema_weights() the EMA ones in their place."""
        lib = _lib.load()
        if self._ema_swapped:
            p, rm, rv = self.ema_buffers()
        else:
            p, rm, rv = self._flat, self._flat_rm, self._flat_rv
        check(lib.fu_bind_buffers(h, ptr(p), ptr(self._flat_grad), ptr(rm), ptr(rv), ptr(self._flat_nbt)))
        check(lib.fu_bind_adam_state(h, ptr(self._flat_m), ptr(self._flat_v)))
        have = self._ema is not None and self._ema_p is not None
        check(lib.fu_bind_ema_state(h, ptr(self._ema_p) if have else None, ptr(self._ema_rm) if have else None,
                                    ptr(self._ema_rv) if have else None))
        check(lib.fu_params_changed(h))
        self._eval_dirty = True

    # ---------------------------------------------------------------- the step
    def adam_step(self, lr: float, step: int, betas=(0.9, 0.999), eps: float = 1e-8, grad_scale: float = 1.0):
        """Native fused Adam on the flat buffers (torch.optim.Adam semantics, water_seg_model.py:200).  With enable_ema() the
        same launch also moves the weight EMA on (fu_adam_ema_step; update number = step)."""
        dev = self._flat.device
        if self._ema_swapped:
            raise RuntimeError("HipUNet: an optimiser step inside ema_weights()")
        if self._ema is not None:
            w = ema_weight(self._ema[0], int(step), self._ema[1])
            check(_lib.load().fu_adam_ema_step(self._ctx, float(lr), float(betas[0]), float(betas[1]), float(eps), int(step),
                                               float(grad_scale), w, self._stream(dev)))
        else:
            check(_lib.load().fu_adam_step(self._ctx, float(lr), float(betas[0]), float(betas[1]), float(eps), int(step),
                                           float(grad_scale), self._stream(dev)))
        self._eval_dirty = True

    # ---------------------------------------------------------------- gradient clipping
    def set_grad_clip(self, max_norm: Optional[float]):
        """Clip the global L2 norm of the gradients to max_norm inside every optimiser step (adam_step / HipAdam.step /
        DataParallelTrainer.step): torch.nn.utils.clip_grad_norm_(parameters, max_norm) ahead of the update, computed on the
        device (fu_set_grad_clip) -- the gradient buffer itself is not rescaled.  None or 0 switches it off.  The setting
        belongs to the module and is re-applied to every context it makes."""
        max_norm = check_grad_clip(max_norm)
        self._grad_clip = max_norm
        if self._ctx is not None:
            check(_lib.load().fu_set_grad_clip(self._ctx, 0.0 if max_norm is None else max_norm))
        return self

    @property
    def grad_clip(self) -> Optional[float]:
        return self._grad_clip

    def grad_clip_state(self) -> Dict[str, float]:
        """What the clipped optimiser steps left on the device (fu_grad_clip_state): of the last one grad_norm (the global norm of the
        gradients as Adam consumed them, before clipping), clip_coef (the factor applied, 1.0 = not clipped), steps,
        clipped_steps and nonfinite_steps (such a step is skipped).  The counters run on over a change of context (another
        tile shape, a larger batch); max_norm is the module's setting.  Synchronises the device."""
        norm, coef, n, k, bad = self._read_clip_state()
        return {"max_norm": self._grad_clip, "grad_norm": norm, "clip_coef": coef, "steps": n, "clipped_steps": k,
                "nonfinite_steps": bad}

    def _read_clip_state(self):
        """(norm, coef, steps, clipped, nonfinite): the current context's state block on top of what earlier contexts left."""
        norm0, coef0, n0, k0, bad0 = self._clip_carry
        if self._ctx is None:
            return self._clip_carry
        norm, coef = C.c_float(), C.c_float()
        n, k, bad = C.c_int64(), C.c_int64(), C.c_int64()
        check(_lib.load().fu_grad_clip_state(self._ctx, C.byref(norm), C.byref(coef), C.byref(n), C.byref(k), C.byref(bad)))
        if n.value == 0:                              # no clipped step on this context yet: the last one's figures stand
            return self._clip_carry
        return norm.value, coef.value, n0 + n.value, k0 + k.value, bad0 + bad.value

    def _save_clip_state(self):
        """Before the context goes: its clip counters go with it, so keep them on the module."""
        if self._grad_clip is not None:
            self._clip_carry = self._read_clip_state()

    # ---------------------------------------------------------------- weight decay
    def set_weight_decay(self, weight_decay: Optional[float], params="weights"):
        """Decoupled weight decay (torch.optim.AdamW) inside every optimiser step (adam_step / HipAdam.step /
        DataParallelTrainer.step): each element of a decayed tensor is multiplied by float32(1 - lr * weight_decay) ahead of
        the Adam update, in the same one launch (fu_set_weight_decay).  params: "weights" -- every tensor with ndim >= 2
        (conv, transposed-conv, fusion and head weights; biases and BatchNorm weight / bias do not decay), "all" -- every
        tensor, what a bare torch.optim.AdamW(model.parameters()) does -- or an iterable of state-dict names.  None or 0
        switches it off.  The setting belongs to the module and is re-applied to every context it makes."""
        weight_decay = check_weight_decay(weight_decay)
        names = [name for name, _, _, _ in self._table]
        if isinstance(params, str):
            if params not in ("weights", "all"):
                raise ValueError(f"set_weight_decay: params must be 'weights', 'all' or parameter names, got {params!r}")
            mask = [params == "all" or p.ndim >= 2 for _, p, _, _ in self._table]
        else:
            wanted = [str(k) for k in params]
            unknown = [k for k in wanted if k not in names]
            if unknown:
                raise KeyError(f"set_weight_decay: no such parameters {unknown[:4]}{' ...' if len(unknown) > 4 else ''}")
            mask = [name in set(wanted) for name in names]
        self._weight_decay = weight_decay
        self._decay_mask = mask if weight_decay > 0.0 else None
        if self._ctx is not None:
            self._arm_weight_decay(self._ctx)
        return self

    def _arm_weight_decay(self, h):
        if self._weight_decay > 0.0:
            mask = (C.c_uint8 * len(self._table))(*[int(f) for f in self._decay_mask])
            check(_lib.load().fu_set_weight_decay(h, self._weight_decay, mask, len(self._table)))
        else:
            check(_lib.load().fu_set_weight_decay(h, 0.0, None, 0))

    @property
    def weight_decay(self) -> float:
        return self._weight_decay

    def decayed_parameter_names(self) -> List[str]:
        """The state-dict names of the tensors the armed weight decay acts on, in parameter order ([] when it is off)."""
        if self._decay_mask is None:
            return []
        return [name for (name, _, _, _), f in zip(self._table, self._decay_mask) if f]

    def _decay_key(self):
        """What a captured step depends on: (weight_decay, flags) or None when no tensor decays."""
        if self._weight_decay <= 0.0 or not any(self._decay_mask):
            return None
        return self._weight_decay, tuple(self._decay_mask)

    # ---------------------------------------------------------------- reports
    def grad_norms(self, grad_scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(per_parameter, total): the L2 norm of every parameter's gradient, in the order of grad_norm_names(), and of all
        of them, times |grad_scale| -- device tensors from one pass over the flat gradient buffer (fu_grad_norms); nothing
        is copied to the host and no optimiser state changes."""
        if self._ctx is None:
            raise RuntimeError("HipUNet.grad_norms() before any forward / backward of the module")
        dev = self._flat.device
        out = torch.empty(len(self._table) + 1, dtype=torch.float32, device=dev)
        check(_lib.load().fu_grad_norms(self._ctx, float(grad_scale), ptr(out), self._stream(dev)))
        return out[:-1], out[-1]

    def grad_norm_names(self) -> List[str]:
        """The parameter names grad_norms() reports, in its order (the parameter table's)."""
        return [name for name, _, _, _ in self._table]

    def fp16_guard_state(self) -> Tuple[int, int]:
        """(optimiser steps skipped because a gradient was not finite, current loss-scale back-off exponent) -- fp16 mode;
        (0, 0) otherwise.  Synchronises the device."""
        n, e = C.c_int64(), C.c_int32()
        check(_lib.load().fu_fp16_guard_state(self._ctx, C.byref(n), C.byref(e)))
        return n.value, e.value


class HipAdam(torch.optim.Adam):
    """A torch.optim.Adam (isinstance holds; same param_groups / defaults) whose step() is ONE launch of libfloodunet's
    fused Adam kernel on the module's flat parameter / gradient / moment buffers (fu_adam_step).

    The reference's optimiser (water_seg_model.py:198-205): lr, default betas / eps, no amsgrad; weight decay only in its
    decoupled form, below.  param_groups[0] carries lr / betas / eps as torch's Adam does (LR schedulers work);
    state_dict() holds {step, exp_avg, exp_avg_sq} per parameter like torch.optim.Adam's, the moments being views of the
    module's flat buffers.  When the module keeps a weight EMA (HipUNet.enable_ema) the step is fu_adam_ema_step, and
    state_dict() carries one more top-level entry "ema" {decay, warmup, params, running_mean, running_var} -- the flat EMA
    buffers -- so that a reloaded optimiser continues the same average.  max_grad_norm: clip the global L2 norm of the
    gradients to it inside every step() (clip_grad_norm_ ahead of the update, on the device: HipUNet.set_grad_clip).
    weight_decay > 0: torch.optim.AdamW's decoupled decay in the same launch (HipUNet.set_weight_decay) on decay_params --
    "weights" (every tensor with ndim >= 2), "all" or an iterable of state-dict names.  param_groups[0] carries
    weight_decay and decoupled_weight_decay=True as torch's does; step() reads weight_decay and lr from there, so schedulers
    and manual changes work, and state_dict() carries the decayed tensors' names as the top-level entry 'decay_params'.
    options: an OptimOptions in place of max_grad_norm / weight_decay / decay_params (its EMA fields are not HipAdam's to
    arm: the module's owner does that)."""

    def __init__(self, net, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: Optional[float] = None, weight_decay: float = 0.0, decay_params="weights",
                 options: Optional[OptimOptions] = None):
        from .unet import HipUNet
        if not isinstance(net, HipUNet):
            raise TypeError("HipAdam drives a HipUNet's flat buffers")
        if options is None:
            options = OptimOptions.make(grad_clip_norm=max_grad_norm, weight_decay=weight_decay, decay_params=decay_params)
        elif (max_grad_norm, weight_decay, decay_params) != (None, 0.0, "weights"):
            raise TypeError("HipAdam(): options together with max_grad_norm / weight_decay / decay_params; give one or the "
                            "other")
        super().__init__([p for _, p, _, _ in net._table], lr=lr, betas=betas, eps=eps, weight_decay=options.weight_decay,
                         decoupled_weight_decay=True)
        net.apply_optim_options(options, ema=False)                       # (also checks the names)
        # Where the trainer leaves a net's decay alone when its own is 0, HipAdam does not: param_groups[0] owns the value,
        # so a net armed before this optimiser is disarmed.  The difference is deliberate and lives here alone.
        if options.weight_decay == 0.0 and net.weight_decay > 0.0:
            net.set_weight_decay(0.0, options.decay_params)
        self._decay_params = options.decay_params
        self._net = net
        self._step = 0

    def _views(self):
        net = self._net
        return [(p, net._flat_m[off:off + n].view(p.shape), net._flat_v[off:off + n].view(p.shape))
                for _, p, off, n in net._table]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        net = self._net
        if net._ctx is None:
            raise RuntimeError("HipAdam.step() before any forward / backward of the module")
        grads = net.grad_views()
        if any(p.grad is None for _, p, _, _ in net._table):
            raise RuntimeError("HipAdam.step(): a parameter has no gradient (the fused kernel updates all of them)")
        # gradients that autograd accumulated outside the flat buffer (the slow path of _return_param_grads) come home
        outside = [(g, p.grad) for (_, p, _, _), g in zip(net._table, grads) if p.grad.data_ptr() != g.data_ptr()]
        if outside:
            torch._foreach_copy_([a for a, _ in outside], [b for _, b in outside])
        g = self.param_groups[0]
        wd = check_weight_decay(g.get("weight_decay", 0.0))
        if wd != net.weight_decay:                    # changed in param_groups since the last step (or loaded)
            net.set_weight_decay(wd, self._decay_params)
        self._step += 1
        net.adam_step(g["lr"], self._step, g["betas"], g["eps"])
        return loss

    def state_dict(self):
        sd = super().state_dict()
        if self._net._flat_m is not None:
            sd["state"] = {i: {"step": torch.tensor(float(self._step)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
                           for i, (_, m, v) in enumerate(self._views())}
        net = self._net
        if net._ema is not None and net._ema_p is not None:
            sd["ema"] = {"decay": net._ema[0], "warmup": net._ema[1], "params": net._ema_p.clone(),
                         "running_mean": net._ema_rm.clone(), "running_var": net._ema_rv.clone()}
        if net.weight_decay > 0.0:
            sd["decay_params"] = net.decayed_parameter_names()
        return sd

    def load_state_dict(self, state_dict):
        st = state_dict.get("state", {})
        super().load_state_dict({"state": {}, "param_groups": state_dict["param_groups"]})
        if st:
            if self._net._flat_m is None:
                raise RuntimeError("HipAdam.load_state_dict(): move the module to its device first")
            for i, (_, m, v) in enumerate(self._views()):
                e = st[i] if i in st else st[str(i)]
                m.copy_(e["exp_avg"])
                v.copy_(e["exp_avg_sq"])
                self._step = int(e["step"])
        if state_dict.get("decay_params") is not None:        # the value itself came with param_groups
            self._decay_params = [str(k) for k in state_dict["decay_params"]]
            self._net.set_weight_decay(self.param_groups[0].get("weight_decay", 0.0), self._decay_params)
        ema = state_dict.get("ema")
        if ema is not None:
            net = self._net
            if net._flat_m is None:
                raise RuntimeError("HipAdam.load_state_dict(): move the module to its device first")
            if net._ema is None:
                net.enable_ema(ema["decay"], ema["warmup"])
            ep, erm, erv = net.ema_buffers()
            ep.copy_(ema["params"])
            erm.copy_(ema["running_mean"])
            erv.copy_(ema["running_var"])
