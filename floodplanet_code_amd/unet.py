"""HipUNet: the reference UNet (st_water_seg/models/unet.py:80-111) executed by libfloodunet.so.

The module owns nn.Parameters / BN buffers with EXACTLY the reference's state_dict keys and OIHW
shapes (``inc.double_conv.0.weight`` ... ``outc.conv.bias``), so checkpoints, ``optim.Adam(self.parameters())``
and ``load_state_dict`` work unchanged.  All arithmetic (forward, loss, backward, optional Adam) happens in
hand-written gfx950 kernels behind the C ABI; torch only supplies device memory, streams and autograd glue.

Storage: every parameter is a view into one flat fp32 buffer in state_dict order (the same for gradients
and BN running statistics), which is what the C side binds to and what data-parallel all-reduce buckets slice.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
from torch.nn import init

from . import _lib
from ._lib import FuConfig, check, ptr
from .ema import check_decay, ema_weight  # noqa: F401 (re-exported)
from .loss_options import LossOptions, check_focal_gamma, check_label_smoothing, check_region_loss  # noqa: F401 (re-exported)
from .optim_options import check_grad_clip, check_weight_decay  # noqa: F401 (re-exported)
from .unet_optim import HipAdam, _OptimMixin  # noqa: F401 (HipAdam re-exported)


# --------------------------------------------------------------------------------------------------
# parameter holders (names mirror nn.Conv2d / nn.BatchNorm2d inside the reference's nn.Sequential)
# --------------------------------------------------------------------------------------------------
class _ConvParams(nn.Module):
    def __init__(self, cin: int, cout: int, k: int, transposed: bool = False):
        super().__init__()
        shape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
        self.weight = nn.Parameter(torch.empty(shape))
        self.bias = nn.Parameter(torch.empty(cout))
        # nn.Conv2d.reset_parameters (same RNG draws, so a seeded construction matches the reference)
        init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        fan_in, _ = init._calculate_fan_in_and_fan_out(self.weight)
        bound = 1 / math.sqrt(fan_in) if fan_in > 0 else 0
        init.uniform_(self.bias, -bound, bound)


class _BNParams(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class _Holder(nn.Module):
    """Plain container; children are attached with add_module so keys match the reference."""


def _double_conv(cin: int, cmid: int, cout: int) -> nn.Module:
    seq = _Holder()
    seq.add_module("0", _ConvParams(cin, cmid, 3))
    seq.add_module("1", _BNParams(cmid))
    seq.add_module("3", _ConvParams(cmid, cout, 3))
    seq.add_module("4", _BNParams(cout))
    h = _Holder()
    h.add_module("double_conv", seq)
    return h


def channel_plan(n_channels: int, base: int, bilinear: bool):
    """unet.py:88-98 generalised to base_feat_channels (unet.py:143-149,176-183)."""
    factor = 2 if bilinear else 1
    e = [base, base * 2, base * 4, base * 8, base * 16 // factor]
    outs = [base * 8 // factor, base * 4 // factor, base * 2 // factor, base]
    return e, outs


def _build_encoder(root: nn.Module, n_channels: int, base: int, bilinear: bool):
    """inc, down1..down4 of UNetEncoder (unet.py:143-149) attached to `root`; construction order == reference so that
    torch.manual_seed(s) gives identical weights."""
    e, _ = channel_plan(n_channels, base, bilinear)
    root.inc = _double_conv(n_channels, e[0], e[0])
    for i in range(1, 5):
        d = _Holder()
        mp = _Holder()
        mp.add_module("1", _double_conv(e[i - 1], e[i], e[i]))
        d.add_module("maxpool_conv", mp)
        root.add_module(f"down{i}", d)


def _build_decoder(root: nn.Module, n_classes: int, base: int, bilinear: bool):
    """up1..up4, outc of UNetDecoder (unet.py:176-184, channel_factor 1) attached to `root`."""
    e, outs = channel_plan(1, base, bilinear)
    low = e[4]
    for k in range(4):
        u = _Holder()
        skip = e[3 - k]
        if bilinear:
            cin = low + skip
            u.add_module("conv", _double_conv(cin, cin // 2, outs[k]))
        else:
            u.add_module("up", _ConvParams(low, low // 2, 2, transposed=True))
            u.add_module("conv", _double_conv(low // 2 + skip, outs[k], outs[k]))
        root.add_module(f"up{k + 1}", u)
        low = outs[k]
    oc = _Holder()
    oc.add_module("conv", _ConvParams(base, n_classes, 1))
    root.outc = oc


class HipUNet(_OptimMixin, nn.Module):
    """Drop-in for ``UNet(n_channels, n_classes, bilinear=True)`` running on MI355X HIP kernels.

    precision: 'fp32' (exact-f32 MFMA; logits within 1e-4 of the reference) or 'bf16'.
    """

    def __init__(self, n_channels: int, n_classes: int, bilinear: bool = True, base_channels: int = 64,
                 precision: str = "fp32"):
        super().__init__()
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}")
        self.n_channels, self.n_classes, self.bilinear = n_channels, n_classes, bilinear
        self.base_channels, self.precision = base_channels, precision
        self._build_tree()

        self._table: List[Tuple[str, nn.Parameter, int, int]] = []  # name, param, offset, numel
        off = 0
        for name, p in self.named_parameters():
            self._table.append((name, p, off, p.numel()))
            off += p.numel()
        self._total = off
        self._bn: List[Tuple[str, _BNParams, int]] = []
        boff = 0
        for name, m in self.named_modules():
            if isinstance(m, _BNParams):
                self._bn.append((name, m, boff))
                boff += m.weight.numel()
        self._total_bn = boff
        self._flat: Optional[torch.Tensor] = None
        self._flat_grad: Optional[torch.Tensor] = None
        self._flat_rm = self._flat_rv = self._flat_nbt = None
        self._init_optim_state()      # the moments, the weight EMA, clipping and decay (unet_optim._OptimMixin)
        self._generation = 0          # counts training forwards: an autograd node may only backward the latest one
        self._flat_valid = False
        self._ctx = None
        self._ctx_key = None
        self._eval_dirty = True
        self._last_batch = 0                          # samples of the last forward; (B, codes) after forward_views
        self._views = None
        # what the fused loss leaves on the device: confusion counts, (n_valid, weight_sum) of the weighted forms, the region
        # report; and the class weights' device copy (_class_weight_dev).  Each is made at the first call that needs it.
        self._confusion: Optional[torch.Tensor] = None
        self._wce_sums = self._region_terms = self._cw_cache = None
        self._exact = None
        self._xbuf = self._sync_cb = None             # exact sync: the exchange buffer and the live callback object
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._mark_dirty())

    def _build_tree(self):
        n_channels, base_channels, bilinear, n_classes = self.n_channels, self.base_channels, self.bilinear, self.n_classes
        _build_encoder(self, n_channels, base_channels, bilinear)
        _build_decoder(self, n_classes, base_channels, bilinear)

    def _enc_config(self):
        """(n_encoders, enc_channels) of fu_config: 0 = the plain UNet."""
        return 0, []

    def _c_param_name(self, name: str) -> str:
        """state_dict key -> the C side's canonical name (identity for the plain UNet)."""
        return name

    # ---------------------------------------------------------------- flat storage
    def _mark_dirty(self):
        self._eval_dirty = True

    def _apply(self, fn, *args, **kwargs):
        self._flat_valid = False
        self._eval_dirty = True
        return super()._apply(fn, *args, **kwargs)

    def _flatten(self, device: torch.device):
        with torch.no_grad():
            flat = torch.empty(self._total, dtype=torch.float32, device=device)
            for _, p, off, n in self._table:
                flat[off:off + n].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + n].view(p.shape)
            rm = torch.empty(self._total_bn, dtype=torch.float32, device=device)
            rv = torch.empty(self._total_bn, dtype=torch.float32, device=device)
            nbt = torch.empty(len(self._bn), dtype=torch.int64, device=device)
            for i, (_, m, off) in enumerate(self._bn):
                c = m.weight.numel()
                rm[off:off + c].copy_(m.running_mean)
                rv[off:off + c].copy_(m.running_var)
                nbt[i].copy_(m.num_batches_tracked)
                m.running_mean = rm[off:off + c]
                m.running_var = rv[off:off + c]
                m.num_batches_tracked = nbt[i]
            self._flat, self._flat_rm, self._flat_rv, self._flat_nbt = flat, rm, rv, nbt
            self._flat_grad = torch.zeros(self._total, dtype=torch.float32, device=device)
            for p_ in (p for _, p, _, _ in self._table):
                p_.grad = None          # (a .grad that aliased the previous flat gradient buffer would go stale)
            self._flatten_optim(device)
        self._flat_valid = True
        self._destroy_ctx()
        if self._ema is not None and self._ema_pending is not None:
            pending, self._ema_pending = self._ema_pending, None
            self.load_ema_state_dict(pending)

    def flat_parameters(self) -> torch.Tensor:
        return self._flat

    def flat_grads(self) -> torch.Tensor:
        return self._flat_grad

    def grad_views(self) -> List[torch.Tensor]:
        g = self._flat_grad
        return [g[off:off + n].view(p.shape) for _, p, off, n in self._table]

    def attach_grads(self):
        """Point every parameter's .grad at its slice of the flat gradient buffer."""
        for (_, p, off, n), gv in zip(self._table, self.grad_views()):
            p.grad = gv

    # ---------------------------------------------------------------- context
    def _destroy_ctx(self):
        if self._ctx is not None:
            self._save_clip_state()
            _lib.load().fu_destroy(self._ctx)
            self._ctx = None
            self._ctx_key = None
            self._last_batch = 0
            self._views = None

    def __del__(self):
        try:
            self._destroy_ctx()
        except Exception:
            pass

    def _get_ctx(self, device: torch.device, B: int, H: int, W: int):
        if device.type != "cuda":
            raise RuntimeError("HipUNet runs only on a ROCm GPU (device type 'cuda'); there is no CPU fallback")
        if not self._flat_valid or self._flat is None or self._flat.device != device:
            self._flatten(device)
        key = (device.index, H, W)
        if self._ctx is not None and self._ctx_key[:3] == key and self._ctx_key[3] >= B:
            return self._ctx
        self._destroy_ctx()
        lib = _lib.load()
        n_enc, enc_ch = self._enc_config()
        cfg = FuConfig(C.sizeof(FuConfig), self.n_channels, self.n_classes, self.base_channels, int(self.bilinear),
                       B, H, W, _lib.PRECISIONS[self.precision], device.index if device.index is not None else 0,
                       n_enc, (C.c_int32 * 6)(*(list(enc_ch) + [0] * (6 - len(enc_ch)))))
        h = C.c_void_p()
        check(lib.fu_create(C.byref(cfg), C.byref(h)))
        self._ctx = h
        self._ctx_key = key + (B,)
        self._verify_table()
        self._arm_optim(h)
        self._install_exact_sync(device)
        return h

    # ---------------------------------------------------------------- exact data-parallel mode
    def enable_exact_sync(self, world_size: int, group=None, enabled: bool = True):
        """SyncBN statistics + global N_valid over the ranks of `group` (include/floodunet.h, fu_set_exact_sync):
        W ranks x B tiles then reproduce one device with W*B tiles.  Gradients hold each rank's share of the global
        gradient afterwards: all-reduce them with SUM and use grad_scale 1 (DataParallelTrainer(exact=True))."""
        self._exact = (int(world_size), group) if enabled and world_size > 1 else None
        if self._ctx is not None:
            self._install_exact_sync(self._flat.device)

    def _install_exact_sync(self, device):
        lib = _lib.load()
        exact = self._exact
        if exact is None:
            if self._ctx is not None:
                check(lib.fu_set_exact_sync(self._ctx, _lib.SYNC_HOOK(0), None, 1, None, 0))   # null hook: off
            return
        import torch.distributed as dist
        world, group = exact
        nbytes = int(lib.fu_exact_sync_bytes(self._ctx))
        self._xbuf = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device=device)
        xbuf = self._xbuf

        def hook(_user, n_elems, is_double):
            try:
                t = xbuf[:n_elems] if is_double else xbuf.view(torch.float32)[:n_elems]
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)   # ordered on the current stream
                return 0
            except Exception:   # never let an exception cross the C ABI
                import traceback
                traceback.print_exc()
                return 1

        self._sync_cb = _lib.SYNC_HOOK(hook)     # keep the callback object alive as long as the context
        check(lib.fu_set_exact_sync(self._ctx, self._sync_cb, None, world, ptr(xbuf), nbytes))

    def _verify_table(self):
        lib = _lib.load()
        n = lib.fu_num_params(self._ctx)
        if n != len(self._table) or lib.fu_total_param_elems(self._ctx) != self._total:
            raise RuntimeError("parameter table mismatch between HipUNet and libfloodunet")
        name = C.c_char_p()
        ndim = C.c_int32()
        shape = (C.c_int64 * 4)()
        off = C.c_int64()
        for i, (pname, p, poff, _) in enumerate(self._table):
            check(lib.fu_param_info(self._ctx, i, C.byref(name), C.byref(ndim), shape, C.byref(off)))
            if name.value.decode() != self._c_param_name(pname) or off.value != poff or \
                    tuple(shape[:ndim.value]) != tuple(p.shape):
                raise RuntimeError(f"parameter {i}: python {pname}{tuple(p.shape)}@{poff} vs C "
                                   f"{name.value.decode()}{tuple(shape[:ndim.value])}@{off.value}")

    @staticmethod
    def _stream(device) -> int:
        return torch.cuda.current_stream(device).cuda_stream

    # ---------------------------------------------------------------- raw calls
    def _forward_raw(self, x, training: bool, want_logits: bool = True) -> Optional[torch.Tensor]:
        """x: the input tensor [B, n_channels, H, W], or a list / tuple of tensors [B, C_k, H, W] that the model sees side by
        side along the channel axis (ef_model.py:28-44 concatenates them; here fu_forward_srcs gathers them inside the
        NCHW -> NHWC conversion: no concatenated copy)."""
        if training and self._ema_swapped:
            raise RuntimeError("HipUNet: a training forward inside ema_weights(): the block serves eval forwards of the "
                               "averaged weights only")
        srcs, B, H, W, dev = self._sources(x)
        ctx = self._get_ctx(dev, B, H, W)
        lib = _lib.load()
        if training or self._eval_dirty:
            check(lib.fu_params_changed(ctx))
            self._eval_dirty = training  # a training step is followed by an optimiser update
        logits = torch.empty(B, self.n_classes, H, W, dtype=torch.float32, device=dev) if want_logits else None
        if len(srcs) == 1:
            check(lib.fu_forward(ctx, ptr(srcs[0]), B, int(training), ptr(logits), self._stream(dev)))
        else:
            arr = (C.c_void_p * len(srcs))(*[t.data_ptr() for t in srcs])
            chs = (C.c_int32 * len(srcs))(*[t.shape[1] for t in srcs])
            check(lib.fu_forward_srcs(ctx, arr, chs, len(srcs), B, int(training), ptr(logits), self._stream(dev)))
        if training:
            self._generation += 1
        self._last_batch = B
        self._views = None
        return logits

    def _sources(self, x):
        """x (a tensor or a list of tensors side by side along C) -> (contiguous fp32 sources, B, H, W, device)."""
        srcs = list(x) if isinstance(x, (list, tuple)) else [x]
        if not srcs or any(t.dim() != 4 for t in srcs) or sum(t.shape[1] for t in srcs) != self.n_channels:
            raise ValueError(f"expected input [B,{self.n_channels},H,W] (in one tensor or split along C), got "
                             f"{[tuple(t.shape) for t in srcs]}")
        srcs = [t.detach().contiguous().float() for t in srcs]
        B, _, H, W = srcs[0].shape
        dev = srcs[0].device
        if any(t.shape[0] != B or t.shape[2:] != (H, W) or t.device != dev for t in srcs):
            raise ValueError("all input tensors must share batch, tile size and device")
        return srcs, B, H, W, dev

    def _class_weight_dev(self, class_weight, device) -> Optional[torch.Tensor]:
        """class_weight (None, a sequence or a tensor) -> fp32 [n_classes] on `device`, validated on the host and rounded to
        fp32 once (check_class_weight).  The device copy is cached and reused while the caller passes the same object (for a
        tensor: at the same version): one host-side check per set of weights, not one per step."""
        if class_weight is None:
            return None
        key = (id(class_weight), getattr(class_weight, "_version", None), torch.device(device))
        cached = self._cw_cache
        if cached is not None and cached[0] == key:
            return cached[2]
        w = check_class_weight(class_weight, self.n_classes)
        dev_w = torch.from_numpy(w).to(device)
        self._cw_cache = (key, class_weight, dev_w)      # (the source object is kept: its id stays taken)
        return dev_w

    def last_weighted_sums(self):
        """(n_valid int64 scalar, weight_sum fp32 scalar) on the device, written by the last fu_loss_ce_weighted or
        fu_loss_ce_focal call: the valid pixels and D = the sum of their targets' class weights (the loss's denominator).
        None before such a call."""
        return self._wce_sums

    def last_region_terms(self):
        """fp32 [1 + n_classes] on the device, written by the last fu_loss_ce_region call with a region weight > 0: [0] = R,
        the mean of 1 - TI_k over the classes but ignore_index (before the weight), [1 + k] = the soft Tversky index TI_k
        (1.0 for the class equal to ignore_index).  None before such a call."""
        return self._region_terms

    def _region_terms_dev(self, device) -> torch.Tensor:
        terms = self._region_terms
        if terms is None or terms.device != torch.device(device):
            terms = self._region_terms = torch.zeros(1 + self.n_classes, dtype=torch.float32, device=device)
        return terms

    def _weighted_sums_dev(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        sums = self._wce_sums
        if sums is None or sums[0].device != torch.device(device):
            sums = self._wce_sums = (torch.zeros((), dtype=torch.int64, device=device),
                                     torch.zeros((), dtype=torch.float32, device=device))
        return sums

    def _loss_raw(self, target: torch.Tensor, ignore_index: int, device, kind: str = "ce", dice_weight: float = 1.0,
                  options: Optional[LossOptions] = None, **loss_kwargs) -> torch.Tensor:
        """The fused loss of the last forward.  options: a LossOptions (what loss / train_step / the trainer pass), or its
        fields as keywords, checked here.  Everything is validated on the host before the library is loaded."""
        if options is None:
            options = LossOptions.make(self.n_classes, kind, **loss_kwargs)
        elif loss_kwargs:
            raise TypeError(f"_loss_raw(): options together with {sorted(loss_kwargs)}; give one or the other")
        if kind not in ("ce", "bce_dice"):
            raise ValueError(f"unknown loss kind {kind!r}")
        gamma = options.focal_gamma
        region = options.region_weight > 0.0
        weighted = options.class_weight is not None or options.label_smoothing != 0.0
        sums = weighted or gamma != 0.0      # the forms that report (n_valid, weight_sum), alone or under a region term
        eps = check_label_smoothing(options.label_smoothing) if weighted or region else 0.0
        lib = _lib.load()
        target = target.contiguous().long()
        loss = torch.empty((), dtype=torch.float32, device=device)
        if kind == "bce_dice":
            fn, args = lib.fu_loss_bce_dice, (float(dice_weight), ptr(loss))
        else:
            if self._confusion is None or self._confusion.device != device:
                self._confusion = torch.zeros(self.n_classes * self.n_classes, dtype=torch.int64, device=device)
            args = (ptr(loss), ptr(self._confusion))
            if not (sums or region):      # the reference's loss: the same call, the same kernels as ever
                fn, args = lib.fu_loss_ce, args + (None,)
            else:
                cw = ptr(self._class_weight_dev(options.class_weight, device))
                n_valid, wsum = self._weighted_sums_dev(device) if sums else (None, None)
                args += (ptr(n_valid), ptr(wsum))
                if region:                # CE (whichever form the other options select) + the region term, one call
                    fn, args = lib.fu_loss_ce_region, (cw, eps, gamma, _lib.FuRegionLoss(*options.region)) + args + (
                        ptr(self._region_terms_dev(device)),)
                elif gamma != 0.0:        # focal modulation of the (weighted) cross entropy
                    fn, args = lib.fu_loss_ce_focal, (cw, gamma) + args
                else:
                    fn, args = lib.fu_loss_ce_weighted, (cw, eps) + args
        check(fn(self._ctx, ptr(target), int(ignore_index), *args, self._stream(device)))
        return loss

    def _backward_raw(self, dlogits: Optional[torch.Tensor], device):
        check(_lib.load().fu_backward(self._ctx, ptr(dlogits), self._stream(device)))

    def pop_confusion(self) -> Optional[torch.Tensor]:
        """[n_classes, n_classes] int64 confusion counts (target row, argmax column) accumulated by the fused
        loss calls since the last pop."""
        if self._confusion is None:
            return None
        out = self._confusion.view(self.n_classes, self.n_classes).clone()
        self._confusion.zero_()
        return out

    def eval_confusion(self, target: torch.Tensor, ignore_index: int) -> torch.Tensor:
        """Per-sample confusion counts of the last forward's resident logits: int64 [B, k, k] on the device,
        M[b, t, p] = #pixels of sample b with target t and argmax p (fu_eval_confusion; ignored / out-of-range targets
        dropped as in the fused loss).  No loss, no logits gradient, no host sync."""
        B = self._last_batch
        if self._ctx is None or B == 0:
            raise RuntimeError("eval_confusion: no forward pass yet")
        k, H, W = self.n_classes, self._ctx_key[1], self._ctx_key[2]
        target = target.contiguous().long()
        if tuple(target.shape) != (B, H, W):
            raise ValueError(f"eval_confusion: target must be [{B}, {H}, {W}] like the last forward, got {tuple(target.shape)}")
        counts = torch.zeros(B, k, k, dtype=torch.int64, device=target.device)
        check(_lib.load().fu_eval_confusion(self._ctx, ptr(target), int(ignore_index), ptr(counts),
                                            self._stream(target.device)))
        return counts

    def prob_histogram(self, target: torch.Tensor, ignore_index: int, n_bins: int = 256, probs=None):
        """Histogram of class probability against target class (calibration.py; include/floodunet.h has the bin rule):
        -> (hist int64 [k, k, n_bins], top int64 [2, n_bins]) on the device, no host sync, one launch.  probs=None: the
        softmax of the last forward's resident logits, all samples of that batch (fu_eval_prob_hist; target
        [last batch, H, W]).  probs: contiguous fp32 [..., k] on the device, e.g. merge_views' output, with target of its
        leading shape (fu_prob_hist).  Ignored / out-of-range targets are dropped as in eval_confusion."""
        from .calibration import check_bins
        n_bins = check_bins(n_bins)
        k = self.n_classes
        lib = _lib.load()
        if probs is None:
            B = self._last_batch
            if self._ctx is None or B == 0:
                raise RuntimeError("prob_histogram: no forward pass yet")
            H, W = self._ctx_key[1], self._ctx_key[2]
            target = target.contiguous().long()
            if tuple(target.shape) != (B, H, W):
                raise ValueError(f"prob_histogram: target must be [{B}, {H}, {W}] like the last forward, got "
                                 f"{tuple(target.shape)}")
        else:
            if probs.dim() < 2 or probs.shape[-1] != k or probs.dtype != torch.float32 or not probs.is_contiguous() \
                    or not probs.is_cuda:
                raise ValueError(f"prob_histogram: probs must be contiguous fp32 [..., {k}] on the GPU, got "
                                 f"{tuple(probs.shape)} {probs.dtype} on {probs.device}")
            target = target.contiguous().long()
            if tuple(target.shape) != tuple(probs.shape[:-1]) or target.device != probs.device or target.numel() == 0:
                raise ValueError(f"prob_histogram: target must be {tuple(probs.shape[:-1])} on {probs.device} and not empty, "
                                 f"got {tuple(target.shape)} on {target.device}")
        hist = torch.zeros(k, k, n_bins, dtype=torch.int64, device=target.device)
        top = torch.zeros(2, n_bins, dtype=torch.int64, device=target.device)
        if probs is None:
            check(lib.fu_eval_prob_hist(self._ctx, ptr(target), int(ignore_index), n_bins, ptr(hist), ptr(top),
                                        self._stream(target.device)))
        else:
            check(lib.fu_prob_hist(ptr(probs), ptr(target), target.numel(), k, int(ignore_index), n_bins, ptr(hist),
                                   ptr(top), self._stream(target.device)))
        return hist, top

    # ---------------------------------------------------------------- test-time augmentation
    def forward_views(self, x, codes, want_logits: bool = False) -> Optional[torch.Tensor]:
        """Eval forward of the T views `codes` (a tta.VIEW_SETS name or a list of view codes) of the B crops x (a tensor
        or a list of tensors side by side along C, as forward): ONE forward of T*B samples, sample v*B + b = view
        codes[v] of crop b, the views taken inside the input gather (fu_forward_views).  Returns the fp32 NCHW logits
        [T*B, k, H, W] when want_logits, else None (they stay resident for merge_views).  BatchNorm always uses the
        running statistics, whatever the module's mode."""
        from .tta import view_codes
        srcs, B, H, W, dev = self._sources(x)
        codes = view_codes(codes, H, W)
        T = len(codes)
        ctx = self._get_ctx(dev, T * B, H, W)
        lib = _lib.load()
        if self._eval_dirty:
            check(lib.fu_params_changed(ctx))
            self._eval_dirty = False
        logits = torch.empty(T * B, self.n_classes, H, W, dtype=torch.float32, device=dev) if want_logits else None
        arr = (C.c_void_p * len(srcs))(*[t.data_ptr() for t in srcs])
        chs = (C.c_int32 * len(srcs))(*[t.shape[1] for t in srcs])
        cds = (C.c_int32 * T)(*codes)
        check(lib.fu_forward_views(ctx, arr, chs, len(srcs), B, T, cds, ptr(logits), self._stream(dev)))
        self._last_batch = T * B
        self._views = (B, codes)
        return logits

    def merge_views(self, target: Optional[torch.Tensor] = None, ignore_index: int = -100, want_probs: bool = True):
        """After forward_views: -> (probs | None, counts | None).  probs: fp32 [B, H, W, k], the mean in view order of
        the inverse views of each view's softmax.  counts (with target int64 [B, H, W]): int64 [B, k, k] confusion counts
        of argmax probs, ignored / out-of-range targets dropped as in eval_confusion.  One launch (fu_merge_views)."""
        views = self._views
        if self._ctx is None or views is None:
            raise RuntimeError("merge_views: the last forward was not forward_views")
        if not want_probs and target is None:
            raise ValueError("merge_views: nothing to compute (want_probs=False and no target)")
        B, _ = views
        k, H, W = self.n_classes, self._ctx_key[1], self._ctx_key[2]
        dev = self._flat.device
        probs = torch.empty(B, H, W, k, dtype=torch.float32, device=dev) if want_probs else None
        counts = None
        if target is not None:
            target = target.contiguous().long()
            if tuple(target.shape) != (B, H, W) or target.device != dev:
                raise ValueError(f"merge_views: target must be [{B}, {H}, {W}] on {dev}, got {tuple(target.shape)} on "
                                 f"{target.device}")
            counts = torch.zeros(B, k, k, dtype=torch.int64, device=dev)
        check(_lib.load().fu_merge_views(self._ctx, ptr(probs), ptr(target), int(ignore_index), ptr(counts),
                                         self._stream(dev)))
        return probs, counts

    # ---------------------------------------------------------------- public API
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """logits = UNet(x).  Differentiable w.r.t. the parameters when grad mode is on and the module trains."""
        if self.training and torch.is_grad_enabled():
            params = [p for _, p, _, _ in self._table]
            return _UNetFn.apply(self, x, *params)
        return self._forward_raw(x, self.training)

    def loss(self, x: torch.Tensor, target: torch.Tensor, ignore_index: int,
             return_logits: bool = False, kind: str = "ce", dice_weight: float = 1.0, class_weight=None,
             label_smoothing: float = 0.0, focal_gamma: float = 0.0, region_weight: float = 0.0,
             region_alpha: float = 0.5, region_beta: float = 0.5, region_smooth: float = 1.0):
        """Fused forward + CrossEntropyLoss(ignore_index) (+ NaN guard) of water_seg_model.py:101-106
        (kind='ce', the reference's loss) or the BCE + soft-Dice extension (kind='bce_dice').
        kind='ce' also takes class_weight (n_classes finite values >= 0: a sequence or a tensor) and label_smoothing in
        [0, 1): nn.CrossEntropyLoss(weight, ignore_index, label_smoothing) in the fused kernels (fu_loss_ce_weighted), with
        loss 0 and a zero gradient where the summed weight of the valid pixels is 0.  focal_gamma > 0 (kind='ce', without
        label smoothing) multiplies every pixel's term by (1 - p[target])^focal_gamma, the focal loss of Lin et al.
        (fu_loss_ce_focal), normalised by the same summed weight.  region_weight > 0 (kind='ce') adds region_weight * R, the
        soft Tversky region term over all classes but ignore_index (fu_loss_ce_region): R = mean_k (1 - TI_k), TI_k =
        (I + s) / (I + region_alpha (P - I) + region_beta (T - I) + s) with s = region_smooth; alpha = beta = 0.5 is soft
        Dice, alpha = beta = 1 soft Jaccard; class weights do not enter it (last_region_terms() holds R and TI_k).  With all
        of them at their defaults the reference's loss runs exactly as before.
        The returned loss is differentiable: ``loss.backward()`` runs the HIP backward."""
        options = LossOptions.make(self.n_classes, kind, class_weight=class_weight, label_smoothing=label_smoothing,
                                   focal_gamma=focal_gamma, region_weight=region_weight, region_alpha=region_alpha,
                                   region_beta=region_beta, region_smooth=region_smooth)
        if self.training and torch.is_grad_enabled():
            params = [p for _, p, _, _ in self._table]
            out = _UNetLossFn.apply(self, x, target, int(ignore_index), bool(return_logits), kind, float(dice_weight),
                                    options, *params)
            return out if return_logits else out[0]
        logits = self._forward_raw(x, self.training, want_logits=return_logits)
        loss = self._loss_raw(target, ignore_index, _device_of(x), kind, dice_weight, options)
        return (loss, logits) if return_logits else loss

    def train_step(self, x: torch.Tensor, target: torch.Tensor, ignore_index: int, kind: str = "ce",
                   dice_weight: float = 1.0, class_weight=None, label_smoothing: float = 0.0,
                   focal_gamma: float = 0.0, region_weight: float = 0.0, region_alpha: float = 0.5,
                   region_beta: float = 0.5, region_smooth: float = 1.0) -> torch.Tensor:
        """forward + loss + backward without autograd; gradients land in the flat buffer / p.grad."""
        options = LossOptions.make(self.n_classes, kind, class_weight=class_weight, label_smoothing=label_smoothing,
                                   focal_gamma=focal_gamma, region_weight=region_weight, region_alpha=region_alpha,
                                   region_beta=region_beta, region_smooth=region_smooth)
        self._forward_raw(x, True, want_logits=False)
        loss = self._loss_raw(target, ignore_index, _device_of(x), kind, dice_weight, options)
        self._backward_raw(None, _device_of(x))
        self.attach_grads()
        return loss

    def flops_per_tile(self) -> Tuple[float, float]:
        f, t = C.c_double(), C.c_double()
        check(_lib.load().fu_flops_per_tile(self._ctx, C.byref(f), C.byref(t)))
        return f.value, t.value

    def block_ranges(self) -> List[Tuple[int, int]]:
        """(offset, numel) of each backward block's gradients in the flat buffer, in backward order."""
        lib = _lib.load()
        out = []
        o, n = C.c_int64(), C.c_int64()
        for b in range(lib.fu_num_blocks(self._ctx)):
            check(lib.fu_block_param_range(self._ctx, b, C.byref(o), C.byref(n)))
            out.append((o.value, n.value))
        return out


def check_class_weight(class_weight, n_classes: int):
    """Class weights of the weighted cross entropy -> numpy fp32 [n_classes], rounded from fp64 once.  ValueError unless
    they are n_classes finite numbers >= 0.  Host arithmetic only: the C call trusts the device copy it is given."""
    import numpy as np
    if isinstance(class_weight, torch.Tensor):
        class_weight = class_weight.detach().cpu().numpy()
    try:
        w = np.asarray(class_weight, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"class weights must be {n_classes} numbers, got {class_weight!r}") from e
    if w.ndim != 1 or w.shape[0] != int(n_classes):
        raise ValueError(f"class weights: expected {n_classes} values (one per class), got shape {tuple(w.shape)}")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError(f"class weights must be finite and >= 0, got {w.tolist()}")
    w32 = w.astype(np.float32)
    if not np.all(np.isfinite(w32)):
        raise ValueError(f"class weights must be finite in fp32, got {w.tolist()}")
    return w32


def _device_of(x):
    return (x[0] if isinstance(x, (list, tuple)) else x).device


def _check_generation(ctx):
    m = ctx.module
    if ctx.generation != m._generation:
        raise RuntimeError(
            "HipUNet: backward() of a forward pass that is no longer the latest training forward of this module. The "
            "saved activations live in the module's single device context (one forward in flight): call backward() "
            "before the next training forward.")


def _save_accumulated(m: "HipUNet"):
    """Before fu_backward overwrites the flat gradient buffer: if some p.grad ALIASES its slice of that buffer (the state
    the fast path of _return_param_grads leaves behind, also after zero_grad(set_to_none=False)), the values about to be
    overwritten are gradients autograd is expected to accumulate into -- keep a copy.  Returns (saved flat buffer or None,
    per-parameter alias flags)."""
    views = m.grad_views()
    alias = [p.grad is not None and p.grad.data_ptr() == v.data_ptr() for (_, p, _, _), v in zip(m._table, views)]
    return (m._flat_grad.clone() if any(alias) else None), alias


def _no_grads(forward) -> tuple:
    """One None per argument of an autograd Function's forward between ctx and *params: the module, the inputs, the options."""
    return (None,) * (forward.__code__.co_argcount - 1)


def _return_param_grads(m: "HipUNet", saved, alias):
    """Gradients of the HIP backward as autograd results.
    * p.grad is None (right after optimizer.zero_grad(set_to_none=True), what Lightning and torch >= 2.0 do): point p.grad at
      the parameter's slice of the flat gradient buffer the kernels have just written and hand autograd nothing to
      accumulate -- no 74 clones, no 74 accumulations, and HipAdam finds the gradients where fu_adam_step reads them.
    * p.grad aliases that slice (a second backward before the optimiser step: gradient accumulation): the kernels have just
      overwritten the accumulated value; add the saved copy back on the device, p.grad then holds old + new, and again
      nothing is returned for autograd to add (returning a clone here would make autograd add it INTO the aliased slice:
      2 * new instead of old + new).
    * p.grad lives elsewhere (set by the user): return a copy and let autograd accumulate into it."""
    views = m.grad_views()
    out = []
    for (_, p, off, n), v, al in zip(m._table, views, alias):
        if p.grad is None:
            p.grad = v
            out.append(None)
        elif al:
            v.add_(saved[off:off + n].view(p.shape))
            out.append(None)
        else:
            out.append(v.clone())
    return tuple(out)


class _UNetFn(torch.autograd.Function):
    """logits = f(x; params): forward through fu_forward, backward through fu_backward(dlogits)."""

    @staticmethod
    def forward(ctx, module: HipUNet, x, *params):
        ctx.module = module
        ctx.device = _device_of(x)
        out = module._forward_raw(x, True)
        ctx.generation = module._generation
        return out

    @staticmethod
    def backward(ctx, dlogits):
        m = ctx.module
        _check_generation(ctx)
        saved, alias = _save_accumulated(m)
        m._backward_raw(dlogits.contiguous().float(), ctx.device)
        return _no_grads(_UNetFn.forward) + _return_param_grads(m, saved, alias)


class _UNetLossFn(torch.autograd.Function):
    """(loss, logits) = CE(f(x; params), target): the fused training_step path."""

    @staticmethod
    def forward(ctx, module: HipUNet, x, target, ignore_index, want_logits, kind, dice_weight, options, *params):
        ctx.module = module
        ctx.device = _device_of(x)
        logits = module._forward_raw(x, True, want_logits=want_logits)
        ctx.generation = module._generation
        loss = module._loss_raw(target, ignore_index, ctx.device, kind, dice_weight, options)
        if logits is None:
            logits = torch.empty(0, device=ctx.device)
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        m = ctx.module
        _check_generation(ctx)
        # the upstream gradient of the loss (ones for a plain loss.backward()) scales dL/dlogits once, on the device
        dl = dloss.detach().reshape(()).to(device=ctx.device, dtype=torch.float32)
        check(_lib.load().fu_scale_loss_grad(m._ctx, ptr(dl), m._stream(ctx.device)))
        saved, alias = _save_accumulated(m)
        m._backward_raw(None, ctx.device)
        return _no_grads(_UNetLossFn.forward) + _return_param_grads(m, saved, alias)
