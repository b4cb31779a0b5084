"""GPU: decoupled weight decay (AdamW) inside the fused Adam step -- the decayed step against "multiply the flagged slices,
then the plain kernel" bit for bit on all four entry points, against torch.optim.AdamW on the CPU, skipped steps, with
clipping armed, the captured-graph form, HipAdam / WaterSegmentationModel / DataParallelTrainer, and fit end to end.  Every
comparison is of bits unless it says otherwise."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd.ema import ema_weight
from floodplanet_code_amd.unet import HipAdam, HipUNet
from oracle import unet_oracle as O
from tools import adamw_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETAS, EPS = (0.9, 0.999), 1e-8
WD = 0.05


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _lr(step):
    """A learning rate that changes with every step (as under a schedule)."""
    return 1e-3 * (1.0 + 0.5 * float(np.cos(step))) * (0.5 if step % 3 == 0 else 1.0)


def _clip_state(lib, ctx):
    norm, coef = C.c_float(), C.c_float()
    n, k, bad = C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(lib.fu_grad_clip_state(ctx, C.byref(norm), C.byref(coef), C.byref(n), C.byref(k), C.byref(bad)))
    return dict(norm=np.float32(norm.value), coef=np.float32(coef.value), steps=n.value, clipped=k.value, nonfinite=bad.value)


def _dev_scalars(lib, ema, step, lr, gscale, w, wd):
    """The caller's device scalars of the _dev forms: nine floats with decay (fu_adamw_scalars), else seven or eight."""
    buf = (C.c_float * 9)()
    if wd is not None:
        _lib.check(lib.fu_adamw_scalars(lr, *BETAS, EPS, step, float(gscale), w if ema else 0.0, wd, buf))
        n = 9
    elif ema:
        _lib.check(lib.fu_adam_ema_scalars(lr, *BETAS, EPS, step, float(gscale), w, buf))
        n = 8
    else:
        _lib.check(lib.fu_adam_scalars(lr, *BETAS, EPS, step, float(gscale), buf))
        n = 7
    return torch.tensor(list(buf)[:n], dtype=torch.float32, device=DEV)


def _call(lib, ctx, entry, step, lr, gscale, w, stream, wd=None):
    """One optimiser step through `entry`; wd: the armed decay (the _dev forms then hand over nine scalars), None: disarmed.
    Returns the caller's device scalars (the _dev forms) or None."""
    if entry == "step":
        _lib.check(lib.fu_adam_step(ctx, lr, *BETAS, EPS, step, float(gscale), stream))
    elif entry == "ema_step":
        _lib.check(lib.fu_adam_ema_step(ctx, lr, *BETAS, EPS, step, float(gscale), w, stream))
    else:
        sc = _dev_scalars(lib, entry == "ema_step_dev", step, lr, gscale, w, wd)
        fn = lib.fu_adam_ema_step_dev if entry == "ema_step_dev" else lib.fu_adam_step_dev
        _lib.check(fn(ctx, sc.data_ptr(), stream))
        return sc
    return None


class _Bound:
    """Two sets of caller-bound flat buffers on one context, `shift` floats past a 16-byte boundary (a local copy of the
    helper of tests/test_gpu_grad_clip.py): [0] takes the decayed step, [1] a copy of the same inputs for the step it is
    compared with."""

    def __init__(self, cin, base, shift, seed, prec="fp32"):
        self.lib = _lib.load()
        self.net = HipUNet(cin, 3, base_channels=base, precision=prec).to(DEV).train()
        self.ctx = self.net._get_ctx(torch.device(DEV), 1, 64, 64)
        self.n, self.nb, self.shift = self.net._total, self.net._total_bn, shift
        self.gen = torch.Generator(device=DEV).manual_seed(seed)
        self.stream = self.net._stream(torch.device(DEV))
        p0 = torch.randn(self.n, device=DEV, generator=self.gen) * 0.1
        self.nbt = torch.zeros(len(self.net._bn), dtype=torch.int64, device=DEV)
        self.sets = []
        for _ in range(2):
            s = dict(p=self.buf(self.n, p0), g=self.buf(self.n), m=self.buf(self.n), v=self.buf(self.n), rm=self.buf(self.nb),
                     rv=self.buf(self.nb), ep=self.buf(self.n, p0 * 0.5), erm=self.buf(self.nb), erv=self.buf(self.nb))
            s["rm"].normal_(generator=self.gen)
            s["rv"].uniform_(0.5, 1.5, generator=self.gen)
            self.sets.append(s)
        for k in ("rm", "rv"):
            self.sets[1][k].copy_(self.sets[0][k])
        self.table = [(off, cnt) for _, _, off, cnt in self.net._table]
        self.ndim = [p.ndim for _, p, _, _ in self.net._table]

    def buf(self, count, init=None):
        t = torch.zeros(count + 8 + self.shift, dtype=torch.float32, device=DEV)[self.shift:self.shift + count]
        assert t.data_ptr() % 16 == (4 * self.shift) % 16
        if init is not None:
            t.copy_(init)
        return t

    def mask(self, kind, seed=0):
        if kind == "default":
            return None, [d >= 2 for d in self.ndim]
        if kind == "all":
            flags = [True] * len(self.table)
        elif kind == "none":
            flags = [False] * len(self.table)
        else:
            flags = (np.random.default_rng(seed).random(len(self.table)) < 0.5).tolist()
        return (C.c_uint8 * len(flags))(*[int(f) for f in flags]), flags

    def bind(self, k, wd=0.0, cmask=None, max_norm=0.0):
        lib, ctx, s = self.lib, self.ctx, self.sets[k]
        _lib.check(lib.fu_bind_buffers(ctx, s["p"].data_ptr(), s["g"].data_ptr(), s["rm"].data_ptr(), s["rv"].data_ptr(),
                                       self.nbt.data_ptr()))
        _lib.check(lib.fu_bind_adam_state(ctx, s["m"].data_ptr(), s["v"].data_ptr()))
        _lib.check(lib.fu_bind_ema_state(ctx, s["ep"].data_ptr(), s["erm"].data_ptr(), s["erv"].data_ptr()))
        _lib.check(lib.fu_set_grad_clip(ctx, max_norm))
        _lib.check(lib.fu_set_weight_decay(ctx, wd, cmask, 0 if cmask is None else len(self.table)))

    def decay_on_device(self, k, flags, lr, wd):
        """The flagged tensors' slices times float32(1 - lr * wd), with torch: one fp32 multiply per element."""
        d = float(adamw_ref.decay_factor(lr, wd))
        for (off, cnt), f in zip(self.table, flags):
            if f:
                self.sets[k]["p"][off:off + cnt].mul_(d)

    def same_state(self, ema):
        a, b = self.sets
        keys = ("p", "m", "v") + (("ep", "erm", "erv") if ema else ())
        return [k for k in keys if not _same(a[k], b[k])]

    def armed(self):
        wd = C.c_double()
        out = (C.c_uint8 * len(self.table))()
        _lib.check(self.lib.fu_weight_decay_state(self.ctx, C.byref(wd), out, len(self.table)))
        return wd.value, [bool(v) for v in out]

    def close(self):
        _lib.check(self.lib.fu_set_grad_clip(self.ctx, 0.0))
        _lib.check(self.lib.fu_set_weight_decay(self.ctx, 0.0, None, 0))
        _lib.check(self.lib.fu_bind_ema_state(self.ctx, None, None, None))
        self.net._bind(self.ctx)


# ------------------------------------------------------------------------------------------------------------ 1. the step on bound buffers
CASES = [
    # cin, base, shift, entry, mask: (3, 8) has a total that is no multiple of 4 (a scalar tail); shifts 1 and 3 make the
    # 16-byte groups straddle tensor boundaries; (4, 8) is the aligned case; (8, 64) the grid-stride loop
    (3, 8, 0, "step", "default"), (3, 8, 1, "step_dev", "default"), (3, 8, 3, "ema_step", "default"),
    (3, 8, 1, "ema_step_dev", "default"), (4, 8, 0, "step_dev", "default"), (4, 8, 0, "ema_step", "all"),
    (3, 8, 3, "step", "all"), (3, 8, 1, "ema_step_dev", "all"), (3, 8, 1, "step", "random"), (3, 8, 3, "step_dev", "random"),
    (4, 8, 0, "ema_step_dev", "random"), (3, 8, 3, "ema_step", "random"), (3, 8, 0, "step_dev", "random"),
    (3, 8, 1, "step", "none"), (3, 8, 3, "ema_step_dev", "none"), (4, 8, 0, "step_dev", "none"), (3, 8, 0, "ema_step", "none"),
    (8, 64, 1, "ema_step_dev", "default"),
]


@pytest.mark.parametrize("cin,base,shift,entry,mask", CASES)
def test_decayed_step_is_decay_followed_by_the_plain_kernel(cin, base, shift, entry, mask):
    """5 steps with gradients randn * 10^(step % 4 - 2) and an lr that changes with every step.  Set [0] takes the armed step;
    on set [1] the flagged tensors' slices are multiplied by float32(1 - lr * wd) with torch on the device and the same
    entry point runs with decay disarmed: parameters, both moments and (EMA forms) the three averages are bit-identical.
    The gradient buffer and the caller's device scalars are only read.  Mask `none` arms the decay with no tensor flagged:
    the step is the plain step on 7 (8) caller scalars -- the launch it issues is checked in the captured-graph test."""
    B = _Bound(cin, base, shift, 600 + cin + shift)
    lib, ctx = B.lib, B.ctx
    if (cin, base) == (3, 8):
        assert B.n % 4 != 0                                             # a scalar tail
    ema = entry.startswith("ema")
    cmask, flags = B.mask(mask, seed=cin + shift)
    if shift and mask in ("default", "random"):                         # a decayed range that starts or ends inside a group
        edges = [e for (off, cnt), f in zip(B.table, flags) if f for e in (off, off + cnt)]
        assert any((e - (4 - shift) % 4) % 4 for e in edges)
    try:
        for step in range(1, 6):
            lr = _lr(step)
            grad = torch.randn(B.n, device=DEV, generator=B.gen) * (10.0 ** float(step % 4 - 2))
            w = ema_weight(0.999, step)
            for s in B.sets:
                s["g"].copy_(grad)
            B.bind(0, WD, cmask)
            assert B.armed() == (WD, flags)
            sc = _call(lib, ctx, entry, step, lr, 0.5, w, B.stream, wd=None if mask == "none" else WD)
            sc0 = None if sc is None else sc.clone()
            B.bind(1)
            assert B.armed() == (0.0, [False] * len(flags))
            B.decay_on_device(1, flags, lr, WD)
            _call(lib, ctx, entry, step, lr, 0.5, w, B.stream)
            torch.cuda.synchronize()
            assert B.same_state(ema) == [], (step, B.same_state(ema))
            assert torch.equal(B.sets[0]["g"], grad)                    # inputs only read
            if sc is not None:
                assert _same(sc, sc0)
            if not ema:                                                 # the plain forms leave the bound averages alone
                assert not B.sets[0]["ep"].ne(B.sets[1]["ep"]).any()
    finally:
        B.close()


def test_decay_acts_only_on_the_flagged_tensors_and_never_on_the_moments():
    """One armed and one disarmed step from the same state with a zero gradient: Adam's own update is then exactly zero
    (m = v = 0, p + 0 / eps), so flagged tensors come out as p * float32(1 - lr * wd), every other element and both moments
    unchanged -- per element across the straddled groups of shift 3."""
    B = _Bound(3, 8, 3, 700)
    try:
        cmask, flags = B.mask("random", seed=5)
        p0 = B.sets[0]["p"].clone()
        B.bind(0, WD, cmask)
        _call(B.lib, B.ctx, "step", 1, 1e-2, 1.0, 0.0, B.stream)
        torch.cuda.synchronize()
        d = float(adamw_ref.decay_factor(1e-2, WD))
        for (off, cnt), f in zip(B.table, flags):
            want = p0[off:off + cnt] * d if f else p0[off:off + cnt]
            assert _same(B.sets[0]["p"][off:off + cnt], want), (off, cnt, f)
        assert not B.sets[0]["m"].any() and not B.sets[0]["v"].any()
    finally:
        B.close()


def test_bad_arguments_on_a_live_context():
    B = _Bound(3, 8, 0, 710)
    try:
        lib, ctx, n = B.lib, B.ctx, len(B.table)
        cmask, flags = B.mask("all")
        for bad in (-1e-3, float("nan"), float("inf")):
            assert lib.fu_set_weight_decay(ctx, bad, None, 0) == _lib.FU_ERR_INVALID
        assert lib.fu_set_weight_decay(ctx, 0.01, cmask, n - 1) == _lib.FU_ERR_INVALID
        assert lib.fu_weight_decay_state(ctx, None, (C.c_uint8 * (n + 1))(), n + 1) == _lib.FU_ERR_INVALID
        assert B.armed() == (0.0, [False] * n)                          # a rejected call arms nothing
        _lib.check(lib.fu_set_weight_decay(ctx, 0.01, None, 0))
        assert B.armed() == (0.01, [d >= 2 for d in B.ndim])            # the default rule
        assert lib.fu_num_params(ctx) == n
    finally:
        B.close()


# ------------------------------------------------------------------------------------------------------------ 2. against torch on the CPU
def _cpu_optim(p0, table, shapes, flags, wd):
    params = [torch.nn.Parameter(p0[off:off + n].clone().view(s)) for (off, n), s in zip(table, shapes)]
    groups = [{"params": [p for p, f in zip(params, flags) if f], "weight_decay": wd},
              {"params": [p for p, f in zip(params, flags) if not f], "weight_decay": 0.0}]
    cls = torch.optim.AdamW if wd > 0 else torch.optim.Adam
    return params, cls([g for g in groups if g["params"]], lr=1e-3, betas=BETAS, eps=EPS, foreach=False)


def test_decayed_step_is_no_further_from_torch_adamw_than_the_plain_step_from_torch_adam():
    """The same 5 steps through torch.optim.Adam / torch.optim.AdamW(foreach=False) on the CPU, per tensor, two groups.  The
    tolerance is measured, not fixed: gap_plain = max |device - torch| of fu_adam_step against Adam over parameters and
    moments -- the device's sqrt / divide against the host's -- and the decayed step must be no further from AdamW.
    Measured on an MI355X: both gaps 1.192e-07, one ulp of a value in [1, 2); on the way the statement
    tests/tools/adamw_ref.py is checked to give torch's bits here too."""
    B = _Bound(3, 8, 1, 800)
    try:
        cmask, flags = B.mask("default")
        shapes = [tuple(p.shape) for _, p, _, _ in B.net._table]
        p0 = B.sets[0]["p"].cpu().clone()
        gaps = {}
        for name, k, wd in (("plain", 1, 0.0), ("decayed", 0, WD)):
            params, opt = _cpu_optim(p0, B.table, shapes, flags, wd)
            ref = [p0.clone(), torch.zeros(B.n), torch.zeros(B.n)]
            gen = torch.Generator(device=DEV).manual_seed(801)
            gap = 0.0
            for step in range(1, 6):
                lr = _lr(step)
                grad = torch.randn(B.n, device=DEV, generator=gen) * (10.0 ** float(step % 4 - 2))
                B.sets[k]["g"].copy_(grad)
                B.bind(k, wd, cmask if wd else None)
                _call(B.lib, B.ctx, "step", step, lr, 1.0, 0.0, B.stream)
                g_host = grad.cpu()
                for q, (off, n) in zip(params, B.table):
                    q.grad = g_host[off:off + n].view(q.shape).clone()
                for group in opt.param_groups:
                    group["lr"] = lr
                opt.step()
                adamw_ref.step_flat(*ref[:1], g_host, *ref[1:], B.table, flags, lr, BETAS, EPS, step, wd)
                torch.cuda.synchronize()
                want = [torch.cat([q.detach().reshape(-1) for q in params]),
                        torch.cat([opt.state[q]["exp_avg"].reshape(-1) for q in params]),
                        torch.cat([opt.state[q]["exp_avg_sq"].reshape(-1) for q in params])]
                for r, t in zip(ref, want):
                    assert _same(r, t)                                  # the statement is torch, here too
                for key, t in zip(("p", "m", "v"), want):
                    gap = max(gap, adamw_ref.max_abs_diff(B.sets[k][key].cpu(), t))
            gaps[name] = gap
        print(f"max |device - torch cpu| over 5 steps: plain Adam {gaps['plain']:.3e}, decayed AdamW {gaps['decayed']:.3e}")
        assert gaps["decayed"] <= gaps["plain"], gaps
    finally:
        B.close()


# ------------------------------------------------------------------------------------------------------------ 3. skipped steps
@pytest.mark.parametrize("prec,bad,clip", [("fp16", float("inf"), None), ("fp32", float("nan"), 1.0)])
def test_a_skipped_step_skips_the_decay_too(prec, bad, clip):
    """Decay armed; an fp16 step with an inf gradient (the guard), a clipped fp32 step with a NaN norm: parameters, moments
    and averages stay bit-unchanged.  The next, finite step is applied exactly as on a twin that never saw the bad one."""
    nets = []
    for _ in range(2):
        net = HipUNet(4, 3, base_channels=8, precision=prec)
        net.load_state_dict(O.make_state(4, 3, 8, True, seed=3))
        net.to(DEV).train()
        net._get_ctx(torch.device(DEV), 2, 64, 64)
        net.enable_ema(0.9, warmup=False)
        net.set_grad_clip(clip)
        net.set_weight_decay(WD)
        for e in net.ema_buffers():
            e.mul_(0.5).add_(0.25)                                      # an update that ran would show
        nets.append(net)
    net, twin = nets
    state = lambda m: (m.flat_parameters(), *m.adam_state(), *m.ema_buffers())                 # noqa: E731
    g = torch.Generator(device=DEV).manual_seed(5)
    before = [t.clone() for t in state(net)]
    net.flat_grads().normal_(generator=g)
    net.flat_grads()[net._total // 2 + 1] = bad
    net.adam_step(1e-2, 1)
    torch.cuda.synchronize()
    for a, b in zip(state(net), before):
        assert _same(a, b)                                              # skipped, the decay with it
    if prec == "fp16":
        assert net.fp16_guard_state()[0] == 1
    else:
        assert net.grad_clip_state()["nonfinite_steps"] == 1
    clean = torch.randn(net._total, device=DEV, generator=g) * 0.1
    for m in nets:
        m.flat_grads().copy_(clean)
        m.adam_step(1e-2, 2)
    torch.cuda.synchronize()
    assert not _same(net.flat_parameters(), before[0])
    for a, b in zip(state(net), state(twin)):
        assert _same(a, b)
    # and the decay is in that step: without it the parameters come out different
    plain = HipUNet(4, 3, base_channels=8, precision=prec)
    plain.load_state_dict(O.make_state(4, 3, 8, True, seed=3))
    plain.to(DEV).train()
    plain._get_ctx(torch.device(DEV), 2, 64, 64)
    plain.set_grad_clip(clip)
    plain.flat_grads().copy_(clean)
    plain.adam_step(1e-2, 2)
    torch.cuda.synchronize()
    assert not _same(plain.flat_parameters(), net.flat_parameters())


# ------------------------------------------------------------------------------------------------------------ 4. with clipping armed
@pytest.mark.parametrize("shift,entry", [(1, "step_dev"), (3, "ema_step"), (0, "step"), (1, "ema_step_dev")])
def test_clipped_decayed_step_is_the_unclipped_decayed_step_at_the_clip_coefficient(shift, entry):
    """Clip + decay armed on set [0]; set [1] takes the armed, unclipped step at grad_scale = float32(gscale) *
    float32(last_coef): bit-identical state.  fu_grad_clip_state is what it is without decay: the same step repeated from
    the same inputs with decay disarmed leaves the same norm and coefficient."""
    B = _Bound(3, 8, shift, 900 + shift)
    lib, ctx = B.lib, B.ctx
    ema = entry.startswith("ema")
    cmask, flags = B.mask("default")
    try:
        n_clipped = 0
        for step in range(1, 5):
            lr, gscale, w = _lr(step), 0.5, ema_weight(0.999, step)
            grad = torch.randn(B.n, device=DEV, generator=B.gen) * (10.0 ** float(step % 4 - 3))
            for s in B.sets:
                s["g"].copy_(grad)
            snap = {k: B.sets[0][k].clone() for k in ("p", "m", "v", "ep", "erm", "erv")}
            B.bind(0, WD, cmask, max_norm=1.0)
            sc = _call(lib, ctx, entry, step, lr, gscale, w, B.stream, wd=WD)
            st = _clip_state(lib, ctx)                                  # synchronises
            if sc is not None:
                assert float(sc[6]) == np.float32(gscale)               # the caller's scalars still hold the pre-clip scale
                assert float(sc[8]) == adamw_ref.decay_factor(lr, WD)
            n_clipped += int(st["coef"] < 1)
            B.bind(1, WD, cmask)
            prod = float(np.float32(gscale) * st["coef"])
            _call(lib, ctx, entry, step, lr, prod, w, B.stream, wd=WD)
            torch.cuda.synchronize()
            assert B.same_state(ema) == [], (step, B.same_state(ema))
            # the clip state without decay, from the same inputs
            after = {k: B.sets[0][k].clone() for k in snap}
            for k, t in snap.items():
                B.sets[0][k].copy_(t)
            B.bind(0, 0.0, None, max_norm=1.0)
            _call(lib, ctx, entry, step, lr, gscale, w, B.stream)
            st2 = _clip_state(lib, ctx)
            assert st2["norm"].tobytes() == st["norm"].tobytes() and st2["coef"].tobytes() == st["coef"].tobytes()
            assert (st2["steps"], st2["nonfinite"]) == (st["steps"] + 1, 0)
            for k, t in after.items():
                B.sets[0][k].copy_(t)
        assert 0 < n_clipped < 4                                        # both kinds of step occurred
    finally:
        B.close()


# ------------------------------------------------------------------------------------------------------------ 5. through the net
def _net(prec="fp32", seed=7, st=None):
    net = HipUNet(8, 3, base_channels=16, precision=prec)
    net.load_state_dict(st if st is not None else O.make_state(8, 3, 16, True, seed=seed))
    return net.to(DEV).train()


def _batch(seed):
    b = O.make_batch(2, 8, 64, 64, seed=seed)
    return b["image"].to(DEV), b["target"].to(DEV)


def _kernel_nodes(path):
    return [l for l in open(path).read().splitlines() if "_ZN2fu" in l]


def _count(nodes, name):
    return len([l for l in nodes if name + "E" in l])                   # the mangled name: <len><name>E<arguments>


@pytest.mark.parametrize("ema", [None, 0.9])
def test_graph_trainer_equals_eager_with_the_same_number_of_kernel_nodes(ema, tmp_path, monkeypatch):
    """DataParallelTrainer(graph=True, weight_decay=) with an lr that changes every step equals the eager trainer bit for bit
    over 4 steps (and a single-rank exact-mode trainer does), with and without a weight EMA.  The captured graph holds as
    many kernel nodes as the one captured without decay, k_adamw[_ema]_dev in the place of k_adam[_ema]_dev; armed with no
    tensor flagged it holds exactly the nodes of the plain graph."""
    from floodplanet_code_amd.distributed import DataParallelTrainer
    st = O.make_state(8, 3, 16, True, seed=7)
    host = [O.make_batch(2, 8, 64, 64, seed=90 + i) for i in range(3)]
    outs, dots = {}, {}
    for tag, graph, wd, exact in (("eager", False, WD, False), ("exact", False, WD, True), ("graph", True, WD, False),
                                  ("plain", True, 0.0, False), ("empty", True, WD, False)):
        net = _net("bf16", st=st)
        if graph:
            dots[tag] = str(tmp_path / f"step_{tag}_{ema}.dot")
            monkeypatch.setenv("FU_GRAPH_DOT", dots[tag])
        else:
            monkeypatch.delenv("FU_GRAPH_DOT", raising=False)
        tr = DataParallelTrainer(net, lr=1e-2, graph=graph, weight_decay=wd, exact=exact, ema_decay=ema)
        if tag == "empty":
            net.set_weight_decay(wd, [])
        losses = []
        for it in range(4):
            tr.lr = 1e-2 * _lr(it + 1) / 1e-3
            b = host[it % 3]
            losses.append(tr.step(b["image"].to(DEV), b["target"].to(DEV), 0))
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph
        outs[tag] = ([l.item() for l in losses], net.flat_parameters().clone(), *[t.clone() for t in net.adam_state()],
                     *([t.clone() for t in net.ema_buffers()] if ema else []))
    for other in ("exact", "graph"):
        assert outs["eager"][0] == outs[other][0] and len(set(outs[other][0])) > 1
        for a, b in zip(outs["eager"][1:], outs[other][1:]):
            assert _same(a, b), other
    assert not _same(outs["graph"][1], outs["plain"][1])            # the decay acted
    for a, b in zip(outs["empty"][1:], outs["plain"][1:]):
        assert _same(a, b)                                          # no tensor flagged: the plain step
    armed, plain, empty = (_kernel_nodes(dots[k]) for k in ("graph", "plain", "empty"))
    old, new = ("k_adam_ema_dev", "k_adamw_ema_dev") if ema else ("k_adam_dev", "k_adamw_dev")
    assert len(armed) == len(plain) == len(empty) > 12
    assert (_count(armed, new), _count(armed, old)) == (1, 0)
    assert (_count(plain, new), _count(plain, old)) == (_count(empty, new), _count(empty, old)) == (0, 1)
    assert not [l for l in plain + empty if "k_adamw" in l]


def test_a_change_of_the_setting_after_capture_captures_again():
    from floodplanet_code_amd.distributed import DataParallelTrainer
    st = O.make_state(8, 3, 16, True, seed=7)
    x, t = _batch(95)
    a, b = _net("bf16", st=st), _net("bf16", st=st)
    tra = DataParallelTrainer(a, lr=1e-2, graph=True, weight_decay=WD)
    trb = DataParallelTrainer(b, lr=1e-2, graph=False, weight_decay=WD)
    for it in range(4):
        if it == 2:
            first = tra._graph
            a.set_weight_decay(2 * WD, "all")
            b.set_weight_decay(2 * WD, "all")
        tra.step(x, t, 0)
        trb.step(x, t, 0)
    torch.cuda.synchronize()
    assert first is not None and tra._graph is not first and tra._g_optim[2] == (2 * WD, (True,) * len(a._table))
    assert _same(a.flat_parameters(), b.flat_parameters())


def test_ema_clipping_and_decay_together_graph_equals_eager():
    """The weight EMA, gradient clipping and weight decay armed together on one DataParallelTrainer: the captured step equals
    the eager one bit for bit over 4 steps with a changing lr -- losses, parameters, both moments, the three EMA buffers and
    the clip state.  The clip norm lies between the smallest and the largest gradient norm of an unclipped eager run, and
    the test asserts that it clipped some of the four steps and not all."""
    from floodplanet_code_amd.distributed import DataParallelTrainer
    st = O.make_state(8, 3, 8, True, seed=11)
    host = [O.make_batch(2, 8, 32, 32, seed=70 + i) for i in range(4)]

    def run(graph, clip):
        net = HipUNet(8, 3, base_channels=8, precision="bf16")
        net.load_state_dict(st)
        net.to(DEV).train()
        tr = DataParallelTrainer(net, lr=1e-2, graph=graph, ema_decay=0.9, grad_clip_norm=clip, weight_decay=WD)
        losses, norms = [], []
        for it, b in enumerate(host):
            tr.lr = 1e-2 * _lr(it + 1) / 1e-3
            losses.append(tr.step(b["image"].to(DEV), b["target"].to(DEV), 0))
            if clip > 1e29:
                norms.append(net.grad_clip_state()["grad_norm"])
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph
        return ([l.item() for l in losses], net.flat_parameters().clone(), *[t.clone() for t in net.adam_state()],
                *[t.clone() for t in net.ema_buffers()]), net.grad_clip_state(), norms

    _, unclipped, norms = run(False, 1e30)
    assert unclipped["clipped_steps"] == 0 and len(norms) == 4 and min(norms) < max(norms)
    clip = 0.5 * (min(norms) + max(norms))
    eager, eager_state, _ = run(False, clip)
    graph, graph_state, _ = run(True, clip)
    print(f"gradient norms of the unclipped run {norms}, clip norm {clip}, clip state {eager_state}")
    assert 0 < eager_state["clipped_steps"] < 4 and eager_state["steps"] == 4 and eager_state["nonfinite_steps"] == 0
    assert eager_state == graph_state
    assert eager[0] == graph[0] and len(set(eager[0])) > 1
    assert len(eager) == 1 + 1 + 2 + 3
    for a, b in zip(eager[1:], graph[1:]):
        assert _same(a, b)


def test_late_fusion_takes_the_setting():
    """HipLateFusion (two encoders, the fusion convs: a longer parameter table) through HipUNet.set_weight_decay / adam_step:
    the armed step equals the flagged slices times float32(d) followed by the disarmed step on a twin."""
    from floodplanet_code_amd.latefusion import HipLateFusion
    nets = []
    for _ in range(2):
        torch.manual_seed(3)
        net = HipLateFusion({"ms_image": 5, "dem": 3}, 3, base_channels=8).to(DEV).train()
        net._get_ctx(torch.device(DEV), 2, 32, 32)
        nets.append(net)
    a, b = nets
    assert _same(a.flat_parameters(), b.flat_parameters())
    a.set_weight_decay(WD)
    names = a.decayed_parameter_names()
    assert names == [k for k, p in a.named_parameters() if p.ndim >= 2] and len(names) > 19
    g = torch.Generator(device=DEV).manual_seed(4)
    for step in (1, 2):
        grad = torch.randn(a._total, device=DEV, generator=g) * 0.1
        d = float(adamw_ref.decay_factor(_lr(step), WD))
        for name, p, off, n in b._table:
            if p.ndim >= 2:
                b.flat_parameters()[off:off + n].mul_(d)
        for net in nets:
            net.flat_grads().copy_(grad)
            net.adam_step(_lr(step), step)
    torch.cuda.synchronize()
    assert _same(a.flat_parameters(), b.flat_parameters()) and _same(a.adam_state()[0], b.adam_state()[0])


# ------------------------------------------------------------------------------------------------------------ 6. HipAdam, the model, fit
def test_hipadam_and_the_model_take_the_trainer_steps_and_the_state_round_trips():
    """Three Lightning-style steps through HipAdam(weight_decay=0.01) and through WaterSegmentationModel(weight_decay=0.01)
    equal DataParallelTrainer(weight_decay=0.01)'s on the parameters, bit for bit, the lr changed in param_groups before
    every step; the optimiser's state_dict carries the setting into a fresh optimiser, which then takes the same fourth
    step; a manual change of param_groups[0]['weight_decay'] reaches the module."""
    from floodplanet_code_amd.distributed import DataParallelTrainer
    from floodplanet_code_amd.models import WaterSegmentationModel
    st = O.make_state(8, 3, 16, True, seed=8)
    batches = [_batch(80 + i) for i in range(4)]
    a = _net(st=st)
    tr = DataParallelTrainer(a, lr=1e-3, weight_decay=0.01)
    plain = _net(st=st)
    trp = DataParallelTrainer(plain, lr=1e-3)
    b = _net(st=st)
    opt = HipAdam(b, lr=1e-3, weight_decay=0.01)
    model = WaterSegmentationModel({"ms_image": 8}, 3, 1e-3, ignore_index=0, base_channels=16, weight_decay=0.01)
    model.model.load_state_dict(st)
    model = model.to(DEV)
    mopt = model.configure_optimizers()
    assert isinstance(mopt, HipAdam) and mopt.param_groups[0]["weight_decay"] == 0.01

    def lightning_step(net_loss, optimizer, x, t, lr):
        optimizer.param_groups[0]["lr"] = lr
        optimizer.zero_grad()
        net_loss(x, t).backward()
        optimizer.step()

    for it in range(3):
        x, t = batches[it]
        tr.lr = trp.lr = _lr(it + 1)
        tr.step(x, t, 0)
        trp.step(x, t, 0)
        lightning_step(lambda x, t: b.loss(x, t, 0), opt, x, t, _lr(it + 1))
        lightning_step(lambda x, t: model.training_step({"image": x, "target": t}, 0), mopt, x, t, _lr(it + 1))
    torch.cuda.synchronize()
    assert _same(a.flat_parameters(), b.flat_parameters()) and _same(a.flat_parameters(), model.model.flat_parameters())
    assert not _same(a.flat_parameters(), plain.flat_parameters())      # the decay acted
    # the round trip: a fresh module and optimiser, without the setting, take it from the state_dict
    sd = opt.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 0.01 and sd["decay_params"] == b.decayed_parameter_names()
    c = _net(st=st)
    c.load_state_dict(b.state_dict())
    c._get_ctx(torch.device(DEV), 2, 64, 64)
    opt2 = HipAdam(c, lr=5e-4)
    assert c.weight_decay == 0.0
    opt2.load_state_dict(sd)
    assert c.weight_decay == 0.01 and c.decayed_parameter_names() == b.decayed_parameter_names()
    assert opt2.param_groups[0]["weight_decay"] == 0.01 and opt2._step == 3
    x, t = batches[3]
    lightning_step(lambda x, t: b.loss(x, t, 0), opt, x, t, _lr(4))
    lightning_step(lambda x, t: c.loss(x, t, 0), opt2, x, t, _lr(4))
    torch.cuda.synchronize()
    assert _same(b.flat_parameters(), c.flat_parameters()) and _same(b.adam_state()[1], c.adam_state()[1])
    opt.param_groups[0]["weight_decay"] = 0.0                           # a manual change is read by the next step
    lightning_step(lambda x, t: b.loss(x, t, 0), opt, x, t, _lr(5))
    assert b.weight_decay == 0.0 and b.decayed_parameter_names() == []
    # another tile shape: a new context takes the module's setting
    small = O.make_batch(2, 8, 32, 32, seed=81)
    old = c._ctx_key
    c.train_step(small["image"].to(DEV), small["target"].to(DEV), 0)
    assert c._ctx_key != old
    wd = C.c_double()
    _lib.check(_lib.load().fu_weight_decay_state(c._ctx, C.byref(wd), None, 0))
    assert wd.value == 0.01


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from tools.tiff_writer import make_floodplanet_tree
    root = str(tmp_path_factory.mktemp("tree"))
    make_floodplanet_tree(root, regions=("RegA", "RegB"), images_per_region=2, label_size=100, s1_size=40)
    return root


def _fit_args(root, exp, extra=()):
    return [root, "--exp_dir", exp, "--sensor", "S1", "--eval_region", "RegB", "--crop", "64", "64", "--stride", "32",
            "--batch_size", "4", "--n_epochs", "2", "--lr", "2e-3", "--base_channels", "8", "--loader", "scene",
            "--n_workers", "0", "--seed", "0", "--save_topk_models", "2", "--device", DEV, *extra]


def test_fit_with_weight_decay_and_a_schedule(tree, tmp_path, capsys):
    """Two epochs of fit --weight_decay 0.01 --lr_schedule cosine: the run records the setting and the number of decayed
    tensors, the checkpoint carries it and serves predict; a decayed conv weight's norm ends smaller than in the same run
    without decay (a comparison of the two runs, not of bits), whose history has the keys it always had."""
    from floodplanet_code_amd import fit, predict
    out = fit.main(_fit_args(tree, str(tmp_path / "wd"), ("--weight_decay", "0.01", "--lr_schedule", "cosine")))
    net = fit.fit_model.last_model.model
    n_decayed = len([p for p in net.parameters() if p.ndim >= 2])
    assert (out["weight_decay"], out["decayed_tensors"]) == (0.01, n_decayed) and 0 < n_decayed < len(net._table)
    for h in out["history"]:
        assert (h["weight_decay"], h["decayed_tensors"]) == (0.01, n_decayed) and np.isfinite(h["train_loss"])
    ckpt = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)
    kw = ckpt["hyper_parameters"]["model"]["model_kwargs"]
    assert kw["weight_decay"] == 0.01 and "decay_all" not in kw and ckpt["hyper_parameters"]["lr_schedule"] == "cosine"
    predict.main([out["checkpoint"], "--data_root", tree, "--batch_size", "4"])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert os.path.exists(os.path.join(res["pred_dir"], "metrics.json"))

    plain = fit.main(_fit_args(tree, str(tmp_path / "plain"), ("--lr_schedule", "cosine")))
    capsys.readouterr()
    assert "weight_decay" not in plain and all("weight_decay" not in h for h in plain["history"])
    last = lambda exp: [os.path.join(exp, "checkpoints", p) for p in os.listdir(os.path.join(exp, "checkpoints"))    # noqa: E731
                        if "epoch=01" in p][0]
    a = torch.load(last(str(tmp_path / "wd")), map_location="cpu", weights_only=False)["state_dict"]
    b = torch.load(last(str(tmp_path / "plain")), map_location="cpu", weights_only=False)["state_dict"]
    key = "model.inc.double_conv.0.weight"
    na, nb = float(a[key].double().norm()), float(b[key].double().norm())
    print(f"|{key}| after 2 epochs: {na:.6f} with --weight_decay 0.01, {nb:.6f} without")
    assert na < nb
