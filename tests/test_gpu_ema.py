"""GPU: the weight EMA fused into the Adam step -- fu_adam_ema_step against fu_adam_step and torch's CPU lerp_, the swap
to the averaged weights for evaluation, the captured-graph form, the fp16 guard, and fit / predict / infer end to end.
Every comparison is of bits unless it says otherwise."""
import json
import os

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd.ema import ema_weight
from floodplanet_code_amd.latefusion import HipLateFusion
from floodplanet_code_amd.unet import HipAdam, HipUNet
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADAM = (1e-3, 0.9, 0.999, 1e-8)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _ulps(a, b):
    """Distance in units of the last place between two fp32 tensors (monotone integer image of the floats)."""
    def key(t):
        i = _bits(t).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()


def _small(prec="fp32", seed=1, cin=4):
    net = HipUNet(cin, 3, base_channels=8, precision=prec)
    net.load_state_dict(O.make_state(cin, 3, 8, True, seed=seed))
    return net.to(DEV).train()


def _batch(seed, cin=4, B=2):
    b = O.make_batch(B, cin, 64, 64, seed=seed)
    return b["image"].to(DEV), b["target"].to(DEV)


# ------------------------------------------------------------------------------------------------------------ 1. update parity
def _cpu_lerp(self_t, end, w):
    """torch's CPU self_t.lerp(end, w) on one thread -> (result, mask).  On one thread ATen's vector loop covers all but the
    last n % 32 elements (two AVX-512 vectors per iteration) and a scalar loop the rest.  mask marks the elements on which
    the two loops disagree on this host: the same data padded to a multiple of 32 sends every element through the vector
    loop, and the bits are compared.  Where both loops are one fma the mask is empty."""
    n = self_t.numel()
    out = self_t.clone().lerp_(end, w)
    pad = -n % 32
    if pad == 0:
        return out, torch.zeros(n, dtype=torch.bool)
    vec = torch.cat([self_t, self_t.new_zeros(pad)]).lerp_(torch.cat([end, end.new_zeros(pad)]), w)[:n]
    return out, _bits(out) != _bits(vec)


@pytest.mark.parametrize("cin,base,shift,skew,steps", [(4, 8, 0, 0, 14), (3, 8, 0, 0, 14), (4, 8, 1, 0, 14), (4, 8, 3, 0, 12),
                                                       (3, 8, 1, 2, 12), (8, 64, 0, 0, 12), (8, 64, 2, 0, 10)])
def test_update_equals_adam_step_and_torch_lerp(cin, base, shift, skew, steps):
    """fu_adam_ema_step on one set of flat buffers, fu_adam_step on copies of the same inputs, `steps` updates with the
    warm-up on (w = 9/11 ... crosses 0.5 at update 9, so both lerp branches run).  Parameters and both moments: bit-identical
    to fu_adam_step's.  EMA of the parameters and of the running statistics: torch's CPU Tensor.lerp_(end, w) applied step by
    step to those parameters, bit for bit, on every element -- the kernel's scalar head and tail included.  Only where this
    host's ATen is seen to disagree with itself (_cpu_lerp: its vector loop against its scalar tail, on the same data) are
    those elements held to 1 ulp, the most a single fused multiply-add can differ from its two-rounding form; the count of
    such elements is printed (0 where both loops are one fma).
    shift != 0 puts every buffer `shift` floats past a 16-byte boundary (the kernel's scalar head); skew != 0 moves the EMA
    buffer alone `skew` floats further, so the buffers are not aligned alike and every element takes the scalar path; the
    parameter counts include ones that are no multiple of 4 (its scalar tail).  base 64: the full-width net, 17.27 M
    parameters."""
    lib = _lib.load()
    net = HipUNet(cin, 3, base_channels=base).to(DEV).train()
    ctx = net._get_ctx(torch.device(DEV), 1, 64, 64)
    n, nb = net._total, net._total_bn
    if (cin, base) == (3, 8):
        assert n % 4 != 0                                               # a scalar tail
    g = torch.Generator(device=DEV).manual_seed(100 + cin + shift)

    def buf(count, init=None, off=shift):
        t = torch.zeros(count + 8 + off, dtype=torch.float32, device=DEV)[off:off + count]
        assert t.data_ptr() % 16 == (4 * off) % 16
        if init is not None:
            t.copy_(init)
        return t

    p0 = torch.randn(n, device=DEV, generator=g) * 0.1
    sets = []
    for _ in range(2):                                                  # [0]: fu_adam_step, [1]: fu_adam_ema_step
        sets.append(dict(p=buf(n, p0), g=buf(n), m=buf(n), v=buf(n), rm=buf(nb), rv=buf(nb)))
    ema_p, ema_rm, ema_rv = buf(n, p0, shift + skew), buf(nb), buf(nb)
    assert (ema_p.data_ptr() % 16 != sets[1]["p"].data_ptr() % 16) == (skew != 0)
    ema_rv.fill_(1.0)
    nbt = torch.zeros(len(net._bn), dtype=torch.int64, device=DEV)
    ref_p, ref_rm, ref_rv = ema_p.cpu(), ema_rm.cpu(), ema_rv.cpu()
    stream = net._stream(torch.device(DEV))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        branches = set()
        for step in range(1, steps + 1):
            grad = torch.randn(n, device=DEV, generator=g) * (10.0 ** float(step % 5 - 3))
            rm = torch.randn(nb, device=DEV, generator=g)
            rv = torch.rand(nb, device=DEV, generator=g) + 0.5
            w = ema_weight(0.999, step)
            branches.add(bool(np.float32(w) < 0.5))
            for k, s in enumerate(sets):
                s["g"].copy_(grad), s["rm"].copy_(rm), s["rv"].copy_(rv)
                _lib.check(lib.fu_bind_buffers(ctx, s["p"].data_ptr(), s["g"].data_ptr(), s["rm"].data_ptr(),
                                               s["rv"].data_ptr(), nbt.data_ptr()))
                _lib.check(lib.fu_bind_adam_state(ctx, s["m"].data_ptr(), s["v"].data_ptr()))
                if k == 0:
                    _lib.check(lib.fu_adam_step(ctx, *ADAM, step, 0.5, stream))
                else:
                    _lib.check(lib.fu_bind_ema_state(ctx, ema_p.data_ptr(), ema_rm.data_ptr(), ema_rv.data_ptr()))
                    _lib.check(lib.fu_adam_ema_step(ctx, *ADAM, step, 0.5, w, stream))
            torch.cuda.synchronize()
            a, b = sets
            assert torch.equal(_bits(a["p"]), _bits(b["p"])), step
            assert torch.equal(_bits(a["m"]), _bits(b["m"])) and torch.equal(_bits(a["v"]), _bits(b["v"])), step
            assert torch.equal(b["g"], grad) and torch.equal(b["rm"], rm) and torch.equal(b["rv"], rv)      # inputs only read
            for name, got, ref, end in (("params", ema_p, ref_p, b["p"]), ("running_mean", ema_rm, ref_rm, rm),
                                        ("running_var", ema_rv, ref_rv, rv)):
                want, split = _cpu_lerp(ref, end.cpu(), w)
                d = _ulps(got.cpu(), want)
                agreed = int(d[~split].max()) if (~split).any() else 0
                where_split = int(d[split].max()) if split.any() else 0
                print(f"step {step} w {w:.6f} {name}: max {agreed} ulp; {int(split.sum())} elements where ATen's own loops "
                      f"differ, max {where_split} ulp there")
                assert agreed == 0, (step, name)
                assert where_split <= 1, (step, name)
                ref.copy_(got.cpu())                                    # the next step starts from the kernel's value
        assert branches == {True, False}
        assert a["p"].ne(p0).any() and torch.isfinite(ema_p).all()
    finally:
        torch.set_num_threads(threads)
        _lib.check(lib.fu_bind_ema_state(ctx, None, None, None))
        net._bind(ctx)


def test_step_without_bound_buffers_is_a_state_error():
    lib = _lib.load()
    net = _small()
    x, t = _batch(3)
    net.train_step(x, t, 0)
    stream = net._stream(torch.device(DEV))
    p0 = net.flat_parameters().clone()
    assert lib.fu_adam_ema_step(net._ctx, *ADAM, 1, 1.0, 0.5, stream) == _lib.FU_ERR_STATE        # no EMA buffers bound
    assert b"fu_bind_ema_state" in lib.fu_last_error()
    scal = torch.zeros(8, device=DEV)
    assert lib.fu_adam_ema_step_dev(net._ctx, scal.data_ptr(), stream) == _lib.FU_ERR_STATE
    one = torch.zeros(4, device=DEV)
    assert lib.fu_bind_ema_state(net._ctx, one.data_ptr(), None, None) == _lib.FU_ERR_INVALID     # all three, or none
    torch.cuda.synchronize()
    assert torch.equal(net.flat_parameters(), p0)                       # nothing was launched
    net.enable_ema(0.9)
    net.adam_step(1e-3, 1)
    net.disable_ema()
    assert lib.fu_adam_ema_step(net._ctx, *ADAM, 2, 1.0, 0.5, stream) == _lib.FU_ERR_STATE        # unbound again
    net.adam_step(1e-3, 2)                                              # the plain kernel still runs
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ 2. no perturbation
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_training_is_not_perturbed(prec):
    """K training steps with the EMA on leave parameters, moments and running buffers bit-identical to K steps without."""
    outs = []
    for ema in (False, True):
        net = _small(prec, seed=2)
        if ema:
            net.enable_ema(0.99)
        for step in range(1, 7):
            x, t = _batch(10 + step)
            net.train_step(x, t, 0)
            net.adam_step(1e-3, step)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (net.flat_parameters(), *net.adam_state(), net._flat_rm, net._flat_rv, net._flat_nbt)])
        if ema:
            assert not torch.equal(net.ema_buffers()[0], net.flat_parameters())
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 3. decay 0
def test_decay_zero_tracks_the_live_weights_exactly():
    net = _small(seed=3).train()
    net.enable_ema(0.0, warmup=False)
    opt = HipAdam(net, lr=1e-3)
    for step in range(1, 5):
        x, t = _batch(20 + step)
        opt.zero_grad()
        net.loss(x, t, 0).backward()
        opt.step()
        torch.cuda.synchronize()
        live, ema = net.state_dict(), net.ema_state_dict()
        assert list(live.keys()) == list(ema.keys())
        for k in live:
            assert live[k].shape == ema[k].shape and live[k].dtype == ema[k].dtype, k
            assert torch.equal(live[k], ema[k]), (step, k)
    assert int(live["inc.double_conv.1.num_batches_tracked"]) == 4


def test_optimizer_state_dict_round_trips_the_average():
    """A reloaded HipAdam continues the same average: train 3 + 3 steps in one go, and 3, save, reload into a fresh module
    and optimiser, 3 more."""
    def steps(net, opt, rng):
        for i in rng:
            x, t = _batch(30 + i)
            opt.zero_grad()
            net.loss(x, t, 0).backward()
            opt.step()

    a = _small(seed=4)
    a.enable_ema(0.9)
    oa = HipAdam(a, lr=1e-3)
    steps(a, oa, range(6))
    b = _small(seed=4)
    b.enable_ema(0.9)
    ob = HipAdam(b, lr=1e-3)
    steps(b, ob, range(3))
    saved_model, saved_opt = {k: v.clone() for k, v in b.state_dict().items()}, ob.state_dict()
    assert set(saved_opt["ema"]) == {"decay", "warmup", "params", "running_mean", "running_var"}
    c = HipUNet(4, 3, base_channels=8)
    c.load_state_dict(saved_model)
    c.to(DEV).train()
    c._get_ctx(torch.device(DEV), 2, 64, 64)
    oc = HipAdam(c, lr=1e-3)
    oc.load_state_dict(saved_opt)
    assert c.ema_enabled
    steps(c, oc, range(3, 6))
    torch.cuda.synchronize()
    assert torch.equal(a.flat_parameters(), c.flat_parameters())
    for x, y in zip(a.ema_buffers(), c.ema_buffers()):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------ 4. swap
def _trained_with_ema(make, prec, cin):
    net = make(prec)
    net.enable_ema(0.9)
    for step in range(1, 5):
        x, t = _batch(40 + step, cin)
        net.train_step(x, t, 0)
        net.adam_step(2e-3, step)
    return net


@pytest.mark.parametrize("kind,prec", [("unet", "fp32"), ("unet", "bf16"), ("latefusion", "fp32")])
def test_ema_weights_swaps_and_restores(kind, prec):
    if kind == "unet":
        cin = 4
        make = lambda p: _small(p, seed=5)                                                       # noqa: E731
        fresh = lambda: HipUNet(4, 3, base_channels=8, precision=prec)                           # noqa: E731
    else:
        cin = 3
        make = lambda p: HipLateFusion({"ms_image": 2, "dem": 1}, 3, base_channels=8, precision=p).to(DEV).train()   # noqa: E731
        fresh = lambda: HipLateFusion({"ms_image": 2, "dem": 1}, 3, base_channels=8, precision=prec)                 # noqa: E731
    net = _trained_with_ema(make, prec, cin)
    x, _ = _batch(50, cin)
    net.eval()
    with torch.no_grad():
        before = net(x).clone()
    flat_before = net.flat_parameters().clone()
    rm_before = net._flat_rm.clone()
    ptr_before = net.flat_parameters().data_ptr()
    other = fresh()
    other.load_state_dict(net.ema_state_dict())
    other.to(DEV).eval()
    with torch.no_grad():
        want = other(x).clone()
    with net.ema_weights():
        with torch.no_grad():
            got = net(x).clone()
        net.train()
        with pytest.raises(RuntimeError, match="ema_weights"):
            net._forward_raw(x, True)
        with pytest.raises(RuntimeError, match="ema_weights"):
            net.adam_step(1e-3, 5)
        net.eval()
    with torch.no_grad():
        after = net(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want))
    assert not torch.equal(got, before)                                 # the average really differs from the live weights
    assert torch.equal(_bits(after), _bits(before))
    assert torch.equal(_bits(net.flat_parameters()), _bits(flat_before)) and net.flat_parameters().data_ptr() == ptr_before
    assert torch.equal(net._flat_rm, rm_before)
    # and training goes on from the live weights
    net.train()
    xb, tb = _batch(51, cin)
    net.train_step(xb, tb, 0)
    net.adam_step(2e-3, 5)
    torch.cuda.synchronize()
    assert not torch.equal(net.flat_parameters(), flat_before)


def test_load_ema_state_dict_inside_the_block_is_served():
    """Values loaded into the average while the context reads it reach the next eval forward (the weights are repacked)."""
    net = _trained_with_ema(lambda p: _small(p, seed=6), "fp32", 4)
    x, _ = _batch(52)
    net.eval()
    sd = {k: (v * 0.5 if v.is_floating_point() else v) for k, v in net.ema_state_dict().items()}
    other = HipUNet(4, 3, base_channels=8)
    other.load_state_dict(sd)
    other.to(DEV).eval()
    with torch.no_grad():
        want = other(x).clone()
        with net.ema_weights():
            first = net(x).clone()
            net.load_ema_state_dict(sd)
            got = net(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)) and not torch.equal(got, first)


def test_ema_weights_needs_enable_ema():
    net = _small()
    with pytest.raises(RuntimeError, match="enable_ema"):
        with net.ema_weights():
            pass
    with pytest.raises(RuntimeError):
        net.ema_state_dict()


# ------------------------------------------------------------------------------------------------------------ 5. graph path
def _kernel_nodes(path):
    lines = [l for l in open(path).read().splitlines() if "_ZN2fu" in l]
    return lines, [l for l in lines if "k_adam" in l]


def test_graph_trainer_equals_eager_with_one_optimiser_launch(tmp_path, monkeypatch):
    """DataParallelTrainer(graph=True, ema_decay=...): 13 steps (the weight crosses 0.5 at the 9th, and the 8-slot scalar
    ring wraps) give loss, parameters, moments and EMA buffers bit-identical to the eager trainer.  The captured graph,
    dumped as the trainer's own diagnostics dump it, holds exactly one optimiser kernel node -- k_adam_ema_dev -- and as
    many kernel nodes as the graph captured without an EMA (whose one optimiser node is k_adam_dev)."""
    from floodplanet_code_amd.distributed import DataParallelTrainer
    st = O.make_state(8, 3, 16, True, seed=7)
    host = [O.make_batch(2, 8, 64, 64, seed=70 + i) for i in range(3)]
    outs, dots = [], {}
    for graph, decay in ((False, 0.999), (True, 0.999), (True, None)):
        net = HipUNet(8, 3, base_channels=16, precision="bf16")
        net.load_state_dict(st)
        net.to(DEV).train()
        if graph:
            dots[decay] = str(tmp_path / f"step_{decay}.dot")
            monkeypatch.setenv("FU_GRAPH_DOT", dots[decay])
        else:
            monkeypatch.delenv("FU_GRAPH_DOT", raising=False)
        tr = DataParallelTrainer(net, lr=1e-2, graph=graph, ema_decay=decay)
        losses = []
        for it in range(13):
            b = host[it % 3]
            losses.append(tr.step(b["image"].to(DEV), b["target"].to(DEV), 0))
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph
        if decay is not None:
            outs.append(([l.item() for l in losses], net.flat_parameters().clone(), net.adam_state()[0].clone(),
                         net.adam_state()[1].clone(), [t.clone() for t in net.ema_buffers()]))
    (la, pa, ma, va, ea), (lb, pb, mb, vb, eb) = outs
    assert la == lb and len(set(lb)) > 1
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    for x, y in zip(ea, eb):
        assert torch.equal(x, y)
    assert not torch.equal(ea[0], pa)
    with_ema, adam_with = _kernel_nodes(dots[0.999])
    without, adam_without = _kernel_nodes(dots[None])
    assert len(adam_with) == 1 and "k_adam_ema_dev" in adam_with[0]
    assert len(adam_without) == 1 and "k_adam_dev" in adam_without[0]
    assert len(with_ema) == len(without) > 10


# ------------------------------------------------------------------------------------------------------------ 6. fp16 skip
def test_fp16_skipped_step_leaves_the_average_untouched():
    """The overflowing scenario of the fp16 guard test (OutConv weights of 3e3: the first fp16 gradient map overflows, the
    gradient buffer holds inf / NaN, the device flag skips the update): the EMA buffers stay untouched by that step, and move
    with the first step that is applied."""
    st = O.make_state(8, 3, 16, True, seed=1)
    st["outc.conv.weight"][:] = st["outc.conv.weight"].sign() * 3.0e3
    batch = O.make_batch(2, 8, 64, 64, seed=2)
    x, t = batch["image"].to(DEV), batch["target"].to(DEV)
    net = HipUNet(8, 3, base_channels=16, precision="fp16")
    net.load_state_dict(st)
    net.to(DEV).train()
    net.enable_ema(0.9, warmup=False)
    net.train_step(x, t, 0)
    torch.cuda.synchronize()
    assert not torch.isfinite(net.flat_grads()).all()                   # the scenario really overflows
    # make the averages differ from the live values, so that an update that ran would show
    for e in net.ema_buffers():
        e.mul_(0.5).add_(0.25)
    p0 = net.flat_parameters().clone()
    e0 = [e.clone() for e in net.ema_buffers()]
    net.adam_step(1e-3, 1)
    torch.cuda.synchronize()
    assert torch.equal(net.flat_parameters(), p0)                       # skipped
    assert net.fp16_guard_state() == (1, 1)
    for e, k in zip(net.ema_buffers(), e0):
        assert torch.equal(_bits(e), _bits(k))
    applied = False
    for step in range(2, 14):
        net.train_step(x, t, 0)
        finite = bool(torch.isfinite(net.flat_grads()).all())
        before = [e.clone() for e in net.ema_buffers()]
        net.adam_step(1e-3, step)
        torch.cuda.synchronize()
        moved = [not torch.equal(e, k) for e, k in zip(net.ema_buffers(), before)]
        assert all(m == finite for m in moved), (step, finite, moved)
        applied = applied or finite
    assert applied and all(torch.isfinite(e).all() for e in net.ema_buffers())


# ------------------------------------------------------------------------------------------------------------ 7. end to end
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


def _write_ckpt(src, dst_exp, state_dict, hyper):
    d = os.path.join(dst_exp, "checkpoints")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, os.path.basename(src))
    torch.save({"state_dict": state_dict, "epoch": 1, "hyper_parameters": hyper}, path)
    return path


def test_fit_predict_infer_with_ema(tree, tmp_path, capsys):
    import copy
    from floodplanet_code_amd import fit, infer, predict
    from floodplanet_code_amd.datasets import FloodplanetTiles, SceneTileLoader, generate_image_slice_object
    from floodplanet_code_amd.models import build_model
    exp = str(tmp_path / "exp")
    out = fit.main(_fit_args(tree, exp, ("--ema_decay", "0.9")))
    capsys.readouterr()
    assert len(out["history"]) == 2
    last = [p for p in os.listdir(os.path.join(exp, "checkpoints")) if "epoch=01" in p]
    assert len(last) == 1
    ckpt_path = os.path.join(exp, "checkpoints", last[0])
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=False)
    kw = ckpt["hyper_parameters"]["model"]["model_kwargs"]
    assert kw["ema_decay"] == 0.9 and kw["ema_warmup"] is True
    raw, ema = ckpt["state_dict"], ckpt["ema_state_dict"]
    assert list(raw.keys()) == list(ema.keys())
    assert all(raw[k].shape == ema[k].shape for k in raw)
    assert any(not torch.equal(raw[k], ema[k]) for k in raw if k.endswith("weight"))
    assert all(torch.equal(raw[k], ema[k]) for k in raw if k.endswith("num_batches_tracked"))

    # the monitored metric is the averaged model's: recompute it from ema_state_dict on the same validation loader
    hyper = ckpt["hyper_parameters"]
    plain_kw = {k: v for k, v in kw.items() if k not in ("ema_decay", "ema_warmup")}
    valid_ds = FloodplanetTiles(tree, "valid", generate_image_slice_object(64, 64, 32), eval_region=copy.copy(hyper["eval_region"]),
                                sensor="S1", channels=hyper["dataset"]["channels"], norm_mode=hyper["norm_mode"],
                                ignore_index=hyper["ignore_index"], seed_num=hyper["seed_num"],
                                train_split_pct=hyper["train_split_pct"], norm_params=hyper["norm_params"])

    def val_miou(state_dict):
        m = build_model(hyper["model"]["name"], valid_ds.n_channels, valid_ds.n_classes, hyper["lr"], 200, None,
                        ignore_index=hyper["ignore_index"], **plain_kw)
        m.load_state_dict(state_dict)
        m = m.to(DEV)
        loader = SceneTileLoader(valid_ds, hyper["batch_size"], DEV, net=m.model, seed=hyper["seed_num"],
                                 ignore_index=hyper["ignore_index"], num_workers=0)
        m.valid_metrics.reset()
        outs = [m.validation_step(b, i) for i, b in enumerate(loader)]
        m.validation_epoch_end(outs)
        return float(m.logged["val_MulticlassJaccardIndex"])

    logged = out["history"][-1]["val_MulticlassJaccardIndex"]
    print("history", logged, "ema", val_miou(ema), "raw", val_miou(raw))
    assert val_miou(ema) == logged

    # predict: auto == ema; raw == a plain checkpoint holding the same state_dict
    plain_hyper = copy.deepcopy(hyper)
    plain_hyper["model"]["model_kwargs"] = plain_kw
    plain_raw = _write_ckpt(ckpt_path, str(tmp_path / "exp_raw"), raw, plain_hyper)
    plain_ema = _write_ckpt(ckpt_path, str(tmp_path / "exp_ema"), ema, plain_hyper)

    def run(path, exp_dir, **kwargs):
        cfg = predict.resolve_cfg(exp_dir, path)
        return predict.predict(cfg, exp_dir, path, "floodplanet", predict_images=True, n_workers=0, data_root=tree,
                               batch_size=4, device=DEV, **kwargs)

    def same(a, b, skip=("weights",)):
        assert {k: v for k, v in a["metrics"].items() if k not in skip} == \
            {k: v for k, v in b["metrics"].items() if k not in skip}
        assert a["image_stats_iou"] == b["image_stats_iou"] and set(a["probabilities"]) == set(b["probabilities"])
        for k in a["probabilities"]:
            np.testing.assert_array_equal(a["probabilities"][k], b["probabilities"][k])

    auto = run(ckpt_path, exp, weights="auto")
    assert json.load(open(os.path.join(auto["pred_dir"], "metrics.json")))["weights"] == "ema"
    as_ema = run(ckpt_path, exp, weights="ema")
    same(auto, as_ema, skip=())
    as_raw = run(ckpt_path, exp, weights="raw")
    assert as_raw["metrics"]["weights"] == "raw"
    before = run(plain_raw, str(tmp_path / "exp_raw"))                  # no flag, no EMA entry: the file it always wrote
    assert "weights" not in json.load(open(os.path.join(before["pred_dir"], "metrics.json")))
    same(as_raw, before)
    same(as_ema, run(plain_ema, str(tmp_path / "exp_ema")))
    assert any(not np.array_equal(as_raw["probabilities"][k], as_ema["probabilities"][k]) for k in as_raw["probabilities"])
    with pytest.raises(KeyError, match=os.path.basename(plain_raw)):
        run(plain_raw, str(tmp_path / "exp_raw"), weights="ema")

    # infer --weights ema: the class maps of a model loaded from the EMA dict
    scenes = os.path.join(tree, "CSDAP_complete", "RegB", "S1")
    infer.main([ckpt_path, scenes, "--out_dir", str(tmp_path / "maps_ema"), "--weights", "ema"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["weights"] == "ema"
    ref = infer.infer(plain_ema, [scenes], str(tmp_path / "maps_ref"))
    assert ref["weights"] == "raw" and ref["n_scenes"] == 3
    got = json.load(open(tmp_path / "maps_ema" / "summary.json"))
    for a, b in zip(got["scenes"], ref["scenes"]):
        assert a["class_pixels"] == b["class_pixels"]
        assert open(a["output"], "rb").read() == open(b["output"], "rb").read()


def test_checkpoint_without_the_flag_is_what_it_always_was(tree, tmp_path, capsys):
    from floodplanet_code_amd import fit, predict
    exp = str(tmp_path / "exp")
    out = fit.main(_fit_args(tree, exp))
    capsys.readouterr()
    ckpt = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)
    assert set(ckpt) == {"state_dict", "epoch", "hyper_parameters"}
    assert ckpt["hyper_parameters"]["model"]["model_kwargs"] == dict(optimizer_name="adam", base_channels=8, precision="fp32")
    predict.main([out["checkpoint"], "--data_root", tree, "--batch_size", "4"])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "weights" not in res and os.path.exists(os.path.join(res["pred_dir"], "metrics.json"))
