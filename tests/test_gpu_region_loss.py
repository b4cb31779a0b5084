"""GPU: the soft Dice / Jaccard / Tversky region term of fu_loss_ce_region (k_region_sums, k_region_finalize,
k_region_grad_add of fu_loss.hip), at the op level on operands the test builds, through HipUNet, the trainers and fit.  The
specification is tests/tools/region_ref.py (NumPy fp64; pinned to fp64 autograd in tests/test_region_loss_cpu.py).

Op level, as tests/test_gpu_loss_ops.py (its Driver: fu_test_loss_buffers hands out the resident logits and the stored loss
gradient):
  a. 2 x 37 x 45 constructed inputs, C in {2, 3, 4, 5, 8}, three ignore values, Dice / Jaccard / Tversky (0.3, 0.7) / s = 1e-3,
     over each CE form;
  b. 592 x 592 with 1 and 3 samples: the later trips of k_region_sums (cap: region_ref.region_cap(3) = 455 blocks) and of the gradient
     pass (4096), with every pixel valid and with only the pixels beyond a cap valid;
  c. weight 0 / region == NULL: the bits of fu_loss_ce, fu_loss_ce_weighted, fu_loss_ce_focal; two calls give the same bits; an
     eval forward's call leaves the gradient buffer alone; the all-ignored batch; rejected calls launch nothing.
Bounds (every element): |loss - spec| <= 1e-5 max(1, |spec|); counts exact; D within 1e-5 relative; every gradient element
within region_ref.grad_bound; invalid pixels exactly 0; region_out (R, TI_k) within 1e-5.

Through the net: the loss in fp32 / bf16 / fp16 against the specification at the returned logits (1e-5), parameter gradients
against the specification's logit gradient through the same backward (1e-5 relative L2 per live tensor, the focal suite's
tolerance); the captured trainer; exact data-parallel mode (1e-6 on the loss, 2e-3 relative L2 on the gradient, the focal
exact-mode test's bounds); fit --region_loss end to end."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch

from conftest import is_dead_bias
from floodplanet_code_amd import _lib
from floodplanet_code_amd._lib import check, ptr
from floodplanet_code_amd.unet import HipUNet
from oracle import unet_oracle as O

sys.path.insert(0, os.path.dirname(__file__))
from test_gpu_loss_ops import SENTINEL, driver  # noqa: E402
from tools import loss_ref as L  # noqa: E402
from tools import region_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLASSES = [2, 3, 4, 5, 8]
LAM = 0.7
CE_FORMS = [("ce", {}), ("weighted", {"eps": 0.1}), ("focal", {"gamma": 2.0})]
NAMES = {(0.5, 0.5, 0.5): "dice s=0.5", (1.0, 1.0, 1.0): "jaccard", (0.3, 0.7, 1.0): "tversky .3 .7", (0.5, 0.5, 1e-3): "dice s=1e-3"}


def _region_call(d, t, ii, region, weight=None, eps=0.0, gamma=0.0, want_status=False, loss_init=-7.0):
    """fu_loss_ce_region on a loss_ops Driver -> dict(loss, n_valid, D, confusion, region_out); region: (weight, alpha, beta,
    smooth), a _lib.FuRegionLoss or None (NULL)"""
    lib, ctx, s = _lib.load(), d.net._ctx, d.net._stream(d.dev)
    t_dev = torch.from_numpy(t).to(DEV)
    loss = torch.full((), loss_init, dtype=torch.float32, device=DEV)
    conf = torch.zeros(d.C * d.C, dtype=torch.int64, device=DEV)
    n_valid = torch.full((), -7, dtype=torch.int64, device=DEV)
    wsum = torch.full((), -7.0, dtype=torch.float32, device=DEV)
    rout = torch.full((1 + d.C,), -7.0, dtype=torch.float32, device=DEV)
    w_dev = None if weight is None else torch.tensor(weight, dtype=torch.float32, device=DEV)
    rg = _lib.FuRegionLoss(*region) if isinstance(region, tuple) else region
    status = lib.fu_loss_ce_region(ctx, ptr(t_dev), ii, ptr(w_dev), eps, gamma, rg, ptr(loss), ptr(conf), ptr(n_valid),
                                   ptr(wsum), ptr(rout), s)
    torch.cuda.synchronize()
    out = {"loss": loss.item(), "n_valid": int(n_valid), "D": float(wsum), "region_out": rout.cpu().numpy().astype(np.float64),
           "confusion": conf.cpu().numpy().reshape(d.C, d.C), "status": status}
    if not want_status:
        check(status)
    return out


def _ce_kw(form, kw):
    """(weight, eps, gamma) of one CE form's keyword arguments"""
    return dict(weight=kw.get("weight") if form != "ce" else None, eps=kw.get("eps", 0.0), gamma=kw.get("gamma", 0.0))


def _hold(d, label, form, z, t, ii, params, kw, training=True, lam=LAM):
    """run CE form + region term on (z, t) and hold it to every bound of the module docstring"""
    alpha, beta, s = params
    ref = R.reference(form, z, t, ii, lam, alpha, beta, s, **kw)
    got = _region_call(d, t, ii, (lam, alpha, beta, s), **_ce_kw(form, kw))
    v = L.valid_mask(t, ii, d.C)
    what = (label, form, d.C, ii, t.size, params)
    want_out = np.concatenate([[ref["R"]], ref["TI"]])
    print(f"{label} {form} C={d.C} ii={ii} P={t.size}: loss {got['loss']!r} spec {ref['loss']!r} (CE {ref['ce_loss']!r}) "
          f"|d| {abs(got['loss'] - ref['loss']):.2e} (bound {1e-5 * max(1.0, abs(ref['loss'])):.2e}); n_valid {got['n_valid']}; "
          f"region_out max |d| {np.abs(got['region_out'] - want_out).max():.2e}")
    assert np.isfinite(got["loss"]) and L.loss_ok(got["loss"], ref["loss"]), what + (got["loss"], ref["loss"])
    assert got["n_valid"] == ref["n_valid"] == int(v.sum()), what
    assert np.array_equal(got["confusion"], ref["confusion"]), what
    if form == "ce":
        assert got["D"] == -7.0, what                                       # weight_sum_out: the weighted and focal forms only
    else:
        assert abs(got["D"] - ref["D"]) <= 1e-5 * ref["D"], what + (got["D"], ref["D"])
    assert np.abs(got["region_out"] - want_out).max() <= 1e-5, what + (got["region_out"], want_out)
    assert (got["region_out"][1:][~R.included(d.C, ii)] == 1.0).all(), what
    if not training:
        return got, None
    g = d.grad()
    bound = R.grad_bound(form, z, t, ii, lam, alpha, beta, s, spec=ref["grad"], **kw)
    ratio = L.worst_ratio(g, ref["grad"], bound)
    err = np.abs(g.astype(np.float64) - ref["grad"])
    at = np.unravel_index(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)), err.shape)
    print(f"    gradient: worst err / bound {ratio:.3f} at pixel {at[0]} class {at[1]} (z {z[at[0]]}, t {t[at[0]]}), "
          f"max |g| {np.abs(ref['grad']).max():.3e}, max |region g| {np.abs(ref['region_grad']).max():.3e}")
    assert np.isfinite(g).all(), what
    assert not g[~v].any(), what                                            # invalid pixels: exactly 0
    assert ratio <= 1.0, what + (ratio,)
    return got, g


# ------------------------------------------------------------------------------------------------ a. constructed inputs
@pytest.mark.parametrize("n_classes,ii", [(c, ii) for c in CLASSES for ii in (0, c - 1, -100)])
def test_constructed_inputs_every_form_and_parameter_set(n_classes, ii):
    B, H, W = L.SHAPE_A
    d = driver(n_classes, B, H, W).forward(B)
    z, t = L.constructed_inputs(n_classes, ii)
    d.set_logits(z)
    for params in R.PARAM_SETS:
        for form, kw in CE_FORMS:
            d.fill_grad(SENTINEL)                                           # every element must be written by the call
            _, g = _hold(d, NAMES[params], form, z, t, ii, params, L.form_kwargs(form, kw, n_classes, ii))
            assert np.abs(g).max() > 0


def test_zero_weight_classes_keep_the_region_term_alive():
    """valid pixels whose classes all carry weight 0: the CE is 0 (D == 0) with a zero gradient, the region term is not"""
    B, H, W = L.SHAPE_A
    d = driver(3, B, H, W).forward(B)
    z, t = L.constructed_inputs(3, -100)
    t = np.where(L.valid_mask(t, -100, 3), t % 2 + 1, t)
    d.set_logits(z)
    d.fill_grad(SENTINEL)
    kw = {"eps": 0.0, "weight": [3.0, 0.0, 0.0]}
    got, g = _hold(d, "zero weights", "weighted", z, t, -100, (0.5, 0.5, 1.0), kw)
    ref = R.reference("weighted", z, t, -100, LAM, 0.5, 0.5, 1.0, **kw)
    assert got["D"] == 0.0 and ref["ce_loss"] == 0.0 and got["loss"] > 0.0 and g.any()


# ------------------------------------------------------------------------------------------------ b. later trips
@pytest.mark.parametrize("form,kw", [("ce", {}), ("weighted", {"eps": 0.1, "weight": [0.0, 0.7, 1.3]})], ids=["ce", "weighted"])
def test_later_trips_of_the_region_passes(form, kw):
    H, W = L.SHAPE_B
    d = driver(3, 3, H, W)
    cap = R.region_cap(3)
    assert cap == 455 and H * W > 3 * 256 * cap and 3 * H * W > 256 * L.GRAD_CAP            # the caps are crossed
    assert (H * W) % (256 * cap) != 0 and (3 * H * W) % (256 * L.GRAD_CAP) != 0             # ragged final trips
    for batch in (1, 3):
        d.forward(batch)
        d.set_logits(L.big_case(batch, 0)[0])
        for b, valid_from in R.big_layouts():
            if b != batch:
                continue
            z, t = L.big_case(batch, valid_from)
            d.fill_grad(SENTINEL)
            params = R.PARAM_SETS[2] if valid_from else R.PARAM_SETS[0]
            got, g = _hold(d, f"valid from {valid_from}", form, z, t, -100, params, kw)
            assert got["loss"] > 0.0 and g[valid_from:].any() and not g[:valid_from].any()


# ------------------------------------------------------------------------------------------------ c. bit identity
def _bits(d, got):
    return (np.float32(got["loss"]).tobytes(), got["n_valid"], got["D"], got["confusion"].tobytes(), d.grad().tobytes())


@pytest.mark.parametrize("form,kw", CE_FORMS, ids=[f[0] for f in CE_FORMS])
def test_weight_zero_and_null_region_give_the_existing_entry_points_bits(form, kw):
    B, H, W = L.SHAPE_A
    for ii in (0, -100):
        d = driver(3, B, H, W).forward(B)
        z, t = L.constructed_inputs(3, ii)
        d.set_logits(z)
        kw_full = L.form_kwargs(form, kw, 3, ii)
        d.fill_grad(SENTINEL)
        want = d.loss(form, t, ii, **kw_full)
        if form == "ce":
            want["D"] = -7.0                                                # fu_loss_ce writes no D; nor does the plain form here
        want = _bits(d, want)
        for region in (None, (0.0, 0.5, 0.5, 1.0), (0.0, 0.3, 0.7, 1e-3)):
            d.fill_grad(SENTINEL)
            got = _region_call(d, t, ii, region, **_ce_kw(form, kw_full))
            assert (got["region_out"] == -7.0).all()                        # nothing new was launched
            assert _bits(d, got) == want, (form, ii, region)
    if form == "weighted":                                                  # weights without smoothing: the weighted kernels too
        d.fill_grad(SENTINEL)
        want = _bits(d, d.loss("weighted", t, ii, weight=kw_full["weight"], eps=0.0))
        d.fill_grad(SENTINEL)
        assert _bits(d, _region_call(d, t, ii, None, weight=kw_full["weight"])) == want


def test_two_calls_give_the_same_bits():
    B, H, W = L.SHAPE_A
    for shape, batch, (z, t), ii in (((3, B, H, W), B, L.constructed_inputs(3, 0), 0),
                                     ((3, 3) + L.SHAPE_B, 3, L.big_case(3, 0), -100)):
        d = driver(*shape).forward(batch)
        d.set_logits(z)
        for form, kw in CE_FORMS[:2] if batch == 3 else CE_FORMS:
            kw = L.form_kwargs(form, kw, 3, ii)
            runs = []
            for _ in range(2):
                d.fill_grad(SENTINEL)
                got = _region_call(d, t, ii, (LAM, 0.3, 0.7, 1.0), **_ce_kw(form, kw))
                runs.append(_bits(d, got) + (got["region_out"].tobytes(),))
            assert runs[0] == runs[1], (form, batch)


def test_eval_forward_loss_is_right_and_leaves_the_gradient_buffer_alone():
    B, H, W = L.SHAPE_A
    d = driver(3, B, H, W).forward(B, training=False)
    z, t = L.constructed_inputs(3, 0)
    d.set_logits(z)
    d.fill_grad(SENTINEL)
    for form, kw in CE_FORMS:
        _hold(d, "eval", form, z, t, 0, (0.5, 0.5, 1.0), L.form_kwargs(form, kw, 3, 0), training=False)
        assert (d.grad() == np.float32(SENTINEL)).all(), form
    d.forward(B, training=True)                                             # the same context trains again afterwards
    d.set_logits(z)
    _hold(d, "after eval", "ce", z, t, 0, (0.5, 0.5, 1.0), {})


def test_all_ignored_batch_gives_zero_loss_and_exactly_zero_gradients():
    B, H, W = L.SHAPE_A
    d = driver(3, B, H, W).forward(B)
    z, t = L.constructed_inputs(3, -100)
    d.set_logits(z)
    for form, kw in CE_FORMS:
        for params in R.PARAM_SETS:
            d.fill_grad(SENTINEL)
            got, g = _hold(d, "all ignored", form, z, np.full_like(t, 2), 2, params, L.form_kwargs(form, kw, 3, 2))
            assert got["loss"] == 0.0 and not g.any() and got["region_out"][0] == 0.0
            assert (got["region_out"][1:] == 1.0).all()                     # TI_k = s / s


def test_rejected_calls_launch_nothing():
    B, H, W = L.SHAPE_A
    d = driver(3, B, H, W).forward(B)
    z, t = L.constructed_inputs(3, 0)
    d.set_logits(z)
    nan, inf = float("nan"), float("inf")
    bad = {"weight -1": dict(region=(-1.0, 0.5, 0.5, 1.0)), "weight NaN": dict(region=(nan, 0.5, 0.5, 1.0)),
           "weight inf": dict(region=(inf, 0.5, 0.5, 1.0)), "alpha -1": dict(region=(1.0, -1.0, 0.5, 1.0)),
           "beta NaN": dict(region=(1.0, 0.5, nan, 1.0)), "alpha inf": dict(region=(1.0, inf, 0.5, 1.0)),
           "alpha + beta 0": dict(region=(1.0, 0.0, 0.0, 1.0)), "smooth 0": dict(region=(1.0, 0.5, 0.5, 0.0)),
           "smooth NaN": dict(region=(1.0, 0.5, 0.5, nan)), "smooth inf": dict(region=(1.0, 0.5, 0.5, inf)),
           "bad options at weight 0": dict(region=(0.0, 0.0, 0.0, 1.0)),
           "eps 1": dict(region=(1.0, 0.5, 0.5, 1.0), eps=1.0), "gamma -1": dict(region=(1.0, 0.5, 0.5, 1.0), gamma=-1.0),
           "gamma with eps": dict(region=(1.0, 0.5, 0.5, 1.0), gamma=2.0, eps=0.1)}
    for what, kw in bad.items():
        d.fill_grad(SENTINEL)
        got = _region_call(d, t, 0, want_status=True, **kw)
        assert got["status"] == _lib.FU_ERR_INVALID and _lib.load().fu_last_error(), what
        assert got["loss"] == -7.0 and got["n_valid"] == -7 and got["D"] == -7.0 and not got["confusion"].any(), what
        assert (got["region_out"] == -7.0).all() and (d.grad() == np.float32(SENTINEL)).all(), what
    d1 = driver(1, B, H, W).forward(B)                                      # one class: no region term, whatever the options
    t1 = np.zeros(B * H * W, np.int64)
    d1.fill_grad(SENTINEL)
    got = _region_call(d1, t1, -100, (1.0, 0.5, 0.5, 1.0), want_status=True)
    assert got["status"] == _lib.FU_ERR_INVALID and got["loss"] == -7.0 and (d1.grad() == np.float32(SENTINEL)).all()
    assert _region_call(d1, t1, -100, (0.0, 0.5, 0.5, 1.0))["loss"] == 0.0  # weight 0 is fu_loss_ce, which takes one class
    d.fill_grad(SENTINEL)
    assert _region_call(d, t, 0, (1.0, 0.5, 0.5, 1.0))["loss"] > 0.0        # the same call, valid, does run


# ------------------------------------------------------------------------------------------------ through the net
def _net(n_in, n_classes, base=16, precision="fp32", seed=0):
    net = HipUNet(n_in, n_classes, base_channels=base, precision=precision)
    net.load_state_dict(O.make_state(n_in, n_classes, base, True, seed=seed))
    return net.to(DEV).train()


def _pixels(logits):
    return logits.detach().cpu().permute(0, 2, 3, 1).reshape(-1, logits.shape[1]).numpy()


REGION = dict(region_weight=LAM, region_alpha=0.3, region_beta=0.7, region_smooth=1.0)


@pytest.mark.parametrize("n_classes", [2, 3])
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_loss_through_the_net_matches_the_specification_at_the_returned_logits(precision, n_classes):
    ii = -100 if n_classes == 2 else 0
    b = O.make_batch(2, 4, 37, 45, seed=60 + n_classes, n_label_values=n_classes)
    x, t_dev, t = b["image"].to(DEV), b["target"].to(DEV), b["target"].reshape(-1).numpy()
    net = _net(4, n_classes, precision=precision, seed=40 + n_classes)
    w = L.class_weights(n_classes, ii)
    for form, ce, kw in (("ce", {}, {}),
                         ("weighted", dict(class_weight=w, label_smoothing=0.1), dict(weight=w, eps=0.1)),
                         ("focal", dict(class_weight=w, focal_gamma=2.0), dict(weight=w, gamma=2.0))):
        loss, logits = net.loss(x, t_dev, ii, return_logits=True, **ce, **REGION)
        loss.backward()
        torch.cuda.synchronize()
        ref = R.reference(form, _pixels(logits), t, ii, LAM, 0.3, 0.7, 1.0, **kw)
        terms = net.last_region_terms().cpu().numpy().astype(np.float64)
        print(f"{precision} C={n_classes} {form}: gpu {loss.item()!r} spec {ref['loss']!r} |d| {abs(loss.item() - ref['loss']):.2e}; "
              f"R {terms[0]!r} spec {ref['R']!r}")
        assert ref["R"] > 0 and L.loss_ok(loss.item(), ref["loss"]), (loss.item(), ref["loss"])
        assert np.abs(terms - np.concatenate([[ref["R"]], ref["TI"]])).max() <= 1e-5
        g = net.flat_grads()
        assert bool(torch.isfinite(g).all()) and bool(g.any())
    if precision == "fp16":
        net.adam_step(1e-3, 1)
        torch.cuda.synchronize()
        assert net.fp16_guard_state() == (0, 0)


def _compare_live_tensors(net, grads_a, grads_b, bound=1e-5):
    live, worst, over = 0, 0.0, []
    for (name, _, off, n) in net._table:
        if is_dead_bias(name):
            continue
        a, g = grads_a[off:off + n].double(), grads_b[off:off + n].double()
        if a.norm().item() == 0.0:
            assert g.norm().item() == 0.0, name
            continue
        rel = ((a - g).norm() / a.norm()).item()
        worst, live = max(worst, rel), live + 1
        if not rel <= bound:
            over.append((name, rel))
    return live, worst, over


@pytest.mark.parametrize("C,ii,params", [(3, 0, (0.5, 0.5, 1.0)), (2, -100, (1.0, 1.0, 1.0)), (4, 3, (0.3, 0.7, 1.0))])
def test_gradients_match_the_specifications_logit_gradient_through_the_same_backward(C, ii, params):
    """Route A: the specification's dL/dlogits at the GPU's logits through fu_backward; route B: the fused loss's own
    backward; control: the specification with alpha and beta swapped (Jaccard: another smoothing) is another loss."""
    dev = torch.device(DEV)
    net = _net(4, C, seed=20 + C)
    b = O.make_batch(2, 4, 37, 45, seed=31 + C, n_label_values=C)
    x, t = b["image"].to(DEV), b["target"].reshape(-1).numpy()
    alpha, beta, s = params

    def route_a(al, be, sm):
        logits = net._forward_raw(x, True)
        g = R.reference("ce", _pixels(logits), t, ii, LAM, al, be, sm)["grad"]
        dl = torch.from_numpy(g.astype(np.float32)).reshape(2, 37, 45, C).permute(0, 3, 1, 2).contiguous().to(DEV)
        net._backward_raw(dl, dev)
        return net.flat_grads().clone()

    grads_a = route_a(alpha, beta, s)
    net.train_step(x, b["target"].to(DEV), ii, region_weight=LAM, region_alpha=alpha, region_beta=beta, region_smooth=s)
    grads_b = net.flat_grads().clone()
    grads_c = route_a(beta, alpha, s) if alpha != beta else route_a(alpha, beta, 4.0 * s)
    torch.cuda.synchronize()
    live, worst, over = _compare_live_tensors(net, grads_a, grads_b)
    print(f"C={C} ii={ii} {params}: {live} live tensors, worst relative L2 {worst:.2e}")
    assert not over, over
    assert live >= 40
    _, worst_c, over_c = _compare_live_tensors(net, grads_c, grads_b)
    print(f"  control: worst relative L2 {worst_c:.2e}, {len(over_c)} tensors over the bound")
    assert len(over_c) >= 1


# ------------------------------------------------------------------------------------------------ captured step
def test_graph_trainer_replays_the_region_loss():
    from floodplanet_code_amd.distributed import DataParallelTrainer
    b = O.make_batch(2, 4, 32, 32, seed=9, n_label_values=3)
    x, t = b["image"].to(DEV), b["target"].to(DEV)
    losses = {}
    for graph in (False, True):
        net = _net(4, 3)
        tr = DataParallelTrainer(net, lr=1e-3, graph=graph, class_weight=(0.0, 0.6, 2.4), **REGION)
        losses[graph] = [tr.step(x, t, 0).item() for _ in range(4)]
        assert (tr._graph is not None) == graph
    torch.cuda.synchronize()
    print("eager", losses[False], "graph", losses[True])
    assert losses[True] == losses[False] and all(np.isfinite(v) for v in losses[True])
    net = _net(4, 3)                                                        # the first step's loss is the specification's
    z = _pixels(net._forward_raw(x, True))
    want = R.reference("weighted", z, b["target"].reshape(-1).numpy(), 0, LAM, 0.3, 0.7, 1.0, weight=[0.0, 0.6, 2.4])
    assert want["R"] > 0 and abs(losses[True][0] - want["loss"]) <= 1e-5


# ------------------------------------------------------------------------------------------------ exact data parallel
def _dp_batch(rank_seed):
    return O.make_batch(2, 8, 64, 64, seed=20 + rank_seed, n_label_values=3)


def _worker_exact(rank, world, port, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    dev = torch.device("cuda", 0)                                           # both ranks share the one GPU (gloo)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from floodplanet_code_amd.distributed import DataParallelTrainer
    net = HipUNet(8, 3, base_channels=16)
    net.load_state_dict(O.make_state(8, 3, 16, True, seed=0))
    net.to(dev).train()
    tr = DataParallelTrainer(net, lr=1e-3, world_size=world, rank=rank, cap_bytes=256 << 10, exact=True, **REGION)
    b = _dp_batch(rank)
    loss = tr.step(b["image"].to(dev), b["target"].to(dev), 0)
    torch.cuda.synchronize()
    torch.save({"loss": loss.cpu(), "terms": net.last_region_terms().cpu(), "grads": net.flat_grads().cpu()},
               f"{out_path}.{rank}")
    dist.destroy_process_group()


def test_exact_mode_two_half_batches_give_the_region_loss_of_the_whole_batch(tmp_path):
    """I, P and T pass through the rank sum: both ranks form the whole batch's R and coefficients"""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "exact.pt")
    mp.spawn(_worker_exact, args=(2, port, out), nprocs=2, join=True)
    res = [torch.load(f"{out}.{r}") for r in range(2)]
    net = HipUNet(8, 3, base_channels=16)
    net.load_state_dict(O.make_state(8, 3, 16, True, seed=0))
    net.to(DEV).train()
    b0, b1 = _dp_batch(0), _dp_batch(1)
    x, t = torch.cat([b0["image"], b1["image"]]).to(DEV), torch.cat([b0["target"], b1["target"]]).to(DEV)
    loss = net.train_step(x, t, 0, **REGION)
    terms = net.last_region_terms().clone().cpu()
    grads = net.flat_grads().clone().cpu()
    torch.cuda.synchronize()
    for r in res:
        print("rank loss", repr(r["loss"].item()), "joint", repr(loss.item()), "R", float(r["terms"][0]), float(terms[0]))
        assert abs(r["loss"].item() - loss.item()) <= 1e-6
        assert float((r["terms"] - terms).abs().max()) <= 1e-6 and float(terms[0]) > 0
    assert res[0]["loss"].item() == res[1]["loss"].item() and torch.equal(res[0]["terms"], res[1]["terms"])
    rel = ((res[0]["grads"] - grads).norm() / grads.norm()).item()
    print("gradient relative L2", rel)
    assert rel <= 2e-3, rel


# ------------------------------------------------------------------------------------------------ fit, end to end
def _fit_args(root, exp, extra=()):
    return [root, "--exp_dir", exp, "--sensor", "S1", "--eval_region", "RegB", "--crop", "64", "64", "--stride", "32",
            "--batch_size", "4", "--n_epochs", "2", "--lr", "2e-3", "--base_channels", "8", "--loader", "scene",
            "--n_workers", "0", "--seed", "0", "--save_topk_models", "1", "--device", DEV, "--no_transforms", "--no_shuffle",
            *extra]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from floodplanet_code_amd.datasets.synthetic import make_s1_tree
    root = str(tmp_path_factory.mktemp("tree"))
    make_s1_tree(root, regions=("RegA", "RegB"), images_per_region=2, label_size=100, s1_size=40)
    return root


def _spy(monkeypatch):
    lib = _lib.load()
    calls = {"fu_loss_ce": 0, "fu_loss_ce_weighted": 0, "fu_loss_ce_focal": 0, "fu_loss_ce_region": 0}

    def wrap(name):
        real = getattr(lib, name)

        def spy(*a):
            calls[name] += 1
            return real(*a)
        monkeypatch.setattr(lib, name, spy)

    for name in calls:
        wrap(name)
    return calls


def test_fit_with_region_loss_and_the_checkpoint_serves_predict_and_infer(tree, tmp_path, capsys, monkeypatch):
    from floodplanet_code_amd import fit, infer, predict
    calls = _spy(monkeypatch)
    out = fit.main(_fit_args(tree, str(tmp_path / "dice"), ("--region_loss", "dice")))
    capsys.readouterr()
    assert calls["fu_loss_ce_region"] > 0
    assert calls["fu_loss_ce"] == 0 and calls["fu_loss_ce_weighted"] == 0 and calls["fu_loss_ce_focal"] == 0
    assert len(out["history"]) == 2 and all(np.isfinite(h["train_loss"]) for h in out["history"])
    assert all(0.0 < h["train_region"] < 1.0 and h["train_region"] < h["train_loss"] for h in out["history"])
    kw = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)["hyper_parameters"]["model"]["model_kwargs"]
    assert (kw["region_weight"], kw["region_alpha"], kw["region_beta"], kw["region_smooth"]) == (1.0, 0.5, 0.5, 1.0)
    ckpt = out["checkpoint"]                       # predict and infer build the model from the hyper_parameters alone
    summary = infer.infer(ckpt, [os.path.join(tree, "CSDAP_complete", "RegB", "S1")], str(tmp_path / "maps"))
    assert summary["n_scenes"] >= 1 and all(os.path.exists(r["output"]) for r in summary["scenes"])
    predict.main([ckpt, "--data_root", tree, "--batch_size", "4"])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert os.path.exists(os.path.join(res["pred_dir"], "metrics.json"))


def test_fit_without_the_flag_never_touches_the_region_entry_point(tree, tmp_path, capsys, monkeypatch):
    from floodplanet_code_amd import fit
    calls = _spy(monkeypatch)
    plain = fit.main(_fit_args(tree, str(tmp_path / "plain")))
    capsys.readouterr()
    assert calls["fu_loss_ce"] > 0 and calls["fu_loss_ce_region"] == 0
    assert all("train_region" not in h for h in plain["history"])
    kw = torch.load(plain["checkpoint"], map_location="cpu", weights_only=False)["hyper_parameters"]["model"]["model_kwargs"]
    assert not any(k.startswith("region_") for k in kw)
