"""CPU: the surface of the decoupled weight decay (AdamW) in the fused Adam step -- header, bindings, argument checks, the nine
scalars, the Python keywords and fit's command line -- and the statement the GPU tests compare against
(tests/tools/adamw_ref.py), pinned bit for bit against torch.optim.AdamW(foreach=False)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib, fit
from tools import adamw_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fu_set_weight_decay", "fu_adamw_scalars", "fu_weight_decay_state")
ADAM = (1e-3, 0.9, 0.999, 1e-8)


# ------------------------------------------------------------------------------------------------------------ 1. C ABI
def test_header_declares_the_entries_and_the_abi_stays_5():
    txt = open(os.path.join(ROOT, "include", "floodunet.h")).read()
    assert int(re.search(r"#define\s+FU_ABI_VERSION\s+(\d+)", txt).group(1)) == 5      # additive: no version bump
    assert re.search(r"int\s+fu_set_weight_decay\(fu_ctx\*\s*ctx,\s*double\s+weight_decay,\s*const\s+uint8_t\*\s*decay_mask,"
                     r"\s*int\s+n_mask\);", txt)
    assert re.search(r"int\s+fu_adamw_scalars\(double\s+lr,\s*double\s+beta1,\s*double\s+beta2,\s*double\s+eps,\s*int64_t\s+step,"
                     r"\s*double\s+grad_scale,\s*double\s+ema_weight,\s*double\s+weight_decay,\s*float\s+out\[9\]\);", txt)
    assert re.search(r"int\s+fu_weight_decay_state\(const\s+fu_ctx\*\s*ctx,\s*double\*\s*weight_decay,\s*uint8_t\*\s*mask_out,"
                     r"\s*int\s+n_mask\);", txt)
    for word in ("torch.optim.AdamW", "(float)(1.0 - lr * weight_decay)", "NINE floats", "TOO SHORT", "ndim >= 2",
                 "before capturing a step"):
        assert word in txt, word                                       # documented as the other entries are


def test_library_binds_the_entries_and_checks_their_arguments():
    lib = _lib.load()
    assert lib.fu_abi_version() == 5
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None, name
    mask = (C.c_uint8 * 4)(1, 0, 1, 0)
    wd = C.c_double(-1.0)
    assert lib.fu_set_weight_decay(None, 0.01, None, 0) == _lib.FU_ERR_INVALID     # null context, before anything touches a device
    assert lib.fu_set_weight_decay(None, 0.01, mask, 4) == _lib.FU_ERR_INVALID
    assert lib.fu_weight_decay_state(None, C.byref(wd), None, 0) == _lib.FU_ERR_INVALID and wd.value == -1.0
    out = (C.c_float * 9)()
    for bad in (-0.01, float("nan"), float("inf"), -float("inf")):
        assert lib.fu_adamw_scalars(*ADAM, 1, 1.0, 0.0, bad, out) == _lib.FU_ERR_INVALID, bad
    assert lib.fu_adamw_scalars(*ADAM, 0, 1.0, 0.0, 0.01, out) == _lib.FU_ERR_INVALID          # step is 1-based
    assert lib.fu_adamw_scalars(*ADAM, 1, 1.0, 1.5, 0.01, out) == _lib.FU_ERR_INVALID          # EMA weight outside [0, 1]
    assert lib.fu_adamw_scalars(*ADAM, 1, 1.0, 0.0, 0.01, None) == _lib.FU_ERR_INVALID


def _bits(values):
    return np.asarray(list(values), dtype=np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("step", [1, 2, 7, 1000])
def test_adamw_scalars(step):
    """Slots 0-6: fu_adam_scalars' bits; slot 7: the EMA weight; slot 8: float32(1 - lr * wd), exactly 1 for wd = 0."""
    lib = _lib.load()
    for lr in (1e-3, 2e-3, 3.3e-4, 1e-5, 0.1, 1.0):
        for wd in (0.0, 1e-4, 0.01, 0.05, 0.3, 1.0, 7.5):
            for gscale, w in ((1.0, 0.0), (0.125, 0.37), (1.0 / 3.0, 1.0)):
                seven, nine = (C.c_float * 7)(), (C.c_float * 9)()
                _lib.check(lib.fu_adam_scalars(lr, 0.9, 0.999, 1e-8, step, gscale, seven))
                _lib.check(lib.fu_adamw_scalars(lr, 0.9, 0.999, 1e-8, step, gscale, w, wd, nine))
                assert _bits(nine)[:7] == _bits(seven)
                assert _bits([nine[7]]) == _bits([np.float32(w)])
                assert _bits([nine[8]]) == _bits([np.float32(1.0 - lr * wd)]) == _bits([adamw_ref.decay_factor(lr, wd)])
                if wd == 0.0:
                    assert nine[8] == 1.0
                eight = (C.c_float * 8)()
                _lib.check(lib.fu_adam_ema_scalars(lr, 0.9, 0.999, 1e-8, step, gscale, w, eight))
                assert _bits(nine)[:8] == _bits(eight)


# ------------------------------------------------------------------------------------------------------------ 2. the reference
def test_adamw_ref_is_torch_adamw_bit_for_bit():
    """tests/tools/adamw_ref.py against torch.optim.AdamW(foreach=False) on the CPU: two parameter groups (decay / no decay),
    7 steps, a changing lr, tensor sizes that are no multiples of 4, gradients spanning 1e-2 .. 1e1, with and without a
    gradient scale folded into the gradients -- parameters and both moments equal as bit patterns after every step."""
    gen = torch.Generator().manual_seed(11)
    shapes = [(5, 3, 3, 3), (5,), (7, 5, 3, 3), (7,), (3, 7, 1, 1), (3,), (1,), (2, 9)]
    decays = [len(s) >= 2 for s in shapes]
    wd, betas, eps = 0.05, (0.9, 0.999), 1e-8
    assert any(int(np.prod(s)) % 4 for s in shapes)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen) * 0.3) for s in shapes]
    opt = torch.optim.AdamW([{"params": [p for p, d in zip(params, decays) if d], "weight_decay": wd},
                             {"params": [p for p, d in zip(params, decays) if not d], "weight_decay": 0.0}],
                            lr=1e-3, betas=betas, eps=eps, foreach=False)
    sizes = [int(np.prod(s)) for s in shapes]
    table = [(sum(sizes[:k]), n) for k, n in enumerate(sizes)]
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).clone()                 # noqa: E731
    p, m, v = flat(params), torch.zeros(sum(sizes)), torch.zeros(sum(sizes))
    for t in range(1, 8):
        lr = 1e-3 * (1.0 + 0.5 * np.cos(t)) * (0.5 if t % 3 == 0 else 1.0)
        grads = [torch.randn(s, generator=gen) * 10.0 ** float(t % 4 - 2) for s in shapes]     # 1e-2 .. 1e1
        for q, g in zip(params, grads):
            q.grad = g.clone()
        for group in opt.param_groups:
            group["lr"] = lr
        opt.step()
        adamw_ref.step_flat(p, flat(grads), m, v, table, decays, lr, betas, eps, t, wd)
        want_m = flat([opt.state[q]["exp_avg"] for q in params])
        want_v = flat([opt.state[q]["exp_avg_sq"] for q in params])
        for name, got, want in (("p", p, flat(params)), ("m", m, want_m), ("v", v, want_v)):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (t, name, adamw_ref.max_abs_diff(got, want))
    # the decay acted, and only where it should: against plain Adam on the same inputs the decayed tensors differ
    q = flat(params)
    plain_p, plain_m, plain_v = flat([torch.zeros(s) for s in shapes]), torch.zeros(sum(sizes)), torch.zeros(sum(sizes))
    g = torch.ones(sum(sizes))
    both = []
    for flags in (decays, [False] * len(shapes)):
        a, b, c = q.clone(), plain_m.clone(), plain_v.clone()
        adamw_ref.step_flat(a, g, b, c, table, flags, 1e-3, betas, eps, 1, wd)
        both.append((a, b, c))
    assert torch.equal(both[0][1], both[1][1]) and torch.equal(both[0][2], both[1][2])         # the moments never see the decay
    for (off, n), d in zip(table, decays):
        assert torch.equal(both[0][0][off:off + n], both[1][0][off:off + n]) != d
    assert plain_p.abs().sum() == 0


# ------------------------------------------------------------------------------------------------------------ 3. Python surface
def test_python_surface_takes_the_new_keywords():
    from floodplanet_code_amd.distributed import DataParallelTrainer
    from floodplanet_code_amd.models import WaterSegmentationModel
    from floodplanet_code_amd.unet import HipAdam, HipUNet, check_weight_decay
    sig = inspect.signature(HipAdam.__init__).parameters
    assert sig["weight_decay"].default == 0.0 and sig["decay_params"].default == "weights"
    for cls in (WaterSegmentationModel, DataParallelTrainer):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["weight_decay"].default == 0.0 and sig["decay_all"].default is False, cls
    assert list(inspect.signature(HipUNet.adam_step).parameters) == ["self", "lr", "step", "betas", "eps", "grad_scale"]
    assert check_weight_decay(None) == 0.0 and check_weight_decay(0) == 0.0 and check_weight_decay("0.5") == 0.5
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            check_weight_decay(bad)


def test_set_weight_decay_bookkeeping_without_a_context():
    from floodplanet_code_amd.unet import HipUNet
    net = HipUNet(3, 3, base_channels=8)
    names = [k for k, _ in net.named_parameters()]
    assert net.weight_decay == 0.0 and net.decayed_parameter_names() == []
    assert net.set_weight_decay(0.01) is net and net.weight_decay == 0.01
    want = [k for k, p in net.named_parameters() if p.ndim >= 2]
    assert net.decayed_parameter_names() == want and 0 < len(want) < len(names)       # the default mask: exactly ndim >= 2
    assert all(k.endswith(".weight") for k in want)
    assert not [k for k in want if net.get_parameter(k).ndim < 2]
    bn_and_bias = [k for k in names if k not in want]
    assert all(net.get_parameter(k).ndim == 1 for k in bn_and_bias)
    assert net.set_weight_decay(0.02, "all").decayed_parameter_names() == names and net.weight_decay == 0.02
    pick = [names[5], names[0], names[-1]]
    assert net.set_weight_decay(0.03, iter(pick)).decayed_parameter_names() == [names[0], names[5], names[-1]]
    assert net._decay_key() == (0.03, tuple(k in pick for k in names))
    assert net.set_weight_decay(0.03, []).decayed_parameter_names() == [] and net._decay_key() is None
    assert net.set_weight_decay(None).weight_decay == 0.0 and net.decayed_parameter_names() == []
    assert net.set_weight_decay(0).weight_decay == 0.0 and net._decay_key() is None
    with pytest.raises(KeyError):
        net.set_weight_decay(0.01, ["inc.double_conv.0.weight", "no.such.tensor"])
    with pytest.raises(ValueError):
        net.set_weight_decay(0.01, "biases")
    with pytest.raises(ValueError):
        net.set_weight_decay(-0.01)
    assert net.weight_decay == 0.0                                     # a rejected call changes nothing


def test_hipadam_param_groups_and_the_model():
    from floodplanet_code_amd.models import WaterSegmentationModel
    from floodplanet_code_amd.unet import HipAdam, HipUNet
    net = HipUNet(3, 3, base_channels=8)
    opt = HipAdam(net, lr=2e-3, weight_decay=0.01)
    g = opt.param_groups[0]
    assert isinstance(opt, torch.optim.Adam)
    assert (g["lr"], g["weight_decay"], g["decoupled_weight_decay"], g["amsgrad"]) == (2e-3, 0.01, True, False)
    assert net.weight_decay == 0.01 and len(net.decayed_parameter_names()) == sum(p.ndim >= 2 for p in net.parameters())
    sd = opt.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 0.01 and sd["decay_params"] == net.decayed_parameter_names()
    plain = HipAdam(HipUNet(3, 3, base_channels=8), lr=2e-3)
    assert plain.param_groups[0]["weight_decay"] == 0.0 and "decay_params" not in plain.state_dict()
    assert plain._net.weight_decay == 0.0 and plain._net.decayed_parameter_names() == []
    every = HipAdam(HipUNet(3, 3, base_channels=8), weight_decay=0.1, decay_params="all")
    assert every._net.decayed_parameter_names() == [k for k, _ in every._net.named_parameters()]
    with pytest.raises(ValueError):
        HipAdam(HipUNet(3, 3, base_channels=8), weight_decay=-1.0)
    m = WaterSegmentationModel({"ms_image": 3}, 3, 1e-3, ignore_index=0, base_channels=8, weight_decay=0.05)
    assert m.weight_decay == 0.05 and m.decay_all is False and m.model.weight_decay == 0.0    # armed with the optimiser
    mopt = m.configure_optimizers()
    assert m.model.weight_decay == 0.05 and mopt.param_groups[0]["weight_decay"] == 0.05
    assert all(m.model.get_parameter(k).ndim >= 2 for k in m.model.decayed_parameter_names())
    m = WaterSegmentationModel({"ms_image": 3}, 3, 1e-3, ignore_index=0, base_channels=8, weight_decay=0.05, decay_all=True)
    m.configure_optimizers()
    assert len(m.model.decayed_parameter_names()) == len(list(m.model.parameters()))
    with pytest.raises(ValueError):
        WaterSegmentationModel({"ms_image": 3}, 3, 1e-3, ignore_index=0, base_channels=8, weight_decay=float("nan"))


# ------------------------------------------------------------------------------------------------------------ 4. fit's command line
def _args(*extra):
    return fit.build_parser().parse_args(["/data", "--exp_dir", "/exp", *extra])


def test_fit_parser_takes_the_options_and_a_plain_line_is_unchanged():
    plain = fit.cfg_from_args(_args())
    assert not {"weight_decay", "decay_all"} & set(plain["model"]["model_kwargs"])
    cfg = fit.cfg_from_args(_args("--weight_decay", "0.01"))
    assert cfg["model"]["model_kwargs"]["weight_decay"] == 0.01 and "decay_all" not in cfg["model"]["model_kwargs"]
    assert {k: v for k, v in cfg.items() if k != "model"} == {k: v for k, v in plain.items() if k != "model"}
    cfg = fit.cfg_from_args(_args("--weight_decay", "0.02", "--decay_all", "--lr_schedule", "cosine"))
    kw = cfg["model"]["model_kwargs"]
    assert (kw["weight_decay"], kw["decay_all"], cfg["lr_schedule"]) == (0.02, True, "cosine")


@pytest.mark.parametrize("extra", [("--weight_decay", "-0.01"), ("--weight_decay", "0"), ("--weight_decay", "nan"),
                                   ("--weight_decay", "inf"), ("--decay_all",)])
def test_fit_rejects_bad_options_before_it_touches_the_data(extra, capsys):
    with pytest.raises(ValueError):
        fit.cfg_from_args(_args(*extra))
    with pytest.raises(SystemExit):
        fit.main(["/nonexistent", "--exp_dir", "/nonexistent", *extra])
    with pytest.raises(SystemExit):
        _args("--weight_decay", "much")
    capsys.readouterr()
