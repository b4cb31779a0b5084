"""CPU: OptimOptions, the one checked value that carries the optimiser's options (weight EMA, gradient clipping, decoupled
weight decay) from the command line to the net -- the checks of make and from_args, the model_kwargs a command line gives,
that the models and the trainer hold one optim_options their five readable attributes agree with, and which library calls a
new context (HipUNet._arm_optim) and the step (HipUNet.adam_step) make for it (a recorder in place of the library).  The
literal rows were recorded from the commit before OptimOptions existed: they pin that nothing a checkpoint or the library
sees has changed."""
import ctypes as C
import dataclasses
import inspect
import os

import pytest
import torch

import test_ema_cpu
import test_grad_clip_cpu
import test_weight_decay_cpu
from floodplanet_code_amd import _lib, fit
from floodplanet_code_amd.ema import check_decay, ema_weight
from floodplanet_code_amd.models import build_model
from floodplanet_code_amd.optim_options import KEYWORDS, OptimOptions, check_grad_clip, check_weight_decay
from floodplanet_code_amd.unet import HipAdam, HipUNet

from test_loss_options_cpu import _Recorder

STREAM = 0x5EED
FIELDS = ("ema_decay", "ema_warmup", "grad_clip_norm", "weight_decay", "decay_params")


# ------------------------------------------------------------------------------------------ the bad sets of the three files
def _bad_lines(test_fn):
    """the command lines a parametrised rejection test lists"""
    (mark,) = [m for m in test_fn.pytestmark if m.name == "parametrize"]
    return [tuple(line) for line in mark.args[1]]


BAD_LINES = (_bad_lines(test_ema_cpu.test_fit_rejects_bad_ema_flags)
             + _bad_lines(test_grad_clip_cpu.test_fit_rejects_bad_options_before_it_touches_the_data)
             + _bad_lines(test_weight_decay_cpu.test_fit_rejects_bad_options_before_it_touches_the_data))
VALUE_FLAGS = {"--ema_decay": "ema_decay", "--grad_clip": "grad_clip_norm", "--weight_decay": "weight_decay"}
SWITCHES = {"--no_ema_warmup": ("ema_warmup", False), "--decay_all": ("decay_all", True)}


def _args(*extra):
    return fit.build_parser().parse_args(["/data", "--exp_dir", "/exp", *extra])


def _as_keywords(line):
    """a command line of optimiser flags as make's keywords; None for a line with any other flag (the lr schedule's)"""
    kw, words = {}, list(line)
    while words:
        w = words.pop(0)
        if w in VALUE_FLAGS:
            kw[VALUE_FLAGS[w]] = float(words.pop(0))
        elif w in SWITCHES:
            kw[SWITCHES[w][0]] = SWITCHES[w][1]
        else:
            return None
    return kw


def test_the_imported_sets_are_the_ones_meant():
    assert len(BAD_LINES) == 3 + 6 + 5
    ours = [line for line in BAD_LINES if _as_keywords(line) is not None]
    assert len(ours) == 3 + 3 + 5 and {w for line in ours for w in line if w.startswith("--")} == set(VALUE_FLAGS) | set(SWITCHES)


@pytest.mark.parametrize("line", BAD_LINES)
def test_from_args_rejects_exactly_the_bad_optimiser_lines(line):
    if _as_keywords(line) is None:                   # the lr schedule's bad lines: not OptimOptions' to judge
        assert OptimOptions.from_args(_args(*line)) == OptimOptions()
        return
    with pytest.raises(ValueError) as e_new:
        OptimOptions.from_args(_args(*line))
    with pytest.raises(ValueError) as e_cfg:
        fit.cfg_from_args(_args(*line))
    assert str(e_new.value) == str(e_cfg.value)


@pytest.mark.parametrize("line", [line for line in BAD_LINES if _as_keywords(line) is not None])
def test_make_rejects_the_values_and_not_the_command_line_rules(line):
    """make runs the constructors' checks: a value outside its domain raises with the check's own message; what is bad on a
    command line only (0 for "on", a modifier without its option) is accepted."""
    kw = _as_keywords(line)
    checks = {"ema_decay": check_decay, "grad_clip_norm": check_grad_clip, "weight_decay": check_weight_decay}
    messages = []
    for name, check in checks.items():
        if name in kw:
            try:
                check(kw[name])
            except ValueError as e:
                messages.append(str(e))
    if messages:
        with pytest.raises(ValueError) as e_make:
            OptimOptions.make(**kw)
        assert str(e_make.value) in messages
        for holder in (lambda: build_model("ms_model", {"ms_image": 2}, 3, 1e-3, 50, None, ignore_index=0, base_channels=8, **kw),
                       lambda: _trainer(**kw)):
            with pytest.raises(ValueError) as e_holder:
                holder()
            assert str(e_holder.value) == str(e_make.value)
    else:
        o = OptimOptions.make(**kw)
        assert o.grad_clip_norm is None and o.weight_decay == 0.0 and o.ema_decay is None
        assert o.decay_all == kw.get("decay_all", False) and o.ema_warmup == kw.get("ema_warmup", True)


def test_make_defaults_types_and_round_trip():
    d = OptimOptions.make()
    assert dataclasses.astuple(d) == (None, True, None, 0.0, "weights") and d == OptimOptions()
    assert tuple(f.name for f in dataclasses.fields(OptimOptions)) == FIELDS
    assert list(inspect.signature(OptimOptions.make).parameters) == [
        "ema_decay", "ema_warmup", "grad_clip_norm", "weight_decay", "decay_all", "decay_params"]
    o = OptimOptions.make(ema_decay="0.5", ema_warmup=0, grad_clip_norm=2, weight_decay=1, decay_all=True)
    assert dataclasses.astuple(o) == (0.5, False, 2.0, 1.0, "all")
    assert [type(v) for v in dataclasses.astuple(o)] == [float, bool, float, float, str]
    assert o.as_kwargs() == dict(ema_decay=0.5, ema_warmup=False, grad_clip_norm=2.0, weight_decay=1.0, decay_all=True)
    assert tuple(o.as_kwargs()) == KEYWORDS and OptimOptions.make(**o.as_kwargs()) == o
    assert OptimOptions.make(grad_clip_norm=0).grad_clip_norm is None and OptimOptions.make(weight_decay=None).weight_decay == 0.0
    names = OptimOptions.make(weight_decay=0.1, decay_params=iter(["a.weight", "b.bias"]))
    assert names.decay_params == ("a.weight", "b.bias") and names.decay_all is False and hash(names) == hash(names)
    assert OptimOptions.make(decay_params="all").decay_all is True
    assert d.given_kwargs() == {} and d.set_fields == ()
    assert o.set_fields == ("ema_decay", "grad_clip_norm", "weight_decay")
    assert OptimOptions.make(decay_all=True).given_kwargs() == {"decay_all": True}           # accepted with weight_decay 0
    with pytest.raises(TypeError):
        OptimOptions.make(decay_all=True, decay_params="all")
    with pytest.raises(TypeError):
        OptimOptions.make(weight_dacay=0.1)
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.weight_decay = 0.0


def test_optim_options_module_needs_neither_torch_nor_the_library():
    import subprocess
    import sys
    code = ("import sys, importlib; m = importlib.import_module('floodplanet_code_amd.optim_options'); "
            "assert m.OptimOptions.make(weight_decay=0.5).weight_decay == 0.5; "
            "assert 'torch' not in sys.modules and not any(k.endswith('_lib') for k in sys.modules)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(os.path.dirname(fit.__file__)))


def test_unet_still_exports_the_checks_and_hipadam():
    import floodplanet_code_amd.unet as U
    import floodplanet_code_amd.unet_optim as UO
    assert U.check_grad_clip is check_grad_clip and U.check_weight_decay is check_weight_decay
    assert U.HipAdam is UO.HipAdam and issubclass(HipUNet, UO._OptimMixin)
    for name in ("enable_ema", "disable_ema", "ema_weights", "ema_state_dict", "load_ema_state_dict", "adam_step", "adam_state",
                 "set_grad_clip", "grad_clip_state", "set_weight_decay", "decayed_parameter_names", "grad_norms",
                 "fp16_guard_state", "apply_optim_options", "optim_key", "_arm_optim", "_bind", "_decay_key"):
        assert callable(getattr(HipUNet, name)), name


# ------------------------------------------------------------------------------------------ model_kwargs, key for key
# (command line, list(model_kwargs.items())) as the parent commit's cfg_from_args gave them: keys, order and values
MODEL_KWARGS = [
    ((), [('optimizer_name', 'adam'), ('base_channels', 64), ('precision', 'fp32')]),
    (('--ema_decay', '0.99'), [('optimizer_name', 'adam'), ('base_channels', 64), ('precision', 'fp32'), ('ema_decay', 0.99),
                               ('ema_warmup', True)]),
    (('--grad_clip', '1.5'), [('optimizer_name', 'adam'), ('base_channels', 64), ('precision', 'fp32'), ('grad_clip_norm', 1.5)]),
    (('--weight_decay', '0.01'), [('optimizer_name', 'adam'), ('base_channels', 64), ('precision', 'fp32'),
                                  ('weight_decay', 0.01)]),
    (('--ema_decay', '0.99', '--grad_clip', '1.5', '--weight_decay', '0.01'),
     [('optimizer_name', 'adam'), ('base_channels', 64), ('precision', 'fp32'), ('ema_decay', 0.99), ('ema_warmup', True),
      ('grad_clip_norm', 1.5), ('weight_decay', 0.01)]),
    (('--ema_decay', '0.99', '--no_ema_warmup'), [('optimizer_name', 'adam'), ('base_channels', 64), ('precision', 'fp32'),
                                                  ('ema_decay', 0.99), ('ema_warmup', False)]),
    (('--weight_decay', '0.02', '--decay_all'), [('optimizer_name', 'adam'), ('base_channels', 64), ('precision', 'fp32'),
                                                 ('weight_decay', 0.02), ('decay_all', True)]),
    (('--ema_decay', '0.9', '--no_ema_warmup', '--grad_clip', '2', '--weight_decay', '0.05', '--decay_all'),
     [('optimizer_name', 'adam'), ('base_channels', 64), ('precision', 'fp32'), ('ema_decay', 0.9), ('ema_warmup', False),
      ('grad_clip_norm', 2.0), ('weight_decay', 0.05), ('decay_all', True)]),
]


@pytest.mark.parametrize("line,want", MODEL_KWARGS)
def test_model_kwargs_of_a_command_line_are_what_they_were(line, want):
    kw = fit.cfg_from_args(_args(*line))["model"]["model_kwargs"]
    assert list(kw.items()) == want
    assert [type(v) for v in kw.values()] == [type(v) for _, v in want]
    given = OptimOptions.from_args(_args(*line)).given_kwargs()
    assert list(given.items()) == want[3:]
    assert OptimOptions.make(**given) == OptimOptions.from_args(_args(*line))     # what a checkpoint's keys rebuild


# ------------------------------------------------------------------------------------------ models and trainer
def _trainer(**kw):
    from floodplanet_code_amd.distributed import DataParallelTrainer
    return DataParallelTrainer(HipUNet(2, 3, base_channels=8), lr=1e-3, **kw)


def _agrees(holder):
    o = holder.optim_options
    assert isinstance(o, OptimOptions)
    assert {k: getattr(holder, k) for k in KEYWORDS} == o.as_kwargs()
    for k in KEYWORDS:
        with pytest.raises(AttributeError):
            setattr(holder, k, 0.5)                  # read-only views of optim_options
    return o


ALL_ON = dict(ema_decay=0.99, ema_warmup=False, grad_clip_norm=0.25, weight_decay=0.05, decay_all=True)


@pytest.mark.parametrize("name", ["ms_model", "ef_model", "lf_model"])
def test_models_hold_one_optim_options(name, monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the GPU library was touched")))
    kw = dict(ignore_index=0, base_channels=8)
    assert _agrees(build_model(name, {"ms_image": 2}, 3, 1e-3, 50, None, **kw)) == OptimOptions()
    m = build_model(name, {"ms_image": 2}, 3, 1e-3, 50, None, **ALL_ON, **kw)
    assert _agrees(m) == OptimOptions(0.99, False, 0.25, 0.05, "all")
    # the EMA is armed at construction, clipping and decay with the optimiser
    assert m.model._ema == (0.99, False) and m.model.grad_clip is None and m.model.weight_decay == 0.0
    opt = m.configure_optimizers()
    assert isinstance(opt, HipAdam) and m.model.optim_key() == (True, 0.25, (0.05, (True,) * len(m.model._table)))
    assert opt.param_groups[0]["weight_decay"] == 0.05 and m.model._ema == (0.99, False)
    zero = build_model(name, {"ms_image": 2}, 3, 1e-3, 50, None, decay_all=True, **kw)          # accepted, arms nothing
    assert _agrees(zero).decay_all is True and zero.configure_optimizers()._net.weight_decay == 0.0


@pytest.mark.parametrize("option,word", [(dict(ema_decay=0.9), "weight EMA"), (dict(grad_clip_norm=1.0), "gradient clipping"),
                                         (dict(weight_decay=0.1), "weight decay")])
def test_torch_adam_refuses_each_option_with_its_own_message(option, word, monkeypatch):
    m = build_model("ms_model", {"ms_image": 2}, 3, 1e-4, 50, None, ignore_index=0, base_channels=8, **option)
    monkeypatch.setenv("FU_TORCH_ADAM", "1")
    (name,) = option
    with pytest.raises(NotImplementedError, match=f"{word} .*FU_TORCH_ADAM=1 together with {name} is not supported"):
        m.configure_optimizers()
    plain = build_model("ms_model", {"ms_image": 2}, 3, 1e-4, 50, None, ignore_index=0, base_channels=8)
    assert type(plain.configure_optimizers()) is torch.optim.Adam


def test_trainer_holds_one_optim_options(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the GPU library was touched")))
    assert _agrees(_trainer()) == OptimOptions()
    tr = _trainer(**ALL_ON)
    assert _agrees(tr) == OptimOptions(0.99, False, 0.25, 0.05, "all")
    assert tr.net.optim_key() == (True, 0.25, (0.05, (True,) * len(tr.net._table))) and tr._g_optim is None
    assert not any(hasattr(tr, k) for k in ("_g_ema", "_g_clip", "_g_decay"))
    # a field left at "off" leaves the net's setting alone
    net = HipUNet(2, 3, base_channels=8).enable_ema(0.5).set_grad_clip(2.0).set_weight_decay(0.3)
    from floodplanet_code_amd.distributed import DataParallelTrainer
    DataParallelTrainer(net, lr=1e-3)
    assert net._ema == (0.5, True) and net.grad_clip == 2.0 and net.weight_decay == 0.3
    # ... for the trainer; HipAdam's param_groups own the decay, so its 0 disarms the net (and nothing else)
    opt = HipAdam(net, lr=1e-3)
    assert net._ema == (0.5, True) and net.grad_clip == 2.0 and net.weight_decay == 0.0 and opt.param_groups[0]["weight_decay"] == 0.0


def test_hipadam_takes_options_or_keywords_not_both():
    o = OptimOptions.make(ema_decay=0.9, grad_clip_norm=0.5, weight_decay=0.01, decay_all=True)
    net = HipUNet(2, 3, base_channels=8)
    opt = HipAdam(net, lr=2e-3, options=o)
    assert net.optim_key() == (False, 0.5, (0.01, (True,) * len(net._table)))            # the EMA is not HipAdam's to arm
    assert opt.param_groups[0]["weight_decay"] == 0.01 and opt.state_dict()["decay_params"] == net.decayed_parameter_names()
    same = HipUNet(2, 3, base_channels=8)
    HipAdam(same, lr=2e-3, max_grad_norm=0.5, weight_decay=0.01, decay_params="all")
    assert same.optim_key() == net.optim_key()
    for extra in (dict(max_grad_norm=1.0), dict(weight_decay=0.1), dict(decay_params="all")):
        with pytest.raises(TypeError, match="one or the other"):
            HipAdam(HipUNet(2, 3, base_channels=8), options=o, **extra)
    assert len(inspect.getdoc(HipAdam).splitlines()[0]) <= 120


# ------------------------------------------------------------------------------------------ the library calls
P, NULL, S = "P", "-", "S"           # a non-null pointer, NULL, the stream
BIND = ("fu_bind_buffers", [NULL, P, P, P, P, P])
MOMENTS = ("fu_bind_adam_state", [NULL, P, P])
EMA_OFF, EMA_ON = ("fu_bind_ema_state", [NULL, NULL, NULL, NULL]), ("fu_bind_ema_state", [NULL, P, P, P])
CHANGED = ("fu_params_changed", [NULL])
CLIP = ("fu_set_grad_clip", [NULL, 0.5])
DECAY = ("fu_set_weight_decay", [NULL, 0.01, P, 74])
ADAM = ("fu_adam_step", [NULL, 0.002, 0.8, 0.99, 1e-07, 3, 0.5, S])
ADAM_EMA = ("fu_adam_ema_step", [NULL, 0.002, 0.8, 0.99, 1e-07, 3, 0.5, 0.6923076923076923, S])
# (options, the calls that arm a new context, the step's call) as the parent commit's _get_ctx tail and adam_step made them
ROWS = [
    (dict(), [BIND, MOMENTS, EMA_OFF, CHANGED], ADAM),
    (dict(weight_decay=0.01), [BIND, MOMENTS, EMA_OFF, CHANGED, DECAY], ADAM),
    (dict(grad_clip_norm=0.5), [BIND, MOMENTS, EMA_OFF, CHANGED, CLIP], ADAM),
    (dict(grad_clip_norm=0.5, weight_decay=0.01), [BIND, MOMENTS, EMA_OFF, CHANGED, CLIP, DECAY], ADAM),
    (dict(ema_decay=0.9), [BIND, MOMENTS, EMA_ON, CHANGED], ADAM_EMA),
    (dict(ema_decay=0.9, weight_decay=0.01), [BIND, MOMENTS, EMA_ON, CHANGED, DECAY], ADAM_EMA),
    (dict(ema_decay=0.9, grad_clip_norm=0.5), [BIND, MOMENTS, EMA_ON, CHANGED, CLIP], ADAM_EMA),
    (dict(ema_decay=0.9, grad_clip_norm=0.5, weight_decay=0.01), [BIND, MOMENTS, EMA_ON, CHANGED, CLIP, DECAY], ADAM_EMA),
    (dict(ema_decay=0.9, grad_clip_norm=0.5, weight_decay=0.01, decay_params="all"),
     [BIND, MOMENTS, EMA_ON, CHANGED, CLIP, DECAY], ADAM_EMA),
    (dict(weight_decay=0.01, decay_params="names"), [BIND, MOMENTS, EMA_OFF, CHANGED, DECAY], ADAM),
]


def _normalised(calls):
    """(name, args) with floats by value, pointers as P / NULL, the stream as S, small integers (counts, the step) as they are"""
    rows = []
    for name, args in calls:
        out = []
        for a in args:
            if a is None:
                out.append(NULL)
            elif type(a) is float:
                out.append(a)
            elif isinstance(a, C.Array):
                out.append(P)
            elif a == STREAM:
                out.append(S)
            else:
                assert type(a) is int, (name, a)
                out.append(P if a > 4096 else a)
        rows.append((name, out))
    return rows


@pytest.mark.parametrize("kw,arm,step", ROWS)
def test_arming_a_context_and_the_step_make_the_calls_they_made(kw, arm, step, monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(HipUNet, "_stream", staticmethod(lambda device: STREAM))
    net = HipUNet(2, 3, base_channels=8)
    net._flatten(torch.device("cpu"))
    names = [k for k, _ in net.named_parameters()]
    pick = [names[0], names[3], names[-1]]
    if kw.get("decay_params") == "names":
        kw = dict(kw, decay_params=pick)
    options = OptimOptions.make(**kw)
    assert net.apply_optim_options(options) is net and not rec.calls             # no context yet: host bookkeeping only
    decayed = {"weights": [k for k, p in net.named_parameters() if p.ndim >= 2], "all": names}.get(options.decay_params, pick)
    assert net.decayed_parameter_names() == (decayed if options.weight_decay else [])
    assert net.optim_key() == (options.ema_decay is not None, options.grad_clip_norm, net._decay_key())
    net._arm_optim(None)
    assert _normalised(rec.calls) == arm
    if options.weight_decay:
        mask = rec.calls[-1][1][2]
        assert [bool(f) for f in mask] == [k in decayed for k in names]
    rec.calls.clear()
    net.adam_step(2e-3, 3, (0.8, 0.99), 1e-7, grad_scale=0.5)
    assert _normalised(rec.calls) == [step]
    if options.ema_decay is not None:
        assert rec.calls[0][1][7] == ema_weight(0.9, 3, True) == step[1][7]


def test_apply_optim_options_arms_the_parts_it_is_asked_to():
    o = OptimOptions.make(ema_decay=0.9, grad_clip_norm=0.5, weight_decay=0.01)
    net = HipUNet(2, 3, base_channels=8).apply_optim_options(o, step=False)
    assert net.optim_key() == (True, None, None)
    net = HipUNet(2, 3, base_channels=8).apply_optim_options(o, ema=False)
    assert net.optim_key()[:2] == (False, 0.5) and net.weight_decay == 0.01
    with pytest.raises(KeyError):
        HipUNet(2, 3, base_channels=8).apply_optim_options(OptimOptions.make(weight_decay=0.1, decay_params=["no.such"]))
