"""CPU: LossOptions, the one checked value that carries the fused cross entropy's options from the command line to the C
call -- which entry point HipUNet._loss_raw picks for it and with which arguments (a recorder in place of the library),
the checks of LossOptions.make, the derived count of _UNetLossFn.backward, and that the models and the trainer keep one
loss_options the seven readable attributes agree with."""
import ctypes as C
import dataclasses
import inspect
import re

import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd.loss_options import LossOptions
from floodplanet_code_amd.models import build_model
from floodplanet_code_amd.unet import HipUNet, _UNetLossFn

from test_region_loss_cpu import BAD                    # the bad region sets of the host-side checks there

FIELDS = ("class_weight", "label_smoothing", "focal_gamma", "region_weight", "region_alpha", "region_beta", "region_smooth")
BAD_FOCAL = [dict(focal_gamma=-1), dict(focal_gamma=float("nan")), dict(focal_gamma=float("inf")),      # the four sets of
             dict(focal_gamma=2, label_smoothing=0.1)]                                                   # test_focal_loss_cpu
STREAM = 0x5EED


# ------------------------------------------------------------------------------------------------------- routing
class _Recorder:
    """Stands in for the loaded library: every attribute is a function that records (name, args) and returns FU_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _f32(v):
    return C.c_float(v).value


W3 = [0.5, 1.0, 2.0]
P, NULL = "P", "-"           # a non-null pointer, NULL
# (keywords, entry point, the arguments after (ctx, target, ignore_index): floats by value, "P" / "-" for pointers, a tuple
# for the FuRegionLoss fields, STREAM last)
ROWS = [
    (dict(), "fu_loss_ce", [P, P, NULL]),
    (dict(region_weight=0, region_alpha=0.3, region_beta=0.7, region_smooth=2.0), "fu_loss_ce", [P, P, NULL]),
    (dict(class_weight=W3), "fu_loss_ce_weighted", [P, 0.0, P, P, P, P]),
    (dict(label_smoothing=0.1), "fu_loss_ce_weighted", [NULL, 0.1, P, P, P, P]),
    (dict(class_weight=W3, label_smoothing=0.1), "fu_loss_ce_weighted", [P, 0.1, P, P, P, P]),
    (dict(focal_gamma=2), "fu_loss_ce_focal", [NULL, 2.0, P, P, P, P]),
    (dict(focal_gamma=0.5, class_weight=W3), "fu_loss_ce_focal", [P, 0.5, P, P, P, P]),
    (dict(region_weight=1), "fu_loss_ce_region", [NULL, 0.0, 0.0, (1.0, 0.5, 0.5, 1.0), P, P, NULL, NULL, P]),
    (dict(region_weight=0.5, region_alpha=0.3, region_beta=0.7, region_smooth=0.1), "fu_loss_ce_region",
     [NULL, 0.0, 0.0, (0.5, 0.3, 0.7, 0.1), P, P, NULL, NULL, P]),
    (dict(region_weight=1, class_weight=W3), "fu_loss_ce_region", [P, 0.0, 0.0, (1.0, 0.5, 0.5, 1.0), P, P, P, P, P]),
    (dict(region_weight=1, label_smoothing=0.1), "fu_loss_ce_region", [NULL, 0.1, 0.0, (1.0, 0.5, 0.5, 1.0), P, P, P, P, P]),
    (dict(region_weight=2, region_alpha=1, region_beta=1, focal_gamma=2, class_weight=W3), "fu_loss_ce_region",
     [P, 0.0, 2.0, (2.0, 1.0, 1.0, 1.0), P, P, P, P, P]),
]


def _one_call(rec, name, want, target, ignore_index):
    assert len(rec.calls) == 1, rec.calls                    # exactly one library call per loss
    got_name, args = rec.calls.pop()
    assert got_name == name
    assert args[0] is None and args[1] == target.data_ptr() and args[2] == ignore_index      # ctx (none on the CPU), t, ii
    assert args[-1] == STREAM
    rest = args[3:-1]
    assert len(rest) == len(want), (name, rest)
    for got, w in zip(rest, want):
        if w == P:
            assert isinstance(got, int) and got != 0, (name, rest)
        elif w == NULL:
            assert got is None, (name, rest)
        elif isinstance(w, tuple):
            assert isinstance(got, _lib.FuRegionLoss)
            assert (got.weight, got.alpha, got.beta, got.smooth) == tuple(_f32(v) for v in w)
        else:
            assert type(got) is float and got == w, (name, rest)


def test_loss_raw_routes_every_option_set_to_one_library_call(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(HipUNet, "_stream", staticmethod(lambda device: STREAM))
    net = HipUNet(2, 3, base_channels=8)
    t = torch.zeros(1, 16, 16, dtype=torch.int64)
    cpu = torch.device("cpu")
    seen_weighted = seen_region = False
    for kw, name, want in ROWS:
        sums_before, terms_before = net.last_weighted_sums(), net.last_region_terms()
        if not seen_weighted:
            assert sums_before is None
        if not seen_region:
            assert terms_before is None
        for form in ("keywords", "options"):
            if form == "keywords":
                loss = net._loss_raw(t, 1, cpu, **kw)
            else:
                loss = net._loss_raw(t, 1, cpu, options=LossOptions.make(net.n_classes, **kw))
            assert loss.shape == () and loss.dtype == torch.float32
            _one_call(rec, name, want, t, 1)
        sums_p = want[-3:-1] if name == "fu_loss_ce_region" else want[-2:]
        if name != "fu_loss_ce" and sums_p == [P, P]:
            seen_weighted = True
        seen_region = seen_region or name == "fu_loss_ce_region"
        assert (net.last_weighted_sums() is not None) == seen_weighted
        assert (net.last_region_terms() is not None) == seen_region
    assert seen_weighted and seen_region
    n_valid, wsum = net.last_weighted_sums()
    assert n_valid.dtype == torch.int64 and wsum.dtype == torch.float32 and n_valid.shape == wsum.shape == ()
    assert net.last_region_terms().shape == (1 + net.n_classes,)

    # kind='bce_dice': its own entry point, no confusion buffer
    fresh = HipUNet(2, 3, base_channels=8)
    for form in ({}, {"options": LossOptions.make(3, "bce_dice")}):
        fresh._loss_raw(t, 1, cpu, kind="bce_dice", dice_weight=0.25, **form)
        _one_call(rec, "fu_loss_bce_dice", [0.25, P], t, 1)
    assert fresh.pop_confusion() is None and fresh.last_weighted_sums() is None and fresh.last_region_terms() is None


def test_loss_raw_takes_options_or_keywords_not_both(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the GPU library was touched")))
    net = HipUNet(2, 3, base_channels=8)
    t = torch.zeros(1, 16, 16, dtype=torch.int64)
    with pytest.raises(TypeError):
        net._loss_raw(t, 0, torch.device("cpu"), options=LossOptions.make(3), focal_gamma=2.0)
    with pytest.raises(TypeError):
        net._loss_raw(t, 0, torch.device("cpu"), focal_gama=2.0)             # an unknown option is no option
    with pytest.raises(ValueError, match="unknown loss kind"):
        net._loss_raw(t, 0, torch.device("cpu"), kind="hinge")
    with pytest.raises(ValueError, match="label_smoothing"):                 # the range check of the weighted route
        net._loss_raw(t, 0, torch.device("cpu"), label_smoothing=1.5)


def test_the_weight_upload_is_cached_per_object(monkeypatch):
    """One host check and one upload per set of weights: the steps after the first find the device copy."""
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(HipUNet, "_stream", staticmethod(lambda device: STREAM))
    import floodplanet_code_amd.unet as U
    checks = []
    real = U.check_class_weight
    monkeypatch.setattr(U, "check_class_weight", lambda w, n: checks.append(1) or real(w, n))
    net = HipUNet(2, 3, base_channels=8)
    t = torch.zeros(1, 16, 16, dtype=torch.int64)
    opts = LossOptions.make(3, class_weight=(0.5, 1.0, 2.0))
    for _ in range(3):
        net._loss_raw(t, 0, torch.device("cpu"), options=opts)
    assert len(checks) == 1 and len({c[1][3] for c in rec.calls}) == 1


# ---------------------------------------------------------------------------------------------- LossOptions.make
def test_make_defaults_and_types():
    d = LossOptions.make()
    assert dataclasses.astuple(d) == (None, 0.0, 0.0, 0.0, 0.5, 0.5, 1.0) and d == LossOptions()
    assert tuple(f.name for f in dataclasses.fields(LossOptions)) == FIELDS
    o = LossOptions.make(3, class_weight=W3, label_smoothing=0, focal_gamma=2, region_weight=1, region_alpha=1,
                         region_beta=0, region_smooth=2)
    assert all(type(getattr(o, k)) is float for k in FIELDS[1:])
    assert o.class_weight is W3                                             # the object it was given, unchecked
    assert LossOptions.make(3, class_weight=[1.0]).class_weight == [1.0]    # (HipUNet._class_weight_dev checks, once)
    assert LossOptions.make(label_smoothing=7).label_smoothing == 7.0       # (checked on the weighted and region routes)
    assert o.region == (1.0, 1.0, 0.0, 2.0)
    assert o.as_kwargs() == dict(zip(FIELDS, dataclasses.astuple(dataclasses.replace(o, class_weight=None))),
                                 class_weight=W3)
    assert o.as_kwargs()["class_weight"] is W3
    assert LossOptions.make(3, **o.as_kwargs()) == o
    with pytest.raises(TypeError):
        LossOptions.make(3, focal_gama=2)


def test_make_is_frozen_and_hashable():
    o = LossOptions.make(3, focal_gamma=2)
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.focal_gamma = 1.0
    assert hash(o) == hash(LossOptions.make(focal_gamma=2.0)) and len({o, LossOptions.make(focal_gamma=2)}) == 1
    assert dataclasses.replace(o, class_weight=(1.0, 2.0, 3.0)).focal_gamma == 2.0


def test_make_raises_what_loss_raw_raises(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the GPU library was touched")))
    net = HipUNet(2, 3, base_channels=8)
    t = torch.zeros(1, 16, 16, dtype=torch.int64)
    for bad_set, match in ((BAD, "region_"), (BAD_FOCAL, "focal_gamma")):
        for bad in bad_set:
            with pytest.raises(ValueError, match=match) as e_make:
                LossOptions.make(3, **bad)
            with pytest.raises(ValueError, match=match) as e_raw:
                net._loss_raw(t, 0, torch.device("cpu"), **bad)
            assert str(e_make.value) == str(e_raw.value)
    # the order of the checks: the focal exponent, its kind, the region numbers, their kind, the class count
    with pytest.raises(ValueError, match="focal_gamma must be"):
        LossOptions.make(1, "bce_dice", focal_gamma=-1, region_weight=-1)
    with pytest.raises(ValueError, match="focal_gamma belongs to kind='ce'"):
        LossOptions.make(1, "bce_dice", focal_gamma=1, region_weight=-1)
    with pytest.raises(ValueError, match="region_weight must be"):
        LossOptions.make(1, "bce_dice", region_weight=-1, class_weight=W3)
    with pytest.raises(ValueError, match="region_weight belongs to kind='ce'"):
        LossOptions.make(1, "bce_dice", region_weight=1, class_weight=W3)
    with pytest.raises(ValueError, match="n_classes >= 2"):
        LossOptions.make(1, region_weight=1)
    assert LossOptions.make(None, region_weight=1).region_weight == 1.0     # class count not known here: not checked
    assert LossOptions.make(1, region_weight=0, region_alpha=1).region_alpha == 1.0


@pytest.mark.parametrize("kw", [dict(class_weight=[1.0, 1.0, 1.0]), dict(label_smoothing=0.1), dict(focal_gamma=2),
                                dict(region_weight=1.0), dict(region_alpha=0.3), dict(region_beta=0.7),
                                dict(region_smooth=2.0)])
def test_make_keeps_the_options_to_kind_ce(kw):
    with pytest.raises(ValueError, match="kind='ce'"):
        LossOptions.make(3, "bce_dice", **kw)
    assert LossOptions.make(3, "bce_dice") == LossOptions()


# --------------------------------------------------------------------------------------- LossOptions.from_args
def _args(*extra):
    from floodplanet_code_amd import fit
    return fit.build_parser().parse_args(["/data", "--exp_dir", "/exp", *extra])


def test_from_args_reads_every_loss_flag():
    assert LossOptions.from_args(_args(), 3) == LossOptions() and LossOptions.from_args(_args()).given_kwargs() == {}
    assert LossOptions.from_args(type("Namespace", (), {})()) == LossOptions()        # a namespace from before the options
    o = LossOptions.from_args(_args("--class_weights", "0", "1", "2.5", "--focal_gamma", "2", "--region_loss", "tversky",
                                    "--tversky", "0.3", "0.7", "--region_weight", "0.5", "--region_smooth", "2"), 3)
    assert o == LossOptions([0.0, 1.0, 2.5], 0.0, 2.0, 0.5, 0.3, 0.7, 2.0)
    assert all(type(getattr(o, k)) is float for k in FIELDS[1:])
    # the kinds: dice and jaccard fix (alpha, beta); the weight and the smoothing default to 1 once a kind is named
    assert LossOptions.from_args(_args("--region_loss", "dice")).region == (1.0, 0.5, 0.5, 1.0)
    assert LossOptions.from_args(_args("--region_loss", "jaccard", "--region_weight", "0.25")).region == (0.25, 1.0, 1.0, 1.0)
    assert LossOptions.from_args(_args("--label_smoothing", "0.1", "--region_loss", "dice")).label_smoothing == 0.1
    # 'balanced' stays a marker for the caller, whatever the class count; it is no model keyword
    b = LossOptions.from_args(_args("--class_weights", "balanced", "--label_smoothing", "0.05"), 3)
    assert b.class_weight == "balanced" and b.given_kwargs() == {"label_smoothing": 0.05}
    assert dataclasses.replace(b, class_weight=(0, 0.75, 1.5)).given_kwargs() == {"class_weights": [0.0, 0.75, 1.5],
                                                                                   "label_smoothing": 0.05}


@pytest.mark.parametrize("extra,message", [
    (("--region_weight", "1"), "--region_weight need --region_loss"),
    (("--tversky", "1", "2", "--region_smooth", "1"), "--tversky, --region_smooth need --region_loss"),
    (("--region_loss", "tversky"), "--region_loss tversky and --tversky A B go together"),
    (("--region_loss", "dice", "--tversky", "1", "1"), "--region_loss tversky and --tversky A B go together"),
    (("--region_loss", "dice", "--region_weight", "-1"), "region_weight must be finite and >= 0, got -1.0"),
    (("--region_loss", "tversky", "--tversky", "0", "0"),
     "region_alpha, region_beta must be finite and >= 0 with alpha + beta > 0, got 0.0, 0.0"),
    (("--focal_gamma", "-1"), "focal_gamma must be finite and >= 0, got -1.0"),
    (("--focal_gamma", "2", "--label_smoothing", "0.1"),
     "focal_gamma=2.0 together with label_smoothing=0.1: a smoothed focal loss is not defined here, set one of them to 0"),
    (("--class_weights", "heavy"), "--class_weights takes 'balanced' or one number per class, got ['heavy']"),
    (("--class_weights", "balanced", "1"), "--class_weights takes 'balanced' or one number per class, got ['balanced', '1']"),
    (("--class_weights", "1", "2"), "--class_weights: 2 weights for 3 classes"),
    # two mistakes on one line: class weights, then the focal exponent, then the region flags' rules, then their numbers
    (("--class_weights", "1", "2", "--region_weight", "1"), "--class_weights: 2 weights for 3 classes"),
    (("--class_weights", "heavy", "--focal_gamma", "-1"), "--class_weights takes 'balanced' or one number per class, got ['heavy']"),
    (("--focal_gamma", "-1", "--region_weight", "1"), "focal_gamma must be finite and >= 0, got -1.0"),
    (("--region_loss", "dice", "--tversky", "1", "1", "--region_weight", "-1"),
     "--region_loss tversky and --tversky A B go together"),
])
def test_from_args_states_the_command_lines_rules(extra, message):
    """The messages fit gave when these rules lived there."""
    with pytest.raises(ValueError) as e:
        LossOptions.from_args(_args(*extra), 3)
    assert str(e.value) == message


def test_given_kwargs_lists_what_is_set_in_the_configs_order():
    full = LossOptions.make(3, class_weight=(1, 2, 3), label_smoothing=0.1, region_weight=2, region_alpha=1, region_beta=1)
    assert list(full.given_kwargs().items()) == [("class_weights", [1.0, 2.0, 3.0]), ("label_smoothing", 0.1),
                                                 ("region_weight", 2.0), ("region_alpha", 1.0), ("region_beta", 1.0),
                                                 ("region_smooth", 1.0)]
    focal = LossOptions.make(3, class_weight=torch.tensor([1.0, 2.0, 3.0]), focal_gamma=2, region_weight=1)
    assert list(focal.given_kwargs()) == ["class_weights", "focal_gamma", "region_weight", "region_alpha", "region_beta",
                                          "region_smooth"]
    assert all(type(v) is float for v in focal.given_kwargs()["class_weights"])
    assert LossOptions.make(focal_gamma=1.5).given_kwargs() == {"focal_gamma": 1.5}
    assert LossOptions.make(region_weight=0, region_alpha=0.3).given_kwargs() == dict(     # the four travel together
        region_weight=0.0, region_alpha=0.3, region_beta=0.5, region_smooth=1.0)
    # a command line that names --region_loss records its four numbers whatever they are; one that does not, none
    off = LossOptions.make(region_weight=0)
    assert off == LossOptions() and off.given_kwargs() == {} and off.given_kwargs(region=False) == {}
    assert off.given_kwargs(region=True) == dict(region_weight=0.0, region_alpha=0.5, region_beta=0.5, region_smooth=1.0)
    assert list(focal.given_kwargs(region=True)) == list(focal.given_kwargs())
    for o in (full, focal, LossOptions()):                       # the keywords rebuild the value (class_weights -> class_weight)
        kw = o.given_kwargs()
        back = LossOptions.make(3, class_weight=kw.pop("class_weights", None), **kw)
        assert dataclasses.replace(back, class_weight=None) == dataclasses.replace(o, class_weight=None)
    m = build_model("ms_model", {"ms_image": 2}, 3, 1e-3, 50, None, ignore_index=0, base_channels=8, **full.given_kwargs())
    assert m.loss_options == dataclasses.replace(full, class_weight=(1.0, 2.0, 3.0))      # they are the model's keywords


def test_loss_options_module_needs_neither_torch_nor_the_library():
    import subprocess
    import sys
    code = ("import sys, importlib.util as u; s = u.spec_from_file_location('lo', sys.argv[1]); m = u.module_from_spec(s); "
            "sys.modules['lo'] = m; s.loader.exec_module(m); assert m.LossOptions.make(3, focal_gamma=2).focal_gamma == 2.0; "
            "assert 'torch' not in sys.modules and not any(k.endswith('_lib') for k in sys.modules)")
    import floodplanet_code_amd.loss_options as lo
    subprocess.run([sys.executable, "-c", code, lo.__file__], check=True)


# ---------------------------------------------------------------------------------------- _UNetLossFn.backward
def test_backward_derives_its_count_of_nones():
    params = list(inspect.signature(_UNetLossFn.forward).parameters.values())
    assert params[-1].kind is inspect.Parameter.VAR_POSITIONAL
    named = [p.name for p in params[:-1]]
    assert [n for n in named if n in FIELDS or "option" in n] == ["options"]          # one loss-options argument, no more
    src = inspect.getsource(_UNetLossFn.backward)
    assert not re.search(r"\(None,\)\s*\*\s*\d|\d\s*\*\s*\(None,\)", src)
    assert "(None, None" not in src

    class _Ctx:
        pass

    # the count itself, without a GPU: backward with everything behind the leading Nones stubbed out
    import floodplanet_code_amd.unet as U
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(U, "_check_generation", lambda ctx: None)
        mp.setattr(U, "_save_accumulated", lambda m: (None, None))
        mp.setattr(U, "_return_param_grads", lambda m, saved, alias: ("grads",))
        mp.setattr(U, "check", lambda status: None)
        mp.setattr(_lib, "load", lambda: _Recorder())
        ctx = _Ctx()
        ctx.device = torch.device("cpu")
        ctx.module = type("M", (), {"_ctx": None, "_stream": staticmethod(lambda d: 0),
                                    "_backward_raw": lambda self, d, dev: None})()
        out = _UNetLossFn.backward(ctx, torch.ones(()), None)
    finally:
        mp.undo()
    assert out == (None,) * (len(named) - 1) + ("grads",)                    # every forward argument but ctx and *params


# ------------------------------------------------------------------------------------------- models and trainer
def _agrees(holder, weights_name):
    o = holder.loss_options
    assert isinstance(o, LossOptions)
    got = tuple(getattr(holder, k) for k in FIELDS[1:])
    assert got == tuple(getattr(o, k) for k in FIELDS[1:]) and all(type(v) is float for v in got)
    assert getattr(holder, weights_name) is o.class_weight
    return o


@pytest.mark.parametrize("name", ["ms_model", "ef_model", "lf_model"])
def test_models_hold_one_loss_options(name, monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the GPU library was touched")))
    kw = dict(ignore_index=0, base_channels=8)
    assert _agrees(build_model(name, {"ms_image": 2}, 3, 1e-3, 50, None, **kw), "class_weights") == LossOptions()
    m = build_model(name, {"ms_image": 2}, 3, 1e-3, 50, None, class_weights=[0.0, 0.5, 2.0], focal_gamma=2.0,
                    region_weight=0.5, region_alpha=0.3, region_beta=0.7, region_smooth=2, **kw)
    assert _agrees(m, "class_weights") == LossOptions((0.0, 0.5, 2.0), 0.0, 2.0, 0.5, 0.3, 0.7, 2.0)
    assert [n for n, _ in m.named_children()][-1] == "loss_func"             # registered last: state_dict()'s order is kept
    # the set_loss_options calls of the weighted, focal and region tests
    assert m.set_loss_options([1, 2, 3], 0.0, 0.5) is m
    assert _agrees(m, "class_weights") == LossOptions((1.0, 2.0, 3.0), 0.0, 0.5)
    m.set_loss_options([1, 2, 3], 0.0, 0.5, 2.0, 1.0, 1.0, 0.5)
    assert _agrees(m, "class_weights") == LossOptions((1.0, 2.0, 3.0), 0.0, 0.5, 2.0, 1.0, 1.0, 0.5)
    m.replace_loss_options(class_weight=[3, 2, 1])                           # what fit does for --class_weights balanced
    assert _agrees(m, "class_weights") == LossOptions((3.0, 2.0, 1.0), 0.0, 0.5, 2.0, 1.0, 1.0, 0.5)
    assert torch.equal(m.loss_func.weight, torch.tensor([3.0, 2.0, 1.0]))
    m.set_loss_options([1, 2, 3], 0.25)
    assert _agrees(m, "class_weights") == LossOptions((1.0, 2.0, 3.0), 0.25)
    assert m.loss_func.label_smoothing == 0.25
    before = m.loss_options
    for bad in (dict(label_smoothing=0.1, focal_gamma=2.0), dict(label_smoothing=1.0), dict(class_weights=[1, 2])):
        with pytest.raises(ValueError):
            m.set_loss_options(**bad)
    assert m.loss_options is before                                          # a rejected call leaves the options as they were
    with pytest.raises(AttributeError):
        m.focal_gamma = 1.0                                                  # read-only views of loss_options


def test_trainer_holds_one_loss_options(monkeypatch):
    from floodplanet_code_amd.distributed import DataParallelTrainer
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the GPU library was touched")))
    net = HipUNet(2, 3, base_channels=8)
    assert _agrees(DataParallelTrainer(net, lr=1e-3), "class_weight") == LossOptions()
    w = torch.tensor([0.5, 1.0, 2.0])
    tr = DataParallelTrainer(net, lr=1e-3, class_weight=w, focal_gamma=2, region_weight=1, region_alpha=1, region_beta=1)
    assert _agrees(tr, "class_weight").region == (1.0, 1.0, 1.0, 1.0) and tr.class_weight is w and tr.focal_gamma == 2.0
    assert _agrees(DataParallelTrainer(net, lr=1e-3, label_smoothing=0.1), "class_weight").label_smoothing == 0.1
    with pytest.raises(ValueError, match="n_classes >= 2"):
        DataParallelTrainer(HipUNet(2, 1, base_channels=8), lr=1e-3, region_weight=1)
    assert not hasattr(tr, "_graph_off") and not hasattr(tr, "_region_kwargs")
