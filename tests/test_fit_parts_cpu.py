"""CPU: the parts fit_model and fit.main are made of, each on its own with plain Python stand-ins for the model, the
optimiser and the loaders -- history_entry (which keys, when, in which order), TopKCheckpoints (which files stay, which is
best, ties), train_epoch (the schedule's lr ahead of every step, steps counted across epochs), validate,
LrSchedule.from_cfg, run_summary's keys, and fit_model itself over the stand-ins."""
import contextlib
import itertools
import os

import pytest
import torch

from floodplanet_code_amd import fit
from floodplanet_code_amd.schedule import LrSchedule, lr_at

FIRST = ["epoch", "train_loss", "val_MulticlassJaccardIndex", "train_tiles_per_s"]


# ------------------------------------------------------------------------------------------------------- stand-ins
class _Loss:
    def __init__(self, value, log):
        self.value, self.log = value, log

    def backward(self):
        self.log.append("backward")

    def detach(self):
        return self.value


class _Net:
    def __init__(self, log):
        self.log = log

    def last_region_terms(self):
        self.log.append("read region")
        return [0.25, 0.0, 0.0]

    def grad_clip_state(self):
        self.log.append("read clip")
        return {"grad_norm": 3.5, "clipped_steps": 2, "max_norm": 1.0}

    def decayed_parameter_names(self):
        return ["a", "b", "c"]


class _Model:
    """What fit_model touches of a WaterSegmentationModel; every call is logged."""

    def __init__(self, mious=(), region_weight=0.0, grad_clip_norm=None, weight_decay=0.0):
        self.log, self.global_step, self.current_epoch, self.logged = [], 0, None, {}
        self.model, self.region_weight, self.weight_decay, self.class_weights = _Net(self.log), region_weight, weight_decay, None
        self.optim_options = type("O", (), {"grad_clip_norm": grad_clip_norm, "weight_decay": weight_decay})()
        self.valid_metrics = type("M", (), {"reset": lambda s: self.log.append("reset")})()
        self._mious = iter(mious)

    def to(self, device):
        return self

    def configure_optimizers(self):
        return _Opt(self.log, weight_decay=self.weight_decay)

    def training_step(self, batch, i):
        self.log.append(("train", i))
        return _Loss(float(batch["loss"]), self.log)

    def validation_step(self, batch, i):
        self.log.append(("valid", i))
        return i

    @contextlib.contextmanager
    def eval_weights(self):
        self.log.append("ema in")
        yield
        self.log.append("ema out")

    def validation_epoch_end(self, outs):
        self.log.append(("epoch_end", list(outs)))
        self.logged["val_MulticlassJaccardIndex"] = torch.tensor(next(self._mious, 0.5))

    def state_dict(self):
        return {"w": torch.zeros(2)}

    def on_save_checkpoint(self, ckpt):
        ckpt["ema_state_dict"] = {"w": torch.ones(2)}


class _Opt:
    def __init__(self, log, lr=0.1, weight_decay=0.0):
        self.log, self.param_groups = log, [{"lr": lr, "weight_decay": weight_decay}]

    def zero_grad(self):
        self.log.append("zero_grad")

    def step(self):
        self.log.append(("step", self.param_groups[0]["lr"]))


def _batches(n, size=4):
    return [{"image": torch.zeros(size, 1, 2, 2), "loss": 1.0 + k} for k in range(n)]


# ------------------------------------------------------------------------------------------------------- history_entry
def test_history_entry_has_the_first_four_keys_and_nothing_else_by_default():
    e = fit.history_entry(2, 0.75, 0.5, 40, 2.0)
    assert list(e) == FIRST and e == {"epoch": 2, "train_loss": 0.75, "val_MulticlassJaccardIndex": 0.5,
                                      "train_tiles_per_s": 20.0}
    assert fit.history_entry(0, 0.75, 0.5, 0, 2.0)["train_tiles_per_s"] is None          # the train loader yielded nothing
    assert fit.history_entry(0, 0.75, 0.5, 8, 0.0)["train_tiles_per_s"] is None


OPTIONAL = [("train_region", dict(train_region=0.25), ["train_region"]),
            ("lr", dict(lr=1e-3), ["lr"]),
            ("clip", dict(clip_state={"grad_norm": 3.5, "clipped_steps": 2, "max_norm": 1.0}), ["grad_norm", "clipped_steps"]),
            ("decay", dict(weight_decay=0.01, decayed_tensors=7), ["weight_decay", "decayed_tensors"]),
            ("plan", dict(plan={"policy": "balanced", "n_kept": 9}), ["plan"])]


@pytest.mark.parametrize("on", list(itertools.product([False, True], repeat=len(OPTIONAL))),
                         ids=lambda on: "".join("01"[f] for f in on))
def test_history_entry_adds_each_key_under_its_condition_in_the_documented_order(on):
    kw, want = {}, list(FIRST)
    for flag, (_, keywords, keys) in zip(on, OPTIONAL):
        if flag:
            kw.update(keywords)
            want += keys
    e = fit.history_entry(1, 0.5, 0.25, 8, 1.0, **kw)
    assert list(e) == want                                                                # these keys, this order, no others
    if on[2]:
        assert (e["grad_norm"], e["clipped_steps"]) == (3.5, 2) and "max_norm" not in e
    if on[4]:
        assert e["plan"] == kw["plan"] and e["plan"] is not kw["plan"]                    # a copy: the loader replans


# ------------------------------------------------------------------------------------------------------- checkpoints
def _reference_topk(ckpt_dir, k, metrics):
    """fit_model's keeper as it stood inside the loop: -> (files kept, best path)."""
    best = []
    for epoch, miou in enumerate(metrics):
        best.append((miou, os.path.join(ckpt_dir, f"model-epoch={epoch:02d}-val_MulticlassJaccardIndex={miou:.4f}.ckpt")))
        best.sort(key=lambda t: -t[0])
        best = best[:k]
    return sorted(os.path.basename(p) for _, p in best), (best[0][1] if best else "")


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("metrics", [[0.2, 0.6, 0.6, 0.4, 0.6, 0.1], [0.5, 0.5, 0.5, 0.5], [0.1, 0.2, 0.3, 0.4, 0.5],
                                     [0.9, 0.3]], ids=str)
def test_topk_keeps_the_files_it_kept_and_names_the_best(tmp_path, k, metrics):
    hyper = {"lr": 1e-3, "model": {"name": "ms_model"}}
    keeper = fit.TopKCheckpoints(str(tmp_path), k, hyper)
    assert keeper.best == "" and os.path.isdir(tmp_path / "checkpoints")
    model = _Model()
    for epoch, miou in enumerate(metrics):
        keeper.save(model, epoch, miou)
        assert len(os.listdir(tmp_path / "checkpoints")) == min(k, epoch + 1)            # pruned as it goes
    files, best = _reference_topk(str(tmp_path / "checkpoints"), k, metrics)
    assert sorted(os.listdir(tmp_path / "checkpoints")) == files and keeper.best == best
    first_best = metrics.index(max(metrics))                                             # a tie: the earlier epoch wins
    assert os.path.basename(best) == f"model-epoch={first_best:02d}-val_MulticlassJaccardIndex={max(metrics):.4f}.ckpt"
    ckpt = torch.load(best, map_location="cpu", weights_only=False)
    assert list(ckpt) == ["state_dict", "epoch", "hyper_parameters", "ema_state_dict"]   # the hook ran, after the three
    assert ckpt["epoch"] == first_best and ckpt["hyper_parameters"] == hyper and ckpt["hyper_parameters"] is not hyper
    assert torch.equal(ckpt["ema_state_dict"]["w"], torch.ones(2))


def test_topk_without_an_experiment_directory_writes_nothing(tmp_path):
    keeper = fit.TopKCheckpoints(None, 3, {})
    keeper.save(_Model(), 0, 0.5)
    assert keeper.best == "" and os.listdir(tmp_path) == []

    class _Plain(_Model):
        on_save_checkpoint = None                                                         # a model without the hook
    keeper = fit.TopKCheckpoints(str(tmp_path), 1, {})
    keeper.save(_Plain(), 0, 0.5)
    assert list(torch.load(keeper.best, weights_only=False)) == ["state_dict", "epoch", "hyper_parameters"]


# ------------------------------------------------------------------------------------------------------- train_epoch
def test_train_epoch_sets_the_schedules_lr_ahead_of_every_step_and_counts_across_epochs():
    cfg = {"lr": 0.1, "n_epochs": 2, "lr_schedule": "cosine", "warmup_steps": 2, "min_lr": 0.01}
    schedule = LrSchedule.from_cfg(cfg, 3)
    model = _Model()
    opt = _Opt(model.log)
    n_steps, seen = 0, []
    for epoch in range(2):
        del model.log[:]
        loss, n_tiles, seconds, n_steps = fit.train_epoch(model, opt, _batches(3), None, schedule, n_steps, "cpu")
        assert (loss.value, n_tiles, n_steps) == (3.0, 12, 3 * (epoch + 1)) and seconds > 0
        per_step = [model.log[k:k + 4] for k in range(0, len(model.log), 4)]
        assert [[s[0], s[1], s[2], s[3][0]] for s in per_step] == \
            [["zero_grad", ("train", i), "backward", "step"] for i in range(3)]           # Lightning's order, nothing else
        seen += [s[3][1] for s in per_step]
    want = [lr_at(n, 0.1, "cosine", 6, 2, 0.01) for n in range(1, 7)]
    assert seen == want and len(set(seen)) == 6 and model.global_step == 6               # 1-based, over both epochs
    assert opt.param_groups[0]["lr"] == want[-1]


def test_train_epoch_without_a_schedule_leaves_the_lr_and_respects_the_limit():
    model = _Model()
    opt = _Opt(model.log, lr=0.3)
    loss, n_tiles, _, n_steps = fit.train_epoch(model, opt, _batches(5, size=2), 2, None, 7, "cpu")
    assert (loss.value, n_tiles, n_steps) == (2.0, 4, 9)
    assert [e for e in model.log if isinstance(e, tuple) and e[0] == "step"] == [("step", 0.3)] * 2
    loss, n_tiles, _, n_steps = fit.train_epoch(model, opt, [], None, None, 9, "cpu")      # an empty loader
    assert (loss, n_tiles, n_steps) == (None, 0, 9)


def test_validate_runs_inside_the_ema_swap_and_returns_the_logged_metric():
    model = _Model(mious=[0.625])
    assert fit.validate(model, _batches(3), 2) == 0.625
    assert model.log == ["reset", "ema in", ("valid", 0), ("valid", 1), "ema out", ("epoch_end", [0, 1])]
    model.logged.clear()
    model.validation_epoch_end = lambda outs: None
    assert fit.validate(model, [], None) == 0.0                                           # nothing logged: zero, as before


# ------------------------------------------------------------------------------------------------------- LrSchedule
def test_lr_schedule_from_cfg_is_none_without_the_keys_and_caps_by_limit_train_batches():
    base = {"lr": 0.1, "n_epochs": 4, "limit_train_batches": None}
    assert LrSchedule.from_cfg(base, 10) is None
    for key, value in (("lr_schedule", "constant"), ("warmup_steps", 0), ("min_lr", 0.0)):      # any one key is a schedule
        s = LrSchedule.from_cfg({**base, key: value}, 10)
        assert s == LrSchedule("constant", 0.1, 0, 0.0, 40) and s.given == (key,)
    s = LrSchedule.from_cfg({**base, "lr_schedule": "poly", "warmup_steps": 3, "min_lr": 0.01, "limit_train_batches": 6}, 10)
    assert s == LrSchedule("poly", 0.1, 3, 0.01, 24)                                      # min(10, 6) x 4
    assert LrSchedule.from_cfg({**base, "lr_schedule": "linear", "limit_train_batches": 60}, 10).total_steps == 40
    assert [s.lr(n) for n in (1, 3, 4, 24, 30)] == [lr_at(n, 0.1, "poly", 24, 3, 0.01) for n in (1, 3, 4, 24, 30)]
    with pytest.raises(ValueError, match="min_lr 1.0 is above the learning rate 0.1"):
        LrSchedule.from_cfg({**base, "min_lr": 1.0}, 10)
    with pytest.raises(ValueError, match="unknown lr schedule"):
        LrSchedule.from_cfg({**base, "lr_schedule": "step"}, 10)


def test_lr_schedule_from_args_checks_and_records_what_was_stated():
    def args(*extra):
        return fit.build_parser().parse_args(["/data", "--exp_dir", "/exp", *extra])
    assert LrSchedule.from_args(args()) is None
    s = LrSchedule.from_args(args("--lr", "0.01", "--warmup_steps", "5"))
    assert s == LrSchedule("constant", 0.01, 5, 0.0, None) and s.given_cfg() == {"warmup_steps": 5}
    s = LrSchedule.from_args(args("--lr_schedule", "cosine", "--min_lr", "1e-6"))
    assert s.given_cfg() == {"lr_schedule": "cosine", "min_lr": 1e-6} and list(s.given_cfg()) == ["lr_schedule", "min_lr"]
    with pytest.raises(ValueError, match="min_lr 1.0 is above the learning rate 0.0001"):
        LrSchedule.from_args(args("--min_lr", "1"))
    with pytest.raises(ValueError, match="warmup_steps must be >= 0"):
        LrSchedule.from_args(args("--warmup_steps", "-1"))


# ------------------------------------------------------------------------------------------------------- fit_model
class _Loader(list):
    last_plan = {"policy": "labelled", "n_kept": 2}


def test_fit_model_over_stand_ins_builds_the_history_and_reads_the_device_once_per_epoch(tmp_path):
    model = _Model(mious=[0.5, 0.75, 0.75], region_weight=1.0, grad_clip_norm=1.0, weight_decay=0.01)
    cfg = {"lr": 0.1, "n_epochs": 3, "save_topk_models": 1, "lr_schedule": "linear", "limit_val_batches": 1}
    best = fit.fit_model(cfg, _Loader(_batches(2)), _batches(2), {"ms_image": 1}, exp_dir=str(tmp_path), device="cpu",
                         model=model)
    assert os.path.basename(best) == "model-epoch=01-val_MulticlassJaccardIndex=0.7500.ckpt"
    assert os.listdir(tmp_path / "checkpoints") == [os.path.basename(best)]
    assert fit.fit_model.last_model is model and model.current_epoch == 2 and model.global_step == 6
    want_keys = FIRST + ["train_region", "lr", "grad_norm", "clipped_steps", "weight_decay", "decayed_tensors", "plan"]
    assert [list(e) for e in model.history] == [want_keys] * 3
    assert [e["epoch"] for e in model.history] == [0, 1, 2]
    assert [e["val_MulticlassJaccardIndex"] for e in model.history] == [0.5, 0.75, 0.75]
    assert [e["lr"] for e in model.history] == [lr_at(n, 0.1, "linear", 6) for n in (2, 4, 6)]     # the last step's
    e = model.history[0]
    assert (e["train_loss"], e["train_region"], e["grad_norm"], e["clipped_steps"], e["weight_decay"], e["decayed_tensors"],
            e["plan"]) == (2.0, 0.25, 3.5, 2, 0.01, 3, _Loader.last_plan)
    # per epoch: the steps, then the two device reads, then validation -- and nothing reads the device inside the steps
    epoch0 = model.log[:model.log.index(("epoch_end", [0])) + 1]
    assert [x for x in epoch0 if isinstance(x, str) and x.startswith("read")] == ["read region", "read clip"]
    assert epoch0.index("read region") > max(i for i, x in enumerate(epoch0) if isinstance(x, tuple) and x[0] == "step")
    assert epoch0.index("read clip") < epoch0.index("reset")
    hyper = torch.load(best, weights_only=False)["hyper_parameters"]
    assert hyper == {**fit.DEFAULTS, **cfg} and list(hyper)[:len(fit.DEFAULTS)] == list(fit.DEFAULTS)


class _Unsized:
    """A train loader whose length must not be asked for: no schedule needs it."""

    def __iter__(self):
        return iter(_batches(1))

    def __len__(self):
        raise AssertionError("no schedule: the loader's length is not taken (a planning loader takes its census for it)")


def test_fit_model_plain_has_the_first_four_keys_only():
    model = _Model()
    assert fit.fit_model({"n_epochs": 2}, _Unsized(), [], {"ms_image": 1}, device="cpu", model=model) == ""
    assert [list(e) for e in model.history] == [FIRST] * 2
    assert not [x for x in model.log if isinstance(x, str) and x.startswith("read")]


# ------------------------------------------------------------------------------------------------------- main's summary
def test_run_summary_has_the_keys_main_printed():
    model = _Model()
    model.history = [{"epoch": 0}]
    base = ["checkpoint", "loader", "train_tiles", "valid_tiles", "history", "class_counts", "class_weights"]
    out = fit.run_summary({"lr": 0.1}, "scene", "/exp/x.ckpt", 12, 5, model, None)
    assert list(out) == base and out == {"checkpoint": "/exp/x.ckpt", "loader": "scene", "train_tiles": 12, "valid_tiles": 5,
                                         "history": [{"epoch": 0}], "class_counts": None, "class_weights": None}
    import json
    import numpy as np
    model.class_weights, model.weight_decay = (0.0, 0.75, 1.5), 0.01
    cfg = {"sampling": {"tile_sampling": "balanced"}, "augmentation": {"zoom": [0.75, 1.5]}}
    out = fit.run_summary(cfg, "tile", "", 12, 5, model, np.array([7, 2, 1], dtype=np.int64))
    assert list(out) == base + ["tile_sampling", "augmentation", "weight_decay", "decayed_tensors"]
    assert out["class_counts"] == [7, 2, 1] and out["class_weights"] == [0.0, 0.75, 1.5]
    assert out["tile_sampling"] == cfg["sampling"] and out["augmentation"] == cfg["augmentation"]
    assert (out["weight_decay"], out["decayed_tensors"]) == (0.01, 3)
    json.dumps(out)                                                                       # one JSON line: plain values only
