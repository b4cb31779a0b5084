"""CPU: fit.cfg_from_args, pinned.  tests/golden/fit_config_pin.json holds, for a matrix of command lines (plain, each option
family alone, everything compatible at once), the config that cfg_from_args returned at the commit before the options values
took the command line over (TileOptions, LossOptions.from_args, LrSchedule): the dict goes into every checkpoint's
hyper_parameters, so its keys, their order, the values and their types are all part of the contract."""
import json
import os

import pytest

from conftest import GOLDEN
from floodplanet_code_amd import fit

BASE = ["/data", "--exp_dir", "/exp"]
with open(os.path.join(GOLDEN, "fit_config_pin.json")) as f:
    CASES = json.load(f)


def test_the_matrix_covers_every_option_family():
    flags = {a for c in CASES for a in c["argv"] if a.startswith("--")}
    parser_flags = {s for a in fit.build_parser()._actions for s in a.option_strings if s.startswith("--")}
    assert parser_flags - flags <= {"--help", "--exp_dir", "--channels", "--train_split_pct", "--ignore_index",
                                    "--no_transforms", "--no_shuffle", "--device"}      # (none of them shapes an options value)
    assert CASES[0]["argv"] == [] and len({c["name"] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cfg_from_args_gives_the_config_it_gave(case):
    cfg = fit.cfg_from_args(fit.build_parser().parse_args(BASE + case["argv"]))
    assert cfg == case["cfg"]                                    # (a list is no tuple, so the containers are pinned too)
    assert json.dumps(cfg) == json.dumps(case["cfg"])            # byte for byte: key order, 8 against 8.0
    assert json.loads(json.dumps(cfg)) == cfg


def test_resolved_class_weights_sit_where_the_command_line_puts_them():
    """What main() does for --class_weights balanced: the same config as stating the numbers, in the same order."""
    rest = ["--focal_gamma", "2", "--region_loss", "dice", "--ema_decay", "0.9", "--weight_decay", "0.1"]
    stated = fit.cfg_from_args(fit.build_parser().parse_args(BASE + ["--class_weights", "0", "0.75", "1.5"] + rest))
    args = fit.build_parser().parse_args(BASE + ["--class_weights", "balanced"] + rest)
    assert json.dumps(fit.cfg_from_args(args, class_weights=[0, 0.75, 1.5])) == json.dumps(stated)
    later = fit.cfg_from_args(args)
    assert "class_weights" not in later["model"]["model_kwargs"]
    fit.set_class_weights(later, (0, 0.75, 1.5))
    assert json.dumps(later) == json.dumps(stated)
    fit.set_class_weights(later, [3, 2, 1])                      # set again: replaced in place
    assert list(later["model"]["model_kwargs"]) == list(stated["model"]["model_kwargs"])
    assert later["model"]["model_kwargs"]["class_weights"] == [3.0, 2.0, 1.0]
