"""CPU: the host side of content-aware tile sampling and crop jitter -- the C ABI declaration of fu_label_box_counts, its
numpy statement, the tile statistics, the epoch planner under the three policies, the jitter stream and the fit command line.
No device call anywhere."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from floodplanet_code_amd import _lib, augment, fit
from floodplanet_code_amd.datasets import FloodplanetTiles, SceneTileLoader, generate_image_slice_object
from floodplanet_code_amd.datasets import sampling
from floodplanet_code_amd.datasets.class_weights import label_class_counts_host
from floodplanet_code_amd.datasets.sampling import jitter_boxes, label_box_counts_host, plan_order, tile_stats
from floodplanet_code_amd.datasets.scene_loader import epoch_order, order_batches, plan_epoch

HEADER = os.path.join(ROOT, "include", "floodunet.h")


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_label_box_counts_and_lib_binds_it():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(fu_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}
    assert int(re.search(r"#define\s+FU_ABI_VERSION\s+(\d+)", txt).group(1)) == 5      # additive: no version bump
    assert "fu_label_box_counts" in decl and len(decl["fu_label_box_counts"].split(",")) == 5
    res, args = _lib.SIGNATURES["fu_label_box_counts"]
    assert res is _lib._i and len(args) == 5 and args[2] == ctypes.POINTER(_lib.FuSceneTrainEntry)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "fu_label_box_counts")
    assert _lib.load().fu_abi_version() == 5


def test_null_context_is_rejected_with_a_message():
    lib = _lib.load()
    table = (_lib.FuSceneTrainEntry * 1)()
    assert lib.fu_label_box_counts(None, 1, table, None, None) == _lib.FU_ERR_INVALID
    assert b"fu_label_box_counts" in lib.fu_last_error()


# ------------------------------------------------------------------------------------------------------------ host census
def _rasters(seed=0):
    g = np.random.default_rng(seed)
    vals = np.array([0, 1, 2, 3, 255], dtype=np.uint8)
    return [g.choice(vals, size=hw, p=[0.3, 0.3, 0.2, 0.1, 0.1]) for hw in ((13, 9), (7, 20), (1, 1))]


def _entries(rasters):
    out = []
    for lab in rasters:
        H, W = lab.shape
        out += [(lab, (0, 0, H, W)), (lab, (H - 1, W - 1, H, W)), (lab, (H // 2, 0, H // 2 + 1, W)),
                (lab, (0, W // 2, H, W // 2 + 1))]
        if H > 6 and W > 8:
            out.append((lab, (2, 3, 6, 8)))
    return out


def test_host_census_equals_a_per_pixel_loop():
    entries = _entries(_rasters())
    got = label_box_counts_host(entries)
    assert got.dtype == np.int64 and got.shape == (len(entries), 3)
    for row, (lab, (h0, w0, hE, wE)) in zip(got, entries):
        want = [0, 0, 0]
        for y in range(h0, hE):
            for x in range(w0, wE):
                v = int(lab[y, x])
                want[1 if v == 2 else (2 if v == 0 else 0)] += 1
        assert row.tolist() == want
        assert int(row.sum()) == (hE - h0) * (wE - w0)
    assert (got.sum(0) > 0).all()                                           # every column is exercised


@pytest.mark.parametrize("nodata", [0, 2])
@pytest.mark.parametrize("n_classes", [2, 3])
def test_host_census_columns_map_to_the_class_counts(nodata, n_classes):
    entries = _entries(_rasters(1))
    cols = label_box_counts_host(entries).sum(0)
    want = np.zeros(n_classes, dtype=np.int64)
    for col, d in enumerate((0, 1, nodata)):
        if 0 <= d < n_classes:
            want[d] += cols[col]
    np.testing.assert_array_equal(want, label_class_counts_host(entries, nodata, n_classes))


def test_host_census_rejects_bad_entries():
    lab = _rasters()[0]
    for bad in ([], [(None, (0, 0, 1, 1))], [(lab.astype(np.int32), (0, 0, 1, 1))], [(lab, (0, 0, 14, 9))],
                [(lab, (3, 3, 3, 5))], [(lab, (-1, 0, 4, 4))]):
        with pytest.raises(ValueError, match="label_box_counts"):
            label_box_counts_host(bad)


# ------------------------------------------------------------------------------------------------------------ tile_stats
def test_tile_stats_hand_written():
    counts = np.array([[10, 3, 7], [0, 0, 20], [5, 0, 0], [0, 4, 0]], dtype=np.int64)     # (other, water, no data)
    # ignore_index 0: no data and class 0 are both ignored -- only water trains
    t, w = tile_stats(counts, 0, 3)
    assert t.tolist() == [3, 0, 0, 4] and w.tolist() == [3, 0, 0, 4]
    # ignore_index 2 (and -1 = the last of 3 classes): no data -> 2 is ignored; classes 0 and 1 train
    for ii in (2, -1):
        t, w = tile_stats(counts, ii, 3)
        assert t.tolist() == [13, 0, 5, 4] and w.tolist() == [3, 0, 0, 4]
    # -1 with two classes: class 1, water, is the ignored one
    t, w = tile_stats(counts, -1, 2)
    assert t.tolist() == [10, 0, 5, 0] and w.tolist() == [0, 0, 0, 0]
    # None ignores nothing, but no data decodes to no class at all
    t, w = tile_stats(counts, None, 3)
    assert t.tolist() == [13, 0, 5, 4] and w.tolist() == [3, 0, 0, 4]
    assert t.dtype == np.int64 and w.dtype == np.int64
    with pytest.raises(ValueError):
        tile_stats(counts[:, :2], 0, 3)


# ------------------------------------------------------------------------------------------------------------ plan_order
KW = dict(shuffle=True, seed=3, epoch=1)


def test_plan_all_is_epoch_order():
    for shuffle in (False, True):
        order, info = plan_order(17, 64, "all", shuffle=shuffle, seed=5, epoch=2)
        assert order == epoch_order(17, shuffle, 5, 2)
        assert info["policy"] == "all" and info["n_kept"] == 17 and info["n_dropped"] == 0 and not info["degraded"]
    with pytest.raises(ValueError, match="tile_sampling"):
        plan_order(17, 64, "some", **KW)


@pytest.mark.parametrize("seed,epoch", [(0, 0), (7, 3)])
@pytest.mark.parametrize("batch_size,drop_last", [(1, False), (4, True), (5, False)])
@pytest.mark.parametrize("shard", [None, (0, 2), (2, 3)])
@pytest.mark.parametrize("shuffle", [False, True])
def test_labelled_with_nothing_to_drop_is_plan_epoch(seed, epoch, batch_size, drop_last, shard, shuffle):
    n = 23
    stats = (np.arange(1, n + 1), np.zeros(n, dtype=np.int64))
    order, info = plan_order(stats, 100, "labelled", shuffle=shuffle, seed=seed, epoch=epoch)
    assert info["n_dropped"] == 0 and info["n_kept"] == n
    assert order_batches(order, batch_size, drop_last, shard) == plan_epoch(n, batch_size, epoch, shuffle, seed, drop_last, shard)


def test_labelled_drops_and_keeps_exactly():
    trainable = np.array([0, 5, 0, 100, 49, 50, 0, 1])
    water = np.array([0, 5, 0, 0, 2, 0, 0, 1])
    order, info = plan_order((trainable, water), 100, "labelled", **KW)
    assert sorted(order) == [1, 3, 4, 5, 7]                                 # each kept index once, no dropped one
    assert (info["n_examples"], info["n_kept"], info["n_dropped"], info["n_water"]) == (8, 5, 3, 3)
    assert order == [[1, 3, 4, 5, 7][j] for j in epoch_order(5, True, 3, 1)]
    order, info = plan_order((trainable, water), 100, "labelled", min_trainable_frac=0.5, **KW)
    assert sorted(order) == [3, 5] and info["n_dropped"] == 6
    order, _ = plan_order((trainable, water), 100, "labelled", shuffle=False, seed=3, epoch=1)
    assert order == [1, 3, 4, 5, 7]


def _strata(n=40, n_water=7, n_dead=6, seed=0):
    g = np.random.default_rng(seed)
    trainable = np.full(n, 50)
    water = np.zeros(n, dtype=np.int64)
    idx = g.permutation(n)
    water[idx[:n_water]] = g.integers(1, 20, n_water)
    trainable[idx[n_water:n_water + n_dead]] = 0
    return (trainable, water), set(idx[:n_water].tolist()), set(idx[n_water:n_water + n_dead].tolist())


@pytest.mark.parametrize("share", [0.5, 0.25, 0.9, 0.0, 1.0])
@pytest.mark.parametrize("shuffle", [False, True])
def test_balanced_share_and_multiplicities(share, shuffle):
    stats, W, dead = _strata()
    L = 40 - len(dead)
    order, info = plan_order(stats, 100, "balanced", water_share=share, shuffle=shuffle, seed=1, epoch=0)
    assert len(order) == L == info["n_kept"] and not set(order) & dead and not info["degraded"]
    n_w = sum(i in W for i in order)
    assert n_w == round(share * L) == info["n_water"] and info["water_share_planned"] == n_w / L
    mult = collections.Counter(order)
    for stratum, k in ((W, n_w), (set(range(40)) - W - dead, L - n_w)):
        m = [mult.get(i, 0) for i in stratum]
        assert max(m) - min(m) <= 1 and sum(m) == k
    if not shuffle:
        assert order[:n_w] == sorted(order[:n_w]) and order[n_w:] == sorted(order[n_w:])
        assert all(i in W for i in order[:n_w])


def test_balanced_is_deterministic_and_differs_between_epochs():
    stats, _, _ = _strata()
    a, _ = plan_order(stats, 100, "balanced", shuffle=True, seed=1, epoch=0)
    b, _ = plan_order(stats, 100, "balanced", shuffle=True, seed=1, epoch=0)
    c, _ = plan_order(stats, 100, "balanced", shuffle=True, seed=1, epoch=1)
    d, _ = plan_order(stats, 100, "balanced", shuffle=True, seed=2, epoch=0)
    assert a == b and a != c and a != d
    # min_water_frac moves tiles from the water stratum to the dry one
    _, lo = plan_order(stats, 100, "balanced", min_water_frac=0.0, water_share=1.0, shuffle=True, seed=1, epoch=0)
    order, hi = plan_order(stats, 100, "balanced", min_water_frac=0.1, water_share=1.0, shuffle=True, seed=1, epoch=0)
    assert all(stats[1][i] >= 10 for i in order) and lo["n_water"] == hi["n_water"] == len(order)


def test_balanced_degrades_to_labelled_when_a_stratum_is_empty():
    trainable = np.array([4, 0, 9, 9, 2])
    for water in (np.zeros(5, dtype=np.int64), np.array([1, 0, 3, 2, 2])):       # no water tile; no dry tile
        order, info = plan_order((trainable, water), 9, "balanced", **KW)
        want, _ = plan_order((trainable, water), 9, "labelled", **KW)
        assert order == want and info["degraded"] and info["policy"] == "balanced" and info["n_kept"] == 4


def test_nothing_kept_raises_and_names_the_thresholds():
    stats = (np.array([0, 3, 0]), np.array([0, 3, 0]))
    for policy in ("labelled", "balanced"):
        with pytest.raises(ValueError, match="min_trainable_frac = 0.5"):
            plan_order(stats, 100, policy, min_trainable_frac=0.5, **KW)
    with pytest.raises(ValueError, match="min_trainable_frac"):
        plan_order((np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)), 100, "labelled", **KW)
    with pytest.raises(ValueError, match="water_share"):
        plan_order(stats, 100, "balanced", water_share=1.5, **KW)


@pytest.mark.parametrize("policy", ["labelled", "balanced"])
@pytest.mark.parametrize("world", [2, 3])
def test_planned_order_shards_equally_and_disjointly(policy, world):
    stats, _, _ = _strata()
    order, _ = plan_order(stats, 100, policy, shuffle=True, seed=4, epoch=2)
    shares = [order_batches(order, 4, False, (r, world)) for r in range(world)]
    assert len({len(s) for s in shares}) == 1
    flat = [[i for b in s for i in b] for s in shares]
    assert all(len(f) == len(order) // world for f in flat)
    for r, f in enumerate(flat):                                            # rank r takes positions r, r + world, ...
        assert f == order[r::world][:len(order) // world]


# ------------------------------------------------------------------------------------------------------------ jitter
def _grid_boxes():
    boxes, hw = [], []
    for H, W in ((100, 100), (70, 53)):
        for h0 in range(0, H, 32):
            for w0 in range(0, W, 32):
                boxes.append((h0, w0, min(h0 + 64, H), min(w0 + 64, W)))
                hw.append((H, W))
    return boxes, hw


@pytest.mark.parametrize("J", [1, 8, 200])
def test_jitter_keeps_size_bounds_and_range(J):
    boxes, hw = _grid_boxes()
    out = jitter_boxes(boxes, hw, J, seed=3, epoch=0)
    moved = 0
    for (h0, w0, hE, wE), (a0, b0, aE, bE), (H, W) in zip(boxes, out, hw):
        assert (aE - a0, bE - b0) == (hE - h0, wE - w0)
        assert 0 <= a0 and aE <= H and 0 <= b0 and bE <= W
        assert abs(a0 - h0) <= J and abs(b0 - w0) <= J
        moved += (a0, b0) != (h0, w0)
    assert moved > 0
    assert out == jitter_boxes(boxes, hw, J, seed=3, epoch=0)
    assert out != jitter_boxes(boxes, hw, J, seed=3, epoch=1) and out != jitter_boxes(boxes, hw, J, seed=4, epoch=0)


def test_jitter_zero_is_the_identity_and_draws_nothing(monkeypatch):
    boxes, hw = _grid_boxes()

    def no_draw(*a, **k):
        raise AssertionError("J = 0 must not draw")
    monkeypatch.setattr(np.random, "RandomState", no_draw)
    assert jitter_boxes(boxes, hw, 0, seed=3, epoch=5) == boxes
    with pytest.raises(ValueError, match="crop_jitter"):
        jitter_boxes(boxes, hw, -1, seed=3, epoch=5)


def test_jitter_offsets_cover_the_whole_range():
    boxes, hw = [(40, 40, 50, 50)] * 400, [(100, 100)] * 400
    out = jitter_boxes(boxes, hw, 2, seed=0, epoch=0)
    assert {b[0] - 40 for b in out} == {-2, -1, 0, 1, 2} == {b[1] - 40 for b in out}


# ------------------------------------------------------------------------------------------------------------ loader
@pytest.fixture()
def tiles(tmp_path):
    from tools.tiff_writer import make_floodplanet_tree
    make_floodplanet_tree(str(tmp_path), regions=("RegA",), images_per_region=2, label_size=90, s1_size=37)
    return FloodplanetTiles(str(tmp_path), "test", generate_image_slice_object(32, 32, 24), eval_region=["RegA"],
                            sensor="S1", ignore_index=0)


_SAMPLE_TRANSFORMS = augment.sample_transforms


class _FakeNet:
    def _get_ctx(self, *a):
        return object()


def _mocked_loader(tiles, monkeypatch, draws, **kw):
    """A SceneTileLoader whose device calls are replaced: resident 'rasters' on the host, no kernel."""
    from floodplanet_code_amd.datasets import assemble
    loader = SceneTileLoader(tiles, 5, "cuda:0", net=_FakeNet(), transforms={}, seed=9, max_resident_bytes=1 << 40, **kw)
    rng = np.random.default_rng(0)
    labels = {}
    items = []
    for ex in tiles.dataset:
        cp = ex["crop_params"]
        H, W = cp.og_height, cp.og_width
        lab = labels.setdefault(ex["image_path"], torch.from_numpy(rng.integers(0, 3, (H, W), dtype=np.uint8)))
        items.append((None, lab, (cp.h0, cp.w0, min(cp.hE, H), min(cp.wE, W))))
    loader._items = items
    def recording(n, cfg, rs):
        flags, angles = _SAMPLE_TRANSFORMS(n, cfg, rs)
        draws.append((flags.tolist(), angles.tolist()))
        return flags, angles
    monkeypatch.setattr(augment, "sample_transforms", recording)
    monkeypatch.setattr(assemble, "scene_train_tiles", lambda ctx, entries, *a, **k: (entries, None, None, None))
    monkeypatch.setattr(sampling, "label_box_counts",
                        lambda ctx, entries: torch.from_numpy(label_box_counts_host([(l.numpy(), b) for l, b in entries])))
    return loader


def test_transforms_stream_does_not_depend_on_the_jitter(tiles, monkeypatch):
    runs = {}
    for J in (0, 8):
        draws = []
        loader = _mocked_loader(tiles, monkeypatch, draws, shuffle=True, crop_jitter=J)
        batches = [b for _ in range(2) for b in loader]
        runs[J] = (draws, [b["index"] for b in batches], batches)
    assert runs[0][0] == runs[8][0] and len(runs[0][0]) == 2 * len(loader)       # the same draws, in the same order
    assert runs[0][1] == runs[8][1]                                              # and the same order of examples
    assert all("boxes" not in b for b in runs[0][2])                             # defaults: today's batch keys
    grid = [it[2] for it in loader._items]
    moved = 0
    for b in runs[8][2]:
        assert [e[2] for e in b["image"]] == b["boxes"]                          # the boxes cut are the boxes reported
        moved += sum(box != grid[i] for i, box in zip(b["index"], b["boxes"]))
    assert moved > 0


def test_loader_plans_lazily_and_caches_the_census(tiles, monkeypatch):
    draws = []
    loader = _mocked_loader(tiles, monkeypatch, draws, shuffle=True, tile_sampling="balanced", water_share=0.5)
    calls = []
    fake = sampling.label_box_counts
    monkeypatch.setattr(sampling, "label_box_counts", lambda ctx, entries: calls.append(len(entries)) or fake(ctx, entries))
    n = len(loader)                                                              # takes the census
    assert calls == [len(tiles)] and n == (loader.last_plan["n_kept"] + 4) // 5
    seen = [len([b for b in loader]) for _ in range(2)]
    assert seen == [n, n] and calls == [len(tiles)]                              # no second census without jitter
    assert loader.last_plan["policy"] == "balanced" and loader.last_plan["n_examples"] == len(tiles)
    for bad in (dict(tile_sampling="some"), dict(water_share=1.5), dict(min_trainable_frac=-0.1), dict(crop_jitter=-1)):
        with pytest.raises(ValueError):
            SceneTileLoader(tiles, 5, "cuda:0", net=None, max_resident_bytes=1 << 40, **bad)


# ------------------------------------------------------------------------------------------------------------ CLI
BASE = ["/data", "--exp_dir", "/exp"]


@pytest.mark.parametrize("extra", [
    ["--loader", "tile", "--tile_sampling", "labelled"],
    ["--loader", "tile", "--crop_jitter", "4"],
    ["--loader", "tile", "--water_share", "0.3"],
    ["--tile_sampling", "balanced", "--water_share", "1.5"],
    ["--tile_sampling", "labelled", "--min_trainable_frac", "-0.1"],
    ["--tile_sampling", "balanced", "--min_water_frac", "2"],
    ["--crop_jitter", "-1"],
    ["--tile_sampling", "most"],
])
def test_bad_sampling_options_are_parser_errors_before_any_device_work(extra, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the options are checked before any data set or device work")
    monkeypatch.setattr(fit, "build_model", no_device)
    monkeypatch.setattr(FloodplanetTiles, "__init__", no_device)
    with pytest.raises(SystemExit) as e:
        fit.main(BASE + extra)
    assert e.value.code == 2


def test_plain_command_line_gives_the_config_it_always_gave():
    args = fit.build_parser().parse_args(BASE)
    old = {k: v for k, v in vars(args).items() if k not in fit.SAMPLING_OPTIONS}     # a namespace from before the options
    assert len(old) == len(vars(args)) - 5
    cfg = fit.cfg_from_args(args)
    assert cfg == fit.cfg_from_args(type("Namespace", (), old)()) and "sampling" not in cfg
    given = fit.cfg_from_args(fit.build_parser().parse_args(BASE + ["--tile_sampling", "balanced", "--crop_jitter", "8"]))
    assert given.pop("sampling") == {"tile_sampling": "balanced", "crop_jitter": 8} and given == cfg
    one = fit.cfg_from_args(fit.build_parser().parse_args(BASE + ["--min_water_frac", "0.25"]))
    assert one["sampling"] == {"min_water_frac": 0.25}
