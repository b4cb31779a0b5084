"""GPU: content-aware tile sampling -- fu_label_box_counts against its numpy statement (exact integers), against the
existing fu_label_class_counts, its rejected calls; SceneTileLoader under tile_sampling / crop_jitter against the kernels
called directly on the boxes it reports (bit for bit); the fit command line end to end."""
import json
import os

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib, augment
from floodplanet_code_amd.datasets import FloodplanetTiles, SceneTileLoader, generate_image_slice_object, sampling
from floodplanet_code_amd.datasets.assemble import scene_crops, scene_train_tiles
from floodplanet_code_amd.datasets.class_weights import label_class_counts
from floodplanet_code_amd.datasets.sampling import label_box_counts, label_box_counts_host
from floodplanet_code_amd.unet import HipUNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUES = np.array([0, 1, 2, 3, 255], dtype=np.uint8)


def _net(th=32, tw=32):
    net = HipUNet(2, 3, base_channels=8).to(DEV).eval()
    net._get_ctx(torch.device(DEV), 1, th, tw)
    return net                                   # keep the module alive: it owns the context


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32),
                                                                      b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ kernel
def _rasters():
    """70 x 53 and 37 x 45: odd widths, so every row of a box starts at another alignment, and the whole 70 x 53 raster is
    more (row, chunk) pairs than the workgroup has threads; 1 x 1; 3 x 1030: rows of more 16-byte chunks than a wave has
    lanes, a width that is no multiple of 16; one raster of no data only and one of water only."""
    g = np.random.default_rng(0)
    out = [g.choice(VALUES, size=hw, p=[0.2, 0.4, 0.25, 0.1, 0.05]) for hw in ((70, 53), (37, 45), (1, 1), (3, 1030))]
    return out + [np.zeros((20, 33), dtype=np.uint8), np.full((20, 33), 2, dtype=np.uint8)]


def _table(rasters):
    """(raster index, box): per raster the whole raster, an unaligned interior box, the last pixel, one full row, one full
    column; on the first raster every w0 in 0..17 x every width in 1..35 (each head and tail of the 16-byte path)."""
    out = []
    for r, lab in enumerate(rasters):
        H, W = lab.shape
        out += [(r, (0, 0, H, W)), (r, (H - 1, W - 1, H, W)), (r, (H // 2, 0, H // 2 + 1, W)), (r, (0, W // 2, H, W // 2 + 1))]
        if H >= 29 and W >= 40:
            out.append((r, (5, 7, 29, 40)))
    out += [(0, (3 + (w0 + dw) % 5, w0, 8 + (w0 + dw) % 5, w0 + dw)) for w0 in range(18) for dw in range(1, 36)]
    return out


def _many(raster, n, seed):
    g = np.random.default_rng(seed)
    H, W = raster.shape
    h0, w0 = g.integers(0, H, n), g.integers(0, W, n)
    return [(int(a), int(b), int(g.integers(a + 1, H + 1)), int(g.integers(b + 1, W + 1))) for a, b in zip(h0, w0)]


@pytest.fixture(scope="module")
def census():
    """The tables, on the host and the device, and the host statement's answer to each (computed once)."""
    rasters = _rasters()
    dev = [torch.from_numpy(r).to(DEV) for r in rasters]
    tables = {"shapes": _table(rasters), "one": [(3, (0, 0, 3, 1030))],
              "many": [(1, b) for b in _many(rasters[1], 2051, 1)]}
    want = {k: label_box_counts_host([(rasters[r], b) for r, b in t]) for k, t in tables.items()}
    return rasters, dev, tables, want


@pytest.mark.parametrize("name", ["shapes", "one", "many"])
def test_kernel_equals_the_host_statement_exactly(census, name):
    rasters, dev, tables, want = census
    net = _net()
    table = tables[name]
    n = len(table)
    assert n == {"shapes": 4 * 6 + 2 + 18 * 35, "one": 1, "many": 2051}[name]
    out = torch.full((n + 2, 3), -7, dtype=torch.int64, device=DEV)          # two guard rows past n
    got = label_box_counts(net._ctx, [(dev[r], b) for r, b in table], counts=out)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got[:n], want[name])                       # rows < n fully overwritten (no -7 survives)
    assert (got[n:] == -7).all()
    areas = np.array([(b[2] - b[0]) * (b[3] - b[1]) for _, b in table])
    np.testing.assert_array_equal(got[:n].sum(1), areas)
    fresh = label_box_counts(net._ctx, [(dev[r], b) for r, b in table])      # and into a buffer of its own
    assert fresh.shape == (n, 3) and fresh.dtype == torch.int64
    np.testing.assert_array_equal(fresh.cpu().numpy(), want[name])


def test_column_sums_equal_the_class_count_kernel(census):
    rasters, dev, tables, want = census
    net = _net()
    entries = [(dev[r], b) for r, b in tables["shapes"]]
    cols = label_box_counts(net._ctx, entries).sum(0).cpu().numpy()
    for nodata in (0, 2):
        for n_classes in (2, 3):
            mapped = np.zeros(n_classes, dtype=np.int64)
            for col, d in enumerate((0, 1, nodata)):
                if 0 <= d < n_classes:
                    mapped[d] += cols[col]
            np.testing.assert_array_equal(mapped, label_class_counts(net._ctx, entries, nodata, n_classes).cpu().numpy())


def test_rejected_calls_leave_the_counts_untouched(census):
    """The bad tables of test_label_class_counts_rejected_calls_leave_the_counts_untouched (all but 'n_classes < 1': this
    call has no such argument)."""
    lib = _lib.load()
    net = _net()
    ctx = net._ctx
    label = census[1][0]                                                    # [70, 53]
    counts = torch.full((2, 3), -7, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def entry(h0=0, w0=0, hE=32, wE=32, lab=label, sh=70, sw=53):
        return _lib.FuSceneTrainEntry(None, None if lab is None else lab.data_ptr(), sh, sw, h0, w0, hE, wE, 0, 0.0)

    def call(entries, n_=None, out=counts, ctx_=ctx, null_table=False):
        table = (_lib.FuSceneTrainEntry * max(len(entries), 1))(*entries)
        return lib.fu_label_box_counts(ctx_, len(entries) if n_ is None else n_, None if null_table else table,
                                       _lib.ptr(out), stream)

    good = [entry(), entry(8, 8, 70, 53)]
    bad = {
        "n < 1": lambda: call(good, n_=0),
        "negative n": lambda: call(good, n_=-2),
        "NULL label": lambda: call([entry(), entry(lab=None)]),
        "empty box": lambda: call([entry(), entry(4, 4, 4, 20)]),
        "inverted box": lambda: call([entry(), entry(20, 4, 10, 20)]),
        "box outside the raster (right)": lambda: call([entry(), entry(0, 30, 32, 54)]),
        "box outside the raster (bottom)": lambda: call([entry(), entry(60, 0, 71, 32)]),
        "negative origin": lambda: call([entry(-1, 0, 31, 32), entry()]),
        "bad raster size": lambda: call([entry(), entry(sh=0)]),
        "NULL counts": lambda: call(good, out=None),
        "NULL context": lambda: call(good, ctx_=None),
        "NULL table": lambda: call(good, null_table=True),
    }
    for what, fn in bad.items():
        assert fn() == _lib.FU_ERR_INVALID, what
        assert b"fu_label_box_counts" in lib.fu_last_error(), what
    torch.cuda.synchronize()
    assert bool((counts == -7).all())
    assert call(good) == _lib.FU_OK                                         # the same table, valid, does run (and WRITES)
    torch.cuda.synchronize()
    host = census[0][0]
    np.testing.assert_array_equal(counts.cpu().numpy(), label_box_counts_host([(host, (0, 0, 32, 32)), (host, (8, 8, 70, 53))]))


# ------------------------------------------------------------------------------------------------------------ loader
def _rewritten_tree(root):
    """A tree of four 100 x 100 label rasters: RegA = one scene of no data only and one with a water blob in a corner on
    land; RegB = one scene of land and no data without water, and one as the generator draws it (0, 1, 2 everywhere)."""
    from tools.tiff_writer import make_floodplanet_tree, write_tiff
    made = make_floodplanet_tree(root, regions=("RegA", "RegB"), images_per_region=2, label_size=100, s1_size=40)
    g = np.random.default_rng(5)
    blob = np.ones((100, 100), dtype=np.uint8)
    blob[:30, :38] = 2
    blob[60:, 50:] = 0
    dry = g.integers(0, 2, (100, 100), dtype=np.uint8)
    new = {"RegA": [np.zeros((100, 100), dtype=np.uint8), blob], "RegB": [dry, None]}
    for (reg, name), rasters in sorted(made.items()):
        lab = new[reg].pop(0)
        if lab is not None:
            write_tiff(os.path.join(root, "CSDAP_complete", reg, "labels", name + ".tif"), lab, rows_per_strip=8)
    return root


@pytest.fixture(scope="module")
def rewritten(tmp_path_factory):
    return _rewritten_tree(str(tmp_path_factory.mktemp("rewritten")))


def _dataset(root, ignore_index, norm_mode=None):
    return FloodplanetTiles(root, "test", generate_image_slice_object(64, 64, 32), eval_region=["RegA", "RegB"], sensor="S1",
                            ignore_index=ignore_index, norm_mode=norm_mode)


def _host_stats(loader, boxes_of, ignore_index):
    """(trainable, water) per example by the host statement, from the loader's resident label rasters."""
    labels = {}
    entries = []
    for i, (_, label, _) in enumerate(loader._items):
        lab = labels.setdefault(label.data_ptr(), label.cpu().numpy())
        entries.append((lab, boxes_of[i]))
    return sampling.tile_stats(label_box_counts_host(entries), ignore_index, 3)


def test_labelled_loader_drops_dead_tiles_and_cuts_the_rest_unchanged(rewritten):
    ds = _dataset(rewritten, 0, "local")                                   # ignore_index 0: only water trains
    net = _net(64, 64)
    loader = SceneTileLoader(ds, 5, DEV, net, shuffle=True, transforms={}, seed=4, tile_sampling="labelled")
    n_batches = len(loader)
    grid = [it[2] for it in (loader._items or [])]
    trainable, _ = _host_stats(loader, grid, 0)
    kept = set(np.flatnonzero(trainable >= 1).tolist())
    assert 0 < len(kept) < len(ds)                                          # the tree has tiles to drop and tiles to keep
    orders = []
    for epoch in range(2):
        seen = []
        batches = list(loader)
        assert len(batches) == n_batches == (len(kept) + 4) // 5
        for batch in batches:
            entries = [loader._items[i][:2] + (box, int(f), float(a)) for i, box, f, a in
                       zip(batch["index"], batch["boxes"], batch["flags"], batch["angles"])]
            assert batch["boxes"] == [grid[i] for i in batch["index"]]     # no jitter: the grid's own boxes
            image, target, mean, std = scene_train_tiles(net._ctx, entries, (64, 64), "local", None, nodata_value=0,
                                                         target_fill=0)
            torch.cuda.synchronize()
            assert _bits_equal(batch["image"], image) and torch.equal(batch["target"], target)
            assert _bits_equal(batch["mean"], mean) and _bits_equal(batch["std"], std)
            seen += batch["index"]
        assert sorted(seen) == sorted(kept)                                 # every kept index once, no dropped one
        orders.append(seen)
    assert orders[0] != orders[1]
    plan = loader.last_plan
    assert (plan["policy"], plan["n_examples"], plan["n_kept"], plan["n_dropped"]) == ("labelled", len(ds), len(kept),
                                                                                     len(ds) - len(kept))


def test_balanced_loader_trains_the_planned_share_of_water_tiles(rewritten):
    ds = _dataset(rewritten, 2)                                            # ignore_index 2: land and water train
    net = _net(64, 64)
    loader = SceneTileLoader(ds, 5, DEV, net, shuffle=True, transforms={}, seed=4, ignore_index=2,
                             tile_sampling="balanced", water_share=0.75)
    index = [i for batch in loader for i in batch["index"]]
    plan = loader.last_plan
    grid = [it[2] for it in loader._items]
    trainable, water = _host_stats(loader, grid, 2)
    assert not plan["degraded"] and plan["n_kept"] == int((trainable >= 1).sum()) == len(index) < len(ds)
    n_water = sum(int(water[i] >= 1) for i in index)
    assert n_water == plan["n_water"] == round(0.75 * len(index)) and plan["water_share_planned"] == n_water / len(index)
    assert all(trainable[i] >= 1 for i in index)


def _host_target(loader, index, boxes, th, tw, nodata):
    out = np.full((len(index), th, tw), nodata, dtype=np.int64)
    for k, (i, (h0, w0, hE, wE)) in enumerate(zip(index, boxes)):
        raw = loader._items[i][1][h0:hE, w0:wE].cpu().numpy()
        dec = np.zeros(raw.shape, dtype=np.int64)
        dec[raw == 2] = 1
        dec[raw == 0] = nodata
        out[k, :hE - h0, :wE - w0] = dec
    return torch.from_numpy(out)


def test_jittered_batches_are_the_chain_on_the_boxes_they_report(rewritten):
    ds = _dataset(rewritten, 2, "local")
    net = _net(64, 64)
    loader = SceneTileLoader(ds, 6, DEV, net, shuffle=True, transforms={}, seed=1, ignore_index=2,
                             tile_sampling="labelled", crop_jitter=8)
    grid = None
    per_epoch = []
    for epoch in range(2):
        boxes_of = {}
        for batch in loader:
            grid = grid or [it[2] for it in loader._items]
            image, mean, std = scene_crops(net._ctx, [(loader._items[i][0], box) for i, box in
                                                      zip(batch["index"], batch["boxes"])], (64, 64), "local")
            target = _host_target(loader, batch["index"], batch["boxes"], 64, 64, 2).to(DEV)
            image, target = augment.apply(image, target, batch["flags"], batch["angles"], target_fill=2)
            torch.cuda.synchronize()
            assert _bits_equal(batch["image"], image) and torch.equal(batch["target"], target)
            assert _bits_equal(batch["mean"], mean) and _bits_equal(batch["std"], std)
            for i, box in zip(batch["index"], batch["boxes"]):
                g = grid[i]
                H, W = loader._items[i][1].shape
                assert (box[2] - box[0], box[3] - box[1]) == (g[2] - g[0], g[3] - g[1])
                assert abs(box[0] - g[0]) <= 8 and abs(box[1] - g[1]) <= 8 and 0 <= box[0] and box[2] <= H and box[3] <= W
                boxes_of[i] = box
        # the census was taken on the jittered boxes: what was kept is what has trainable pixels THERE
        full = sampling.jitter_boxes(grid, [tuple(it[1].shape) for it in loader._items], 8, 1, epoch)
        trainable, _ = _host_stats(loader, full, 2)
        assert sorted(boxes_of) == np.flatnonzero(trainable >= 1).tolist()
        assert all(full[i] == b for i, b in boxes_of.items())
        per_epoch.append(boxes_of)
    assert any(per_epoch[0][i] != per_epoch[1].get(i) for i in per_epoch[0])          # fresh offsets every epoch
    assert any(b != grid[i] for i, b in per_epoch[0].items())


def test_census_runs_once_without_jitter_and_the_second_epoch_keeps_nothing(rewritten, monkeypatch):
    ds = _dataset(rewritten, 2)
    net = _net(64, 64)
    calls = []
    real = sampling.label_box_counts

    def counting(ctx, entries, *a, **k):
        calls.append(len(entries))
        return real(ctx, entries, *a, **k)
    monkeypatch.setattr(sampling, "label_box_counts", counting)
    loader = SceneTileLoader(ds, 5, DEV, net, shuffle=True, transforms={}, seed=0, ignore_index=2,
                             tile_sampling="balanced")
    for batch in loader:
        pass
    del batch
    torch.cuda.synchronize()
    assert calls == [len(ds)]                                               # one launch over the whole split
    base = torch.cuda.memory_allocated()
    for batch in loader:
        pass
    del batch
    torch.cuda.synchronize()
    assert calls == [len(ds)] and torch.cuda.memory_allocated() <= base
    # with jitter the boxes change, so every epoch counts again
    jittered = SceneTileLoader(ds, 5, DEV, net, shuffle=True, transforms={}, seed=0, ignore_index=2,
                               tile_sampling="balanced", crop_jitter=3)
    del calls[:]
    for _ in range(2):
        for batch in jittered:
            pass
    assert calls == [len(ds), len(ds)]


def test_default_loader_batches_carry_no_boxes_and_run_no_census(rewritten, monkeypatch):
    def no_census(*a, **k):
        raise AssertionError("the defaults take no census")
    monkeypatch.setattr(sampling, "label_box_counts", no_census)
    loader = SceneTileLoader(_dataset(rewritten, 0), 5, DEV, _net(64, 64), shuffle=True, transforms={}, seed=0)
    keys = {k for batch in loader for k in batch}
    assert keys == {"image", "target", "mean", "std", "index", "flags", "angles"} and loader.last_plan is None


# ------------------------------------------------------------------------------------------------------------ end to end
def _fit_args(root, exp, extra=()):
    return [root, "--exp_dir", exp, "--sensor", "S1", "--eval_region", "RegB", "--crop", "64", "64", "--stride", "32",
            "--batch_size", "4", "--n_epochs", "2", "--lr", "2e-3", "--base_channels", "8", "--loader", "scene",
            "--n_workers", "0", "--seed", "0", "--save_topk_models", "1", "--device", DEV, *extra]


def test_fit_cli_balanced_and_jittered(rewritten, tmp_path, capsys):
    from floodplanet_code_amd import fit, predict
    out = fit.main(_fit_args(rewritten, str(tmp_path / "exp"), ("--ignore_index", "2", "--tile_sampling", "balanced",
                                                                "--crop_jitter", "8", "--water_share", "0.5")))
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = {"tile_sampling": "balanced", "crop_jitter": 8, "water_share": 0.5}
    assert line["tile_sampling"] == want == out["tile_sampling"] and len(out["history"]) == 2
    for h in out["history"]:
        assert np.isfinite(h["train_loss"]) and 0.0 <= h["val_MulticlassJaccardIndex"] <= 1.0
        plan = h["plan"]
        assert plan["policy"] == "balanced" and not plan["degraded"] and 0 < plan["n_kept"] < plan["n_examples"]
        assert plan["n_water"] == round(0.5 * plan["n_kept"])
    ckpt = out["checkpoint"]
    hyper = torch.load(ckpt, map_location="cpu", weights_only=False)["hyper_parameters"]
    assert hyper["sampling"] == want and hyper["ignore_index"] == 2
    predict.main([ckpt, "--data_root", rewritten, "--batch_size", "4"])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert os.path.exists(os.path.join(res["pred_dir"], "metrics.json"))


def test_fit_cli_labelled_with_nothing_to_drop_trains_to_the_same_bits(tmp_path, capsys):
    """The stock synthetic tree: labels 0, 1, 2 everywhere, so under ignore_index 0 every tile has a trainable pixel and
    'labelled' plans plan_epoch's own order -- the same batches, the same draws, the same weights."""
    from tools.tiff_writer import make_floodplanet_tree
    from floodplanet_code_amd import fit
    root = str(tmp_path / "tree")
    make_floodplanet_tree(root, regions=("RegA", "RegB"), images_per_region=2, label_size=100, s1_size=40)
    states = {}
    for name, extra in (("plain", ()), ("labelled", ("--tile_sampling", "labelled"))):
        out = fit.main(_fit_args(root, str(tmp_path / name), extra))
        states[name] = (torch.load(out["checkpoint"], map_location="cpu", weights_only=False)["state_dict"], out)
    capsys.readouterr()
    plan = states["labelled"][1]["history"][-1]["plan"]
    assert plan["n_dropped"] == 0 and plan["n_kept"] == states["labelled"][1]["train_tiles"]
    assert "plan" not in states["plain"][1]["history"][-1] and "tile_sampling" not in states["plain"][1]
    a, b = states["plain"][0], states["labelled"][0]
    assert a.keys() == b.keys() and len(a) > 0
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
