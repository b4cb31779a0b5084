"""GPU: label-free scene inference -- fu_scene_crops against cut-then-fu_assemble_tiles (bit for bit) and its rejected
calls, the whole-scene resample against the host restatement, resident-grid crops against TileLoader's device path,
infer() against predict() (bit for bit) and against the oracle network, and the bound on resident scenes."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd import infer as I
from floodplanet_code_amd.datasets.assemble import assemble_tiles, scene_crops
from floodplanet_code_amd.datasets.resize import resize_lanczos4
from floodplanet_code_amd.datasets.tiff import read_tiff
from floodplanet_code_amd.unet import HipUNet
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
sys.path.insert(0, os.path.dirname(__file__))


def _bits_equal(a, b):
    """Bit for bit, NaN included (a 1 x 1 box has std 0 under 'local': 0 / 0 on both sides)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32),
                                                                      b.contiguous().view(torch.int32))


def _ctx():
    net = HipUNet(2, 3, base_channels=8).to(DEV).eval()
    net._get_ctx(torch.device(DEV), 1, 32, 32)
    return net                                   # keep the module alive: it owns the context


def _scenes(C, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(C, h, w, generator=g) * 5 - 1).to(DEV) for h, w in ((70, 53), (40, 90), (25, 25))]


# (scene, h0, w0, hE, wE): full boxes, partial edge boxes, a box that is the whole (small) scene, scenes interleaved
BOXES = [(0, 0, 0, 32, 32), (1, 8, 58, 40, 90), (0, 64, 40, 70, 53), (2, 0, 0, 25, 25), (1, 0, 0, 32, 32),
         (0, 32, 21, 64, 53), (2, 10, 3, 25, 20), (1, 39, 0, 40, 1)]


def _reference(scenes, boxes, C, norm_mode, gp):
    raw = torch.zeros(len(boxes), C, 32, 32, device=DEV)
    for i, (s, h0, w0, hE, wE) in enumerate(boxes):
        raw[i, :, :hE - h0, :wE - w0] = scenes[s][:, h0:hE, w0:wE]
    vh = torch.tensor([b[3] - b[1] for b in boxes], dtype=torch.int32, device=DEV)
    vw = torch.tensor([b[4] - b[2] for b in boxes], dtype=torch.int32, device=DEV)
    return assemble_tiles([raw], norm_mode, (vh, vw), gp)


@pytest.mark.parametrize("norm_mode", [None, "local", "global"])
@pytest.mark.parametrize("C", [2, 4, 7])
def test_scene_crops_equal_cut_then_assemble_bit_for_bit(norm_mode, C):
    net = _ctx()
    scenes = _scenes(C, seed=C)
    gp = (torch.linspace(-0.5, 0.7, C), torch.linspace(0.5, 2.0, C)) if norm_mode == "global" else None
    for rows in (list(range(len(BOXES))), [3], [7, 1, 6, 2]):
        boxes = [BOXES[r] for r in rows]
        got = scene_crops(net._ctx, [(scenes[b[0]], b[1:]) for b in boxes], (32, 32), norm_mode, gp)
        want = _reference(scenes, boxes, C, norm_mode, gp)
        torch.cuda.synchronize()
        for g_, w_ in zip(got, want):
            assert _bits_equal(g_, w_), (norm_mode, C, rows)
    if norm_mode == "local":                     # the statistics are per box: a partial box is not the padded tile's
        m = scene_crops(net._ctx, [(scenes[0], (64, 40, 70, 53))], (32, 32), "local")[1]
        assert torch.allclose(m[0, :, 0, 0].double(), scenes[0][:, 64:70, 40:53].double().mean((1, 2)), atol=1e-6)


def test_scene_crops_reject_bad_calls_without_launching():
    net = _ctx()
    lib = _lib.load()
    scene = torch.rand(2, 40, 50, device=DEV)
    out = torch.full((2, 2, 32, 32), 7.0, device=DEV)
    mean, std = torch.full((2, 2), 7.0, device=DEV), torch.full((2, 2), 7.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()

    def call(entries, n=None, C=2, tile=(32, 32), mode=0, m=None, s=None, gm=None, gs=None):
        n = len(entries) if n is None else n
        tab = (_lib.FuSceneCrop * max(len(entries), 1))(*[_lib.FuSceneCrop(p, sh, sw, *b) for p, sh, sw, b in entries])
        return lib.fu_scene_crops(net._ctx, n, tab, C, tile[0], tile[1], mode, gm, gs, 0.0, out.data_ptr(), m, s, stream)

    good = (scene.data_ptr(), 40, 50, (0, 0, 32, 32))
    cases = [([good, (scene.data_ptr(), 40, 50, (20, 30, 41, 50))], "outside its scene"),
             ([good, (scene.data_ptr(), 40, 50, (-1, 0, 10, 10))], "outside its scene"),
             ([good, (scene.data_ptr(), 40, 50, (5, 5, 5, 9))], "empty"),
             ([good, (scene.data_ptr(), 40, 50, (0, 0, 33, 8))], "larger than the tile"),
             ([good, (None, 40, 50, (0, 0, 8, 8))], "null scene")]
    for entries, msg in cases:
        assert call(entries) == _lib.FU_ERR_INVALID and msg.encode() in lib.fu_last_error(), msg
    assert call([good], n=0) == _lib.FU_ERR_INVALID
    assert call([good], mode=3) == _lib.FU_ERR_INVALID and b"norm_mode" in lib.fu_last_error()
    assert call([good], mode=1) == _lib.FU_ERR_INVALID and b"mean_out" in lib.fu_last_error()
    assert call([good], mode=1, m=mean.data_ptr()) == _lib.FU_ERR_INVALID
    assert call([good], mode=2) == _lib.FU_ERR_INVALID and b"global" in lib.fu_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((mean == 7.0).all()) and bool((std == 7.0).all())   # nothing ran
    assert call([good], mode=1, m=mean.data_ptr(), s=std.data_ptr()) == _lib.FU_OK
    torch.cuda.synchronize()
    assert not bool((out[0] == 7.0).any()) and bool((out[1] == 7.0).all())


def _host_grid(raster, H, W):
    """floodplanet.py's whole-raster path on the host: resize (a no-op at the same size), then the S1 scaling."""
    img = raster if raster.shape[1:] == (H, W) else resize_lanczos4(raster, H, W)
    return np.nan_to_num(np.clip((img + 50) / 100, 0, 1)).astype(np.float32)


@pytest.mark.parametrize("src,grid", [((36, 41), (36, 41)), ((40, 40), (100, 100)), ((1100, 37), (4500, 61)),
                                      ((300, 200), (77, 450))])
def test_whole_scene_resample_equals_host_restatement(src, grid):
    g = np.random.default_rng(sum(src) + sum(grid))
    raster = (g.random((2,) + src, dtype=np.float32) * 70 - 50).astype(np.float32)
    raster[0, 0, 0] = np.nan
    got = I.resident_grid(torch.from_numpy(raster), 1, grid, DEV).cpu().numpy()
    np.testing.assert_array_equal(got, _host_grid(raster, *grid))


def test_resample_guard_rejects_grids_one_launch_cannot_cover():
    raster = torch.zeros(1, 8, 8)
    with pytest.raises(_lib.FloodUNetError, match="too large"):
        I.resident_grid(raster, 0, (300000, 4), DEV)


@pytest.mark.parametrize("norm_mode", [None, "local"])
def test_resident_grid_crops_equal_tileloader_batches(tmp_path, norm_mode):
    from tools.tiff_writer import make_floodplanet_tree
    from floodplanet_code_amd.datasets import FloodplanetTiles, TileLoader, generate_image_slice_object
    root = str(tmp_path)
    make_floodplanet_tree(root, regions=("RegA", "RegB"), images_per_region=2, label_size=90, s1_size=37)
    ds = FloodplanetTiles(root, "test", generate_image_slice_object(32, 32, 24), eval_region=["RegA", "RegB"],
                          sensor="S1", ignore_index=0, norm_mode=norm_mode, output_metadata=True)
    net = _ctx()
    grids = {}
    n = 0
    for batch in TileLoader(ds, 7, DEV, device_assembly=True, device_resize=True):
        boxes = []
        for md in batch["metadata"]:
            p, cp = md["image_path"], md["crop_params"]
            if p not in grids:
                raster, _ = ds._load_raw_raster(p, "ALL")
                grids[p] = I.resident_grid(torch.from_numpy(raster), 1, (cp.og_height, cp.og_width), DEV)
            boxes.append((grids[p], (cp.h0, cp.w0, cp.hE, cp.wE)))
        got = scene_crops(net._ctx, boxes, (32, 32), norm_mode)
        torch.cuda.synchronize()
        for key, g_ in zip(("image", "mean", "std"), got):
            assert _bits_equal(g_, batch[key]), key
        n += len(boxes)
    assert n == len(ds) and len(grids) == 4


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """As test_gpu_predict's fixture: a one-epoch checkpoint of a 2-channel S1 model and a labelled tree."""
    from tools.tiff_writer import make_floodplanet_tree
    from floodplanet_code_amd.fit import SyntheticTiles, fit_model
    root = str(tmp_path_factory.mktemp("tree"))
    make_floodplanet_tree(root, regions=("RegA", "RegB"), images_per_region=2, label_size=100, s1_size=40)
    exp = str(tmp_path_factory.mktemp("exp"))
    ch = {"ms_image": 2}
    cfg = dict(lr=2e-3, n_epochs=1, batch_size=2, save_topk_models=1, ignore_index=0, crop_height=64, crop_width=64,
               crop_stride=32, eval_region=["RegA", "RegB"], n_workers=0,
               model=dict(name="ms_model", model_kwargs=dict(optimizer_name="adam", base_channels=8, precision="fp32")))
    ckpt = fit_model(cfg, SyntheticTiles(3, 2, ch, 64, 64, DEV, seed=1), SyntheticTiles(1, 2, ch, 64, 64, DEV, seed=2),
                     ch, 3, exp_dir=exp, device=DEV)
    return root, exp, ckpt


@pytest.mark.parametrize("tta", [None, "d4"])
def test_infer_canvases_equal_predict_bit_for_bit(trained, tmp_path, tta):
    from floodplanet_code_amd import predict as P
    root, exp, ckpt = trained
    cfg = P.resolve_cfg(exp, ckpt)
    per_scene = len(I.crop_boxes(100, 100, 64, 64, 32))
    assert per_scene == 9
    pred = P.predict(cfg, exp, ckpt, "floodplanet", predict_images=True, eval_dataset_split="test", n_workers=0,
                     data_root=root, batch_size=per_scene, device=DEV, tta=tta)["probabilities"]
    paths = sorted(os.path.join(root, "CSDAP_complete", key.split("/")[0], "S1", key.split("/")[1] + ".tif")
                   for key in pred)
    out = I.infer(ckpt, paths, str(tmp_path / "out"), cfg=cfg, size=(100, 100), stride=32, batch_size=per_scene,
                  tta=tta, keep_probabilities=True)
    assert out["n_scenes"] == len(pred) == 4 and out["n_crops"] == 4 * per_scene
    for rec in out["scenes"]:
        region = os.path.basename(os.path.dirname(os.path.dirname(rec["input"])))
        name = os.path.splitext(os.path.basename(rec["input"]))[0]
        want = pred[f"{region}/{name}"]
        got = out["probabilities"][rec["output"]]
        np.testing.assert_array_equal(got, want)
        cls = read_tiff(rec["output"])
        np.testing.assert_array_equal(cls, (np.clip(want.argmax(-1), 0, 1) * 255).astype(np.uint8))
        assert rec["output"] == str(tmp_path / "out" / f"{region}_pred" / f"{name}.tif")
        assert rec["class_pixels"] == np.bincount(want.argmax(-1).ravel(), minlength=3).tolist()


def _write_scenes(d, sizes, seed):
    from tools.tiff_writer import write_tiff
    g = np.random.default_rng(seed)
    paths = []
    for i, (h, w) in enumerate(sizes):
        s1 = (g.random((2, h, w), dtype=np.float32) * 70 - 50).astype(np.float32)
        p = os.path.join(d, "Scenes", f"S_{i:02d}.tif")
        write_tiff(p, s1, planar=2, rows_per_strip=7)
        paths.append(p)
    return paths


def test_infer_end_to_end_against_oracle(trained, tmp_path):
    from floodplanet_code_amd import predict as P
    root, exp, ckpt = trained
    cfg = P.resolve_cfg(exp, ckpt)
    sizes = [(40, 40), (37, 52), (20, 70), (33, 33)]
    paths = _write_scenes(str(tmp_path), sizes, seed=4)
    out = I.infer(ckpt, [str(tmp_path / "Scenes")], str(tmp_path / "out"), cfg=cfg, scale=2, stride=32, batch_size=5,
                  keep_probabilities=True)
    summary = json.load(open(tmp_path / "out" / "summary.json"))
    assert summary["n_crops"] == out["n_crops"] and summary["n_scenes"] == 4
    state = {k[len("model."):]: v.float().cpu() for k, v in torch.load(ckpt, weights_only=False)["state_dict"].items()}
    total = 0
    for rec, p, (h, w) in zip(summary["scenes"], paths, sizes):
        assert rec["input"] == p and rec["source_size"] == [h, w] and rec["grid_size"] == [2 * h, 2 * w]
        H, W = 2 * h, 2 * w
        grid = _host_grid(read_tiff(p), H, W)
        boxes = I.crop_boxes(H, W, 64, 64, 32)
        assert rec["crops"] == len(boxes)
        total += len(boxes)
        x = torch.zeros(len(boxes), 2, 64, 64)
        for i, (h0, w0, hE, wE) in enumerate(boxes):
            x[i, :, :hE - h0, :wE - w0] = torch.from_numpy(grid[:, h0:hE, w0:wE])
        logits = O.unet_forward(dict(state), x, False).numpy()
        want = O.stitch_reference(logits, boxes, H, W)[0]
        got = out["probabilities"][rec["output"]]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-4)
        srt = np.sort(want, axis=-1)
        decided = (srt[..., -1] - srt[..., -2]) > 1e-4
        cls = read_tiff(rec["output"])
        np.testing.assert_array_equal(cls[decided], (np.clip(want.argmax(-1), 0, 1) * 255).astype(np.uint8)[decided])
        assert sum(rec["class_pixels"]) == H * W
    assert total == summary["n_crops"] and total % 5 != 0          # batches cross scene boundaries, the last is partial


def test_resident_scenes_stay_bounded(trained, tmp_path):
    from floodplanet_code_amd import predict as P
    root, exp, ckpt = trained
    cfg = P.resolve_cfg(exp, ckpt)
    sizes = [(50 + 13 * (i % 4), 70 + 17 * (i % 3)) for i in range(12)]
    _write_scenes(str(tmp_path), sizes, seed=8)
    bs = 4
    out = I.infer(ckpt, [str(tmp_path / "Scenes")], str(tmp_path / "out"), cfg=cfg, stride=32, batch_size=bs)
    owners = [i for i, (h, w) in enumerate(sizes) for _ in I.crop_boxes(h, w, 64, 64, 32)]
    batches = [set(owners[j:j + bs]) for j in range(0, len(owners), bs)]
    bound = max(len(a | b) for a, b in zip(batches, batches[1:]))
    assert out["n_scenes"] == 12 and out["n_crops"] == len(owners)
    assert 1 <= out["max_resident_scenes"] <= bound < 12
    assert len(os.listdir(tmp_path / "out" / "Scenes_pred")) == 12


OPTION_SETS = [dict(), dict(tta="flips", blend="hann", write_probs="u8", write_margin=True),
               dict(write_probs="f32", sieve=4, water_threshold=0.4)]


@pytest.mark.parametrize("kw", OPTION_SETS, ids=["defaults", "flips+hann+u8+margin", "f32+sieve+threshold"])
def test_infer_with_options_equals_infer_with_keywords(trained, tmp_path, kw):
    """One InferOptions and the loose keywords are the same run: byte-identical rasters, equal summaries (but for the two
    timings).  A scene smaller than a crop, one of several crops and one of exactly a crop, batches that straddle them."""
    from floodplanet_code_amd import predict as P
    from floodplanet_code_amd.infer_options import InferOptions
    root, exp, ckpt = trained
    cfg = P.resolve_cfg(exp, ckpt)
    _write_scenes(str(tmp_path), [(40, 50), (70, 90), (64, 64)], seed=11)
    kw = dict(kw, stride=32, batch_size=3)
    runs = {}
    for form in ("options", "keywords"):
        out_dir = tmp_path / form
        how = dict(options=InferOptions.make(**kw)) if form == "options" else kw
        out = I.infer(ckpt, [str(tmp_path / "Scenes")], str(out_dir), cfg=cfg, **how)
        files = sorted(os.listdir(out_dir / "Scenes_pred"))
        text = (out_dir / "summary.json").read_text()
        assert out == json.loads(text)                                         # what it returns is what it wrote
        summary = json.loads(text.replace(str(out_dir), "OUT"))
        del summary["seconds"], summary["crops_per_s"]
        runs[form] = (files, [open(out_dir / "Scenes_pred" / f, "rb").read() for f in files], summary)
    files, blobs, summary = runs["options"]
    assert len(files) == 3 * (1 + ("write_probs" in kw) + ("write_margin" in kw))
    assert runs["keywords"][0] == files and runs["keywords"][1] == blobs                         # byte-identical rasters
    assert runs["keywords"][2] == summary
    assert [s["crops"] for s in summary["scenes"]] == [1, 4, 4] and summary["n_crops"] == 9     # batches straddle scenes
    assert summary["max_resident_scenes"] == 2 and summary["stride"] == 32
    assert ("sieve" in summary) == ("sieve" in kw) and ("threshold" in summary) == ("water_threshold" in kw)
