"""CPU: the host side of batched scene prediction (floodplanet_code_amd.predict) -- ranked lists, output directory,
config resolution, PNG writer -- and the argument checks of fu_stitch_add_batch that need no context."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd import predict as P


def test_ranked_image_text_matches_the_reference_layout():
    # two images tie at 0.5 (the larger path comes first), values whose x100 shows float rounding
    stats = {"/d/CSDAP_complete/RegA/S1/AAA_0_7.tif": [0.5, 0.5],
             "/d/CSDAP_complete/RegB/S1/BBB_1_8.tif": [0.25, 0.75],
             "/d/CSDAP_complete/RegC/S1/CCC_2_9.tif": [0.1, 0.2],
             "/d/CSDAP_complete/RegA/S1/DDD_3_10.tif": [1.0]}
    want = ("Ranked image F1-score \n"
            "---------------------- \n"
            "DDD_3_10: 100.0% \n"
            "BBB_1_8: 50.0% \n"
            "AAA_0_7: 50.0% \n"
            "CCC_2_9: 15.000000000000002% \n")
    assert P.ranked_images_text(stats, "F1-score") == want


def test_ranked_region_text_matches_the_reference_layout():
    stats = {"RegA": [0.3], "RegB": [0.7, 0.1], "RegC": [0.4]}
    want = ("Ranked region iou \n"
            "---------------------- \n"
            "RegC: 40.0% \n"
            "RegB: 40.0% \n"
            "RegA: 30.0% \n")
    assert P.ranked_regions_text(stats, "iou") == want


def test_ranked_files_written_with_reference_names(tmp_path):
    img = {"/x/R/S1/A_1.tif": [0.5]}
    P.write_ranked_files(str(tmp_path), img, img, {"R": [0.5]}, {"R": [0.25]})
    assert sorted(os.listdir(tmp_path)) == ["ranked_images_F1-score.txt", "ranked_images_mIoU.txt",
                                            "ranked_regions_F1-Score.txt", "ranked_regions_iou.txt"]
    assert (tmp_path / "ranked_regions_iou.txt").read_text() == \
        "Ranked region iou \n---------------------- \nR: 25.0% \n"
    other = tmp_path / "no_regions"
    other.mkdir()
    P.write_ranked_files(str(other), img, img, {}, {})
    assert sorted(os.listdir(other)) == ["ranked_images_F1-score.txt", "ranked_images_mIoU.txt"]


def test_prediction_dir_and_checkpoint_name_quirk():
    ck = "/e/xp/checkpoints/model-epoch=01-val_MulticlassJaccardIndex=0.4321.ckpt"
    cfg = dict(P.CONFIG_DEFAULTS, eval_region=None)
    assert P.prediction_dir(cfg, "/e/xp", ck, "floodplanet") == \
        "/e/xp/predictions_PS_alldata_4/floodplanet/split_pct_0.8/model-epoch=01-val_MulticlassJaccardIndex=0"
    cfg["eval_region"] = "RegA"
    assert P.prediction_dir(cfg, "/e/xp", ck, "floodplanet") == \
        "/e/xp/predictions_PS_alldata_4/floodplanet/RegA/model-epoch=01-val_MulticlassJaccardIndex=0"
    cfg["eval_region"] = ["RegA", "RegC"]
    assert P.prediction_dir(cfg, "/e/xp", ck, "floodplanet").endswith("/floodplanet/RegA_RegC/"
                                                                      "model-epoch=01-val_MulticlassJaccardIndex=0")


def test_cfg_from_checkpoint_hyper_parameters_without_yaml(tmp_path):
    exp = tmp_path / "exp"
    (exp / "checkpoints").mkdir(parents=True)
    ck = exp / "checkpoints" / "model-epoch=00-val_MulticlassJaccardIndex=0.1000.ckpt"
    hp = {"lr": 3e-4, "batch_size": 4, "crop_height": 64, "crop_width": 64, "eval_region": None,
          "model": {"name": "ms_model", "model_kwargs": {"base_channels": 8, "precision": "fp32"}}}
    torch.save({"state_dict": {}, "epoch": 0, "hyper_parameters": hp}, str(ck))
    cfg = P.resolve_cfg(str(exp), str(ck))
    assert cfg["lr"] == 3e-4 and cfg["batch_size"] == 4 and cfg["crop_height"] == 64
    assert cfg["crop_stride"] == 150 and cfg["train_split_pct"] == 0.8 and cfg["n_workers"] == 4   # conf/config.yaml
    assert cfg["eval_region"] is None
    assert cfg["model"]["name"] == "ms_model" and cfg["model"]["model_kwargs"]["base_channels"] == 8
    assert cfg["dataset"] == {"name": "floodplanet", "channels": "ALL", "sensor": "S1", "dataset_kwargs": None}


def _png_decode(path):
    """Minimal decoder for what write_png emits (8-bit, filter 0, one IDAT)."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 4], "big")
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert int.from_bytes(data[pos + 8 + n:pos + 12 + n], "big") == zlib.crc32(tag + body)
        chunks[tag] = body
        pos += 12 + n
    w, h = int.from_bytes(chunks[b"IHDR"][:4], "big"), int.from_bytes(chunks[b"IHDR"][4:8], "big")
    ch = {0: 1, 2: 3, 6: 4}[chunks[b"IHDR"][9]]
    raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(h, 1 + w * ch)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, ch)


@pytest.mark.parametrize("shape", [(7, 5), (6, 9, 3), (4, 3, 4)])
def test_png_writer_round_trip(tmp_path, shape):
    a = np.random.default_rng(1).integers(0, 256, size=shape, dtype=np.uint8)
    path = str(tmp_path / "x.png")
    P.write_png(path, a)
    got = _png_decode(path)
    np.testing.assert_array_equal(got.reshape(a.shape), a)


@pytest.mark.parametrize("shape", [(7, 5), (6, 9, 3), (4, 3, 4)])
def test_png_writer_round_trip_pil(tmp_path, shape):
    Image = pytest.importorskip("PIL.Image")
    a = np.random.default_rng(2).integers(0, 256, size=shape, dtype=np.uint8)
    path = str(tmp_path / "x.png")
    P.write_png(path, a)
    with Image.open(path) as im:
        np.testing.assert_array_equal(np.asarray(im), a)


def test_softmax_png_and_conf_matrix_image_rules():
    prob = np.array([[[0.2, 0.3, 0.5], [0.999, 0.0005, 0.0005]]], np.float32)
    np.testing.assert_array_equal(P.softmax_png(prob), (prob * 255).astype(np.uint8))
    pred = np.array([[1, 1, 0, 0, 2]])
    gt = np.array([[1, 0, 1, 0, 1]])
    cm = P.conf_matrix_image(pred, gt)
    np.testing.assert_array_equal(cm[0], [[255, 255, 255], [0, 255, 255], [255, 0, 0], [0, 0, 0], [0, 0, 0]])


def test_stitch_add_batch_rejects_bad_arguments_without_context():
    lib = _lib.load()
    table = (_lib.FuStitchEntry * 1)()
    assert lib.fu_stitch_add_batch(None, 1, table, None) == _lib.FU_ERR_INVALID
    assert b"fu_stitch_add_batch" in lib.fu_last_error()
    for n in (0, -3):
        assert lib.fu_stitch_add_batch(None, n, table, None) == _lib.FU_ERR_INVALID
        assert b"n = " in lib.fu_last_error()
    assert lib.fu_stitch_add_batch(None, 1, None, None) == _lib.FU_ERR_INVALID
    assert lib.fu_eval_confusion(None, None, 0, None, None) == _lib.FU_ERR_INVALID
    assert b"fu_eval_confusion" in lib.fu_last_error()
    assert ctypes.sizeof(_lib.FuStitchEntry) == 48
