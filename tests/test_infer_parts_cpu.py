"""CPU: the parts infer() is made of, each on its own and without a GPU -- stitch.PackedRead (several tensors, one read),
infer.SceneQueue (which crops run in which batch, which scenes finish after it, what is resident) and infer.write_scene
(arrays in, rasters and the summary record out)."""
import itertools
import os

import numpy as np
import pytest
import torch

from floodplanet_code_amd import infer as I
from floodplanet_code_amd.datasets.tiff import read_geotiff_tags, read_tiff
from floodplanet_code_amd.infer_options import InferOptions
from floodplanet_code_amd.stitch import PackedRead

K, H, W = 3, 3, 5            # 15 pixels: the fp32 canvas starts at a byte offset that 4 does not divide


def _scene_arrays(seed=0):
    g = np.random.default_rng(seed)
    return {"counts": g.integers(0, 1 << 40, K).astype(np.int64), "class": g.integers(0, 2, (H, W)).astype(np.uint8) * 255,
            "probs": g.integers(0, 256, (K, H, W)).astype(np.uint8), "margin": g.integers(0, 256, (H, W)).astype(np.uint8),
            "canvas": g.random((H, W, K), dtype=np.float32), "sieve": np.array([7, 1 << 33], np.int64)}


# ------------------------------------------------------------------------------------------------------- PackedRead
@pytest.mark.parametrize("write_probs,margin,sieve", list(itertools.product([None, "u8", "f32"], [False, True],
                                                                            [False, True])))
def test_packed_read_round_trips_every_combination(write_probs, margin, sieve, monkeypatch):
    want = _scene_arrays()
    names = ["counts", "class"] + ["probs"] * (write_probs == "u8") + ["margin"] * margin \
        + ["canvas"] * (write_probs == "f32") + ["sieve"] * sieve                 # finalize_scene's order
    tensors = {n: torch.from_numpy(want[n].copy()) for n in names}
    cats = []
    real_cat = torch.cat
    monkeypatch.setattr(torch, "cat", lambda parts, *a, **k: cats.append(len(parts)) or real_cat(parts, *a, **k))
    read = PackedRead()
    for n in names:
        read.add(n, tensors[n])
    got = read.read()
    assert cats == [len(names)]                                                   # one concatenation: one read
    assert list(got) == names
    for n in names:
        assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, n
        assert got[n].tobytes() == want[n].tobytes(), n                           # bit-equal
    if write_probs == "f32":
        assert (8 * K + H * W * (1 + margin)) % 4 != 0                            # (the canvas does sit unaligned)
    with pytest.raises(ValueError, match="registered twice"):
        read.add("class", tensors["class"])


def test_packed_read_sees_what_is_written_before_the_read():
    """The parts are views: an in-place change between add and read (the sieve's) is what comes back."""
    t = torch.zeros(H, W, dtype=torch.uint8)
    read = PackedRead()
    read.add("class", t)
    t[1, 2] = 9
    assert read.read()["class"][1, 2] == 9


# -------------------------------------------------------------------------------------------------------- SceneQueue
def test_scene_queue_batches_finishes_and_uploads_lazily():
    n_boxes = [1, 5, 2]
    uploaded, decoded = [], []

    def scenes():
        for i in range(3):
            decoded.append(i)
            yield {"index": i}

    def upload(item):
        i = item["index"]
        uploaded.append(i)
        return i, f"scene{i}", [f"b{j}" for j in range(n_boxes[i])]

    queue = I.SceneQueue(scenes(), upload, 3)
    batches, finished, uploaded_by, resident_at = [], [], [], []
    for batch in queue.batches():
        batches.append(batch)
        uploaded_by.append(list(uploaded))
        resident_at.append(list(queue.resident))
        assert all(queue.resident[i] == f"scene{i}" for i, _ in batch)           # a batch's scenes are resident
        finished.append(queue.stitched(batch))
    assert batches == [[(0, "b0"), (1, "b0"), (1, "b1")], [(1, "b2"), (1, "b3"), (1, "b4")], [(2, "b0"), (2, "b1")]]
    assert finished == [[(0, "scene0")], [(1, "scene1")], [(2, "scene2")]]
    assert uploaded_by == [[0, 1], [0, 1], [0, 1, 2]] and decoded == [0, 1, 2]    # nothing before it is needed
    assert resident_at == [[0, 1], [1], [2]] and queue.max_resident == 2
    assert not queue.resident


def test_scene_queue_reports_scenes_in_scene_order_and_handles_no_scenes():
    queue = I.SceneQueue(iter([{"index": i} for i in range(3)]), lambda it: (it["index"], it["index"], ["a"]), 4)
    (batch,) = list(queue.batches())
    assert batch == [(0, "a"), (1, "a"), (2, "a")] and queue.max_resident == 3
    assert queue.stitched(batch) == [(0, 0), (1, 1), (2, 2)]
    empty = I.SceneQueue(iter([]), lambda it: pytest.fail("nothing to upload"), 4)
    assert list(empty.batches()) == [] and empty.max_resident == 0


# ------------------------------------------------------------------------------------------------------- write_scene
TAGS = {33550: (10.0, 10.0, 0.0), 33922: (0.0, 0.0, 0.0, 500000.0, 4000000.0, 0.0)}
BASE_KEYS = ["input", "output", "source_size", "grid_size", "crops", "class_pixels"]


@pytest.mark.parametrize("kw,files,keys", [
    (dict(), [""], BASE_KEYS),
    (dict(write_probs="u8", write_margin=True), ["", "_prob", "_margin"], BASE_KEYS + ["probabilities", "margin"]),
    (dict(write_probs="f32", sieve=4), ["", "_prob"], BASE_KEYS + ["probabilities", "sieve"]),
], ids=["plain", "u8+margin", "f32+sieve"])
def test_write_scene_writes_the_rasters_and_returns_the_record(kw, files, keys, tmp_path):
    arrays = _scene_arrays(seed=1)
    options = InferOptions.make(**kw).resolve(64, 64, 4)
    scene = {"hw": (H, W), "src_hw": (2 * H, 2 * W), "tags": TAGS, "n": 4}
    out = str(tmp_path / "R_pred" / "img.tif")
    rec = I.write_scene(arrays, scene, options, "/in/R/S1/img.tif", out)
    assert list(rec) == keys
    assert sorted(os.listdir(tmp_path / "R_pred")) == sorted("img" + f + ".tif" for f in files)
    assert (rec["input"], rec["output"], rec["source_size"], rec["grid_size"], rec["crops"]) \
        == ("/in/R/S1/img.tif", out, [2 * H, 2 * W], [H, W], 4)
    assert rec["class_pixels"] == arrays["counts"].tolist()
    cls = read_tiff(out)
    assert cls.dtype == np.uint8 and np.array_equal(cls, arrays["class"])
    for f in files:                                                               # every raster carries the footprint
        tags = read_geotiff_tags(out[:-4] + f + ".tif")
        assert tuple(tags[33550]) == (20.0, 20.0, 0.0) and tuple(tags[33922]) == TAGS[33922]
    if kw.get("write_probs") == "u8":
        prob = read_tiff(rec["probabilities"])
        assert rec["probabilities"] == out[:-4] + "_prob.tif" and prob.dtype == np.uint8
        assert np.array_equal(prob, arrays["probs"])
        assert np.array_equal(read_tiff(rec["margin"]), arrays["margin"]) and rec["margin"] == out[:-4] + "_margin.tif"
    if kw.get("write_probs") == "f32":
        prob = read_tiff(rec["probabilities"])
        assert prob.dtype == np.float32 and prob.shape == (K, H, W)
        assert prob.tobytes() == np.ascontiguousarray(arrays["canvas"].transpose(2, 0, 1)).tobytes()
        assert rec["sieve"] == {"min_pixels": 4, "connectivity": 4, "passes": 1, "merged_components": 7,
                                "changed_pixels": 1 << 33}
        assert list(rec["sieve"]) == ["min_pixels", "connectivity", "passes", "merged_components", "changed_pixels"]


def test_run_summary_keys_and_their_conditions():
    plain = InferOptions.make().resolve(64, 64, 4)
    s = I.run_summary([], 0, 0.0, 0, plain, "raw")
    assert list(s) == ["scenes", "n_scenes", "n_crops", "seconds", "crops_per_s", "max_resident_scenes", "tta", "weights",
                       "blend", "stride"]
    assert (s["crops_per_s"], s["tta"], s["weights"], s["blend"], s["stride"]) == (None, None, "raw", "uniform", 64)
    full = InferOptions.make(tta=[0, 3], blend="hann", sieve=4, water_threshold=0.4).resolve(64, 64, 4)
    recs = [{"sieve": {"merged_components": 2, "changed_pixels": 5}},
            {"sieve": {"merged_components": 1, "changed_pixels": 3}}]
    s = I.run_summary(recs, 18, 2.0, 2, full, "ema")
    assert list(s)[-2:] == ["threshold", "sieve"] and s["tta"] == [0, 3] and s["crops_per_s"] == 9.0 and s["stride"] == 32
    assert s["threshold"] == {"class": 1, "threshold": 0.4, "source": "option"}
    assert s["sieve"] == {"min_pixels": 4, "connectivity": 4, "passes": 1, "merged_components": 3, "changed_pixels": 8}
    assert I.run_summary([], 0, 1.0, 0, InferOptions.make(tta="d4").resolve(64, 64, 4), "raw")["tta"] == "d4"
