"""CPU: the numpy statement of the zoom of fu_scene_train_tiles_ex (sampling.zoom_tile_host) against torch's interpolate, and
the draw of the zoomed boxes (sampling.zoom_boxes)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from floodplanet_code_amd.datasets import sampling

# (source size, output size): magnify, reduce (a source larger than the tile), identity, one axis only, odd output
CASES = [((11, 13), (20, 24)), ((37, 41), (20, 24)), ((20, 24), (20, 24)), ((40, 48), (20, 24)), ((10, 12), (20, 24)),
         ((13, 24), (20, 24)), ((9, 7), (19, 21)), ((33, 29), (19, 21))]


def _tile(src, seed):
    rng = np.random.RandomState(seed)
    image = (rng.rand(3, *src) * 5 - 1).astype(np.float32)
    label = rng.randint(0, 4, size=src).astype(np.uint8)
    return image, label


@pytest.mark.parametrize("src, out", CASES)
def test_labels_equal_torch_nearest_exact(src, out):
    _, label = _tile(src, 1)
    got = sampling.zoom_tile_host(None, label, out)[1]
    want = F.interpolate(torch.from_numpy(label)[None, None].float(), size=out, mode="nearest-exact")[0, 0].numpy()
    assert got.dtype == np.uint8 and got.shape == out
    assert int((got != want.astype(np.uint8)).sum()) == 0


@pytest.mark.parametrize("src, out", CASES)
def test_image_equals_torch_bilinear_within_the_weight_rounding(src, out):
    """The two differ only in how the interpolation weights are rounded (torch computes the source coordinate as
    scale * (i + 0.5) - 0.5 with its own scale): a weight error of at most 2 spacings of the largest coordinate times the
    largest difference between neighbouring pixels, plus a few roundings of the value itself."""
    image, _ = _tile(src, 2)
    got = sampling.zoom_tile_host(image, None, out)[0]
    want = F.interpolate(torch.from_numpy(image)[None], size=out, mode="bilinear", align_corners=False)[0].numpy()
    dn = max(float(np.abs(np.diff(image, axis=1)).max()), float(np.abs(np.diff(image, axis=2)).max()))
    bound = 2 * float(np.spacing(np.float32(max(src)))) * dn + 4 * float(np.finfo(np.float32).eps) * float(np.abs(image).max())
    err = float(np.abs(got - want).max())
    print("src", src, "out", out, "max |numpy - torch|", err, "bound", bound)
    assert got.dtype == np.float32 and got.shape == (3,) + out
    assert err <= bound


@pytest.mark.parametrize("size", [(20, 24), (19, 21), (1, 1), (7, 1)])
def test_identity_zoom_returns_its_input_bit_for_bit(size):
    image, label = _tile(size, 3)
    got_i, got_l = sampling.zoom_tile_host(image, label, size)
    assert got_i.tobytes() == image.tobytes() and np.array_equal(got_l, label)
    i0, i1, w, nearest = sampling.zoom_axis_host(size[0], size[0])
    assert np.array_equal(i0, np.arange(size[0])) and np.array_equal(nearest, i0) and (w == 0).all()


def test_axis_taps_stay_inside_the_source():
    for src in (1, 2, 3, 7, 50, 511):
        for out in (1, 2, 5, 24, 256):
            i0, i1, w, nearest = sampling.zoom_axis_host(src, out)
            for a in (i0, i1, nearest):
                assert a.min() >= 0 and a.max() <= src - 1
            assert w.dtype == np.float32 and w.min() >= 0 and w.max() < 1 + 1e-6 and ((i1 - i0) <= 1).all()


def test_zoom_boxes_stay_inside_keep_output_sizes_and_are_deterministic():
    rasters = [(90, 90), (64, 200), (40, 40), (33, 70)]
    boxes, shapes = [], []
    for k, (H, W) in enumerate(rasters):
        for h0 in range(0, H, 24):
            for w0 in range(0, W, 24):
                boxes.append((h0, w0, min(h0 + 32, H), min(w0 + 32, W)))      # edge tiles are clipped
                shapes.append((H, W))
    src, out = sampling.zoom_boxes(boxes, shapes, (0.5, 2.0), seed=7, epoch=3)
    assert len(src) == len(out) == len(boxes)
    ratios = []
    for (h0, w0, hE, wE), (a, b, aE, bE), (oh, ow), (H, W) in zip(boxes, src, out, shapes):
        assert (oh, ow) == (hE - h0, wE - w0)                                  # the output size stays the box's own
        assert 0 <= a < aE <= H and 0 <= b < bE <= W                           # non-empty, inside the raster
        sh, sw = aE - a, bE - b
        assert sh <= max(2 * (hE - h0), 1) and sw <= max(2 * (wE - w0), 1)
        if 2 * (hE - h0) <= H:                                                 # not clamped to the raster: z within range
            ratios.append((hE - h0) / sh)
        if a > 0 and aE < H:                                                   # not shifted: the centre is kept
            assert abs((a + aE) - (h0 + hE)) <= 1
        if b > 0 and bE < W:
            assert abs((b + bE) - (w0 + wE)) <= 1
    ratios = np.array(ratios)
    assert ratios.min() >= 0.5 - 0.05 and ratios.max() <= 2.0 + 0.15 and ratios.min() < 0.8 and ratios.max() > 1.3
    assert sampling.zoom_boxes(boxes, shapes, (0.5, 2.0), seed=7, epoch=3) == (src, out)
    assert sampling.zoom_boxes(boxes, shapes, (0.5, 2.0), seed=7, epoch=4)[0] != src
    assert sampling.zoom_boxes(boxes, shapes, (0.5, 2.0), seed=8, epoch=3)[0] != src
    # a range of exactly 1 returns the boxes themselves
    assert sampling.zoom_boxes(boxes, shapes, (1.0, 1.0), seed=7, epoch=0) == ([tuple(b) for b in boxes], out)
    # the draws are log-uniform: about half of them magnify
    z = np.array([(hE - h0) / (aE - a) for (h0, _, hE, _), (a, _, aE, _), (H, _) in zip(boxes, src, shapes) if hE - h0 == 32])
    assert 0.3 < (z > 1).mean() < 0.7


@pytest.mark.parametrize("bad", [(0.0, 1.0), (1.2, 0.8), (0.4, 1.0), (1.0, 2.5), (-1.0, 1.0), (1.0,), "wide"])
def test_zoom_range_is_checked(bad):
    with pytest.raises(ValueError):
        sampling.check_zoom_range(bad)
    with pytest.raises(ValueError):
        sampling.zoom_boxes([(0, 0, 8, 8)], [(16, 16)], bad, 0, 0)
