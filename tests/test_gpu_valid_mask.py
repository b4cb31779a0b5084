"""GPU: nodata in scene inference -- fu_scene_valid_mask and fu_mask_box_counts against the numpy statements of
datasets/valid_mask.py, the masked finalisation against a numpy restatement written here, their rejected calls, and
infer --nodata end to end.  The rule is integer-exact: equality throughout, but for the one comparison between runs that
batch the same crops differently."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd import infer as I
from floodplanet_code_amd.datasets.tiff import read_geotiff_tags, read_tiff
from floodplanet_code_amd.datasets.valid_mask import (axis_tables, box_valid_counts, box_valid_counts_host, grid_valid_host,
                                                      scene_valid_mask, source_valid_host)
from floodplanet_code_amd.postprocess import sieve_host
from floodplanet_code_amd.stitch import GpuImageStitcher
from floodplanet_code_amd.unet import HipUNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _net(th=32, tw=32):
    net = HipUNet(2, 3, base_channels=8).to(DEV).eval()
    net._get_ctx(torch.device(DEV), 1, th, tw)
    return net                                   # keep the module alive: it owns the context


def fill_cases(C, h, w, nodata, seed=0):
    """The fill patterns of tests/test_valid_mask_cpu.py: a fill corner, a single fill pixel, NaN / Inf in one band, a pixel
    where only some bands equal nodata."""
    g = np.random.default_rng(seed)
    a = (g.random((C, h, w), dtype=np.float32) * 70 - 50).astype(np.float32)
    a[a == 0] = 1.0
    fill = np.float32(0 if nodata is None else nodata)
    a[:, :h // 3, : w // 4] = fill
    a[:, h // 2, w // 2] = fill
    a[C - 1, h - 2, 1] = np.nan
    a[0, h - 1, w - 1] = np.inf
    a[C // 2, 0, w - 1] = -np.inf
    a[0, h - 3, w - 3] = fill
    return a


# --------------------------------------------------------------------------------------------------------------- mask
# (37, 51): a pixel count that is no multiple of 4, so the bands are not aligned alike and go the plain way
SHAPES = [((37, 52), (37, 52)), ((37, 52), (74, 104)), ((37, 52), (23, 31)), ((64, 64), (64, 64)), ((37, 51), (37, 51))]


@pytest.mark.parametrize("nodata", [0, -9999, None], ids=["0", "-9999", "off"])
@pytest.mark.parametrize("C", [1, 2, 7])
@pytest.mark.parametrize("src,dst", SHAPES, ids=["identity", "2x", "0.6x", "aligned", "odd"])
def test_scene_valid_mask_equals_the_host_statement(src, dst, C, nodata):
    a = fill_cases(C, src[0], src[1], nodata)
    tables = axis_tables(src, dst)
    want = grid_valid_host(source_valid_host(a, nodata), *tables)
    mask, n_valid = scene_valid_mask(torch.from_numpy(a).to(DEV), nodata, axis_tables(src, dst, DEV))
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == dst and n_valid.dtype == torch.int64 and n_valid.shape == (1,)
    np.testing.assert_array_equal(mask.cpu().numpy(), want)
    assert int(n_valid.item()) == int(want.sum()) and 0 < want.sum() < want.size


@pytest.mark.parametrize("src,dst", SHAPES[1:4], ids=["2x", "0.6x", "aligned"])
def test_scene_without_a_valid_pixel_and_scene_without_fill(src, dst):
    tabs = axis_tables(src, dst, DEV)
    none = np.full((2,) + src, -9999, dtype=np.float32)
    none[1, 3, 5] = np.nan
    mask, n_valid = scene_valid_mask(torch.from_numpy(none).to(DEV), -9999, tabs)
    assert not mask.any() and int(n_valid.item()) == 0
    full = np.random.default_rng(1).random((2,) + src, dtype=np.float32) + 1
    mask, n_valid = scene_valid_mask(torch.from_numpy(full).to(DEV), 0, tabs)
    assert mask.all() and int(n_valid.item()) == dst[0] * dst[1]
    off = torch.from_numpy(np.concatenate([[0.0], full.ravel()]).astype(np.float32)).to(DEV)[1:].view(2, *src)
    mask, n_valid = scene_valid_mask(off, 0, tabs)            # a raster 4 bytes off the 16-byte boundary: head and plain path
    assert off.data_ptr() % 16 == 4 and mask.all() and int(n_valid.item()) == dst[0] * dst[1]


# ------------------------------------------------------------------------------------------------------------- census
@pytest.fixture(scope="module")
def census():
    m = (np.random.default_rng(3).random((100, 150)) < 0.6).astype(np.uint8)
    m[:64, 86:] = 0                                          # a box without a valid pixel among the twelve
    boxes = I.crop_boxes(100, 150, 64, 64, 32) + [(5, 7, 6, 8), (0, 0, 100, 150), (3, 33, 50, 80)]
    assert len(boxes) == 15
    return m, torch.from_numpy(m).to(DEV), boxes, box_valid_counts_host(m, boxes)


@pytest.mark.parametrize("n", [1, 15])
def test_box_valid_counts_equals_the_host_statement(census, n):
    m, dev, boxes, want = census
    net = _net()
    table = boxes[-2:-1] if n == 1 else boxes                 # n = 1: the whole mask, more work than the block has threads
    out = torch.full((n + 2,), -7, dtype=torch.int64, device=DEV)
    got = box_valid_counts(net._ctx, dev, table, counts=out)
    torch.cuda.synchronize()
    assert got.shape == (n,)
    np.testing.assert_array_equal(out.cpu().numpy()[:n], want[-2:-1] if n == 1 else want)   # written, not added to
    assert (out[n:] == -7).all()
    fresh = box_valid_counts(net._ctx, dev, table)
    np.testing.assert_array_equal(fresh.cpu().numpy(), out.cpu().numpy()[:n])
    if n == 15:
        assert (want[:12] == 0).sum() == 1 and want[-3] == m[5, 7] and want[-2] == m.sum()
        every = [(2, w0, 9, w0 + dw) for w0 in range(6) for dw in range(1, 12)]               # each head and tail
        np.testing.assert_array_equal(box_valid_counts(net._ctx, dev, every).cpu().numpy(), box_valid_counts_host(m, every))


# ----------------------------------------------------------------------------------------------------------- finalise
def quantize(x):
    return np.rint(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)


def finalize_host(canvas, weight, eps, class_values, thr, valid, nodata_value):
    """include/floodunet.h's statement of fu_stitch_finalize_maps_masked in numpy, every operation in fp32."""
    k = canvas.shape[-1]
    s = weight + np.float32(eps)
    live = s > 0
    if valid is not None:
        live = live & (valid != 0)
    inv = np.float32(1) / np.where(live, s, np.float32(1))
    v = np.where(live[..., None], canvas * inv[..., None], np.float32(0)).astype(np.float32)
    am = v.argmax(-1)
    decided = am.copy()
    if thr is not None:
        cls, t = thr
        others = v.copy()
        others[..., cls] = -np.inf
        decided = np.where(v[..., cls] >= np.float32(t), cls, others.argmax(-1))
    decided[~live] = 0
    srt = np.sort(v, axis=-1)
    margin = np.where(live, srt[..., -1] - srt[..., -2], np.float32(0))
    cmap = np.asarray(class_values if class_values is not None else range(k), dtype=np.uint8)[decided]
    if valid is not None:
        cmap[valid == 0] = nodata_value
    return {"canvas": v, "class": cmap, "probs": quantize(v).transpose(2, 0, 1), "margin": quantize(margin),
            "counts": np.bincount(decided[live], minlength=k).astype(np.int64)}


def _canvas(H, W, k, seed):
    g = np.random.default_rng(seed)
    weight = g.integers(0, 4, (H, W)).astype(np.float32)
    p = g.random((H, W, k), dtype=np.float32)
    p /= p.sum(-1, keepdims=True)
    canvas = (p * weight[..., None]).astype(np.float32)
    valid = (g.random((H, W)) < 0.7).astype(np.uint8)
    return canvas, weight, valid


def _combine(canvas, weight, eps, offset=0, **kw):
    """combine_maps of a stitcher that holds this one canvas; eps 0 = a window blend's.  offset 1: canvas, weight and mask
    start one element past an aligned allocation."""
    def dev(a, dtype):
        t = torch.zeros(a.size + offset, dtype=dtype, device=DEV)
        t[offset:] = torch.from_numpy(a.ravel()).to(DEV)
        return t[offset:].view(a.shape)
    k = canvas.shape[-1]
    st = GpuImageStitcher(types.SimpleNamespace(n_classes=k, _ctx=None), DEV, blend="uniform" if eps else "hann")
    st.image_canvas["a"], st.weight_canvas["a"] = dev(canvas, torch.float32), dev(weight, torch.float32)
    if kw.get("valid") is not None:
        kw["valid"] = dev(kw["valid"], torch.uint8)
        assert kw["valid"].data_ptr() % 4 == offset
    out = st.combine_maps("a", probs=True, margin=True, counts=True, **kw)
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


@pytest.mark.parametrize("thr", [None, (1, 0.4)], ids=["argmax", "threshold"])
@pytest.mark.parametrize("eps", [1e-5, 0.0])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("hw", [(45, 37), (64, 64)])
def test_masked_finalisation_equals_its_numpy_statement(hw, k, eps, thr):
    canvas, weight, valid = _canvas(hw[0], hw[1], k, seed=hw[0] + k)
    values = [0] + [255] * (k - 1)
    want = finalize_host(canvas, weight, eps, values, thr, valid, 127)
    assert (want["class"] == 127).sum() == (valid == 0).sum() > 0
    for offset in (0, 1):                                     # aligned, and the plain path of misaligned views
        got = _combine(canvas, weight, eps, offset, class_values=values, threshold=thr, valid=valid, nodata_value=127)
        for name in ("canvas", "class", "probs", "margin", "counts"):
            np.testing.assert_array_equal(got[name], want[name], err_msg=f"{name}, offset {offset}")
    plain_want = finalize_host(canvas, weight, eps, values, thr, None, None)
    for offset in (0, 1):                                     # valid=None: the existing path, byte for byte
        got = _combine(canvas, weight, eps, offset, class_values=values, threshold=thr)
        for name in ("canvas", "class", "probs", "margin", "counts"):
            np.testing.assert_array_equal(got[name], plain_want[name], err_msg=f"plain {name}, offset {offset}")
    got = _combine(canvas, weight, eps, valid=valid, nodata_value=200)       # identity class values
    np.testing.assert_array_equal(got["class"], finalize_host(canvas, weight, eps, None, None, valid, 200)["class"])


def test_masked_entry_point_without_a_mask_is_the_existing_one():
    canvas, weight, _ = _canvas(45, 37, 3, seed=9)
    lib = _lib.load()
    outs = []
    for masked in (False, True):
        cv, wt = torch.from_numpy(canvas).to(DEV), torch.from_numpy(weight).to(DEV)
        cls = torch.full((45, 37), SENTINEL, dtype=torch.uint8, device=DEV)
        pr = torch.full((3, 45, 37), SENTINEL, dtype=torch.uint8, device=DEV)
        mg = torch.full((45, 37), SENTINEL, dtype=torch.uint8, device=DEV)
        cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
        args = [_lib.ptr(cv), _lib.ptr(wt), 3, 45, 37, 1e-5, 1, None, _lib.ptr(cls), _lib.ptr(pr), _lib.ptr(mg), _lib.ptr(cnt),
                None]
        if masked:
            _lib.check(lib.fu_stitch_finalize_maps_masked(*args, None, -5, _stream()))    # nodata_value is not looked at
        else:
            _lib.check(lib.fu_stitch_finalize_maps_ex(*args, _stream()))
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (cv, cls, pr, mg, cnt)])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


# --------------------------------------------------------------------------------------------------------- rejections
def test_rejected_mask_calls_leave_the_outputs_at_their_sentinel():
    lib = _lib.load()
    src, dst = (12, 20), (24, 40)
    raster = torch.ones(2, *src, device=DEV)
    iy, wy, ix, wx = axis_tables(src, dst, DEV)
    scratch = torch.full(src, SENTINEL, dtype=torch.uint8, device=DEV)
    mask = torch.full(dst, SENTINEL, dtype=torch.uint8, device=DEV)
    n_valid = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    good = dict(raster=_lib.ptr(raster), C=2, src_h=src[0], src_w=src[1], use_nodata=1, nodata=0.0, iy=_lib.ptr(iy),
                wy=_lib.ptr(wy), ix=_lib.ptr(ix), wx=_lib.ptr(wx), grid_h=dst[0], grid_w=dst[1], scratch=_lib.ptr(scratch),
                mask=_lib.ptr(mask), n_valid=_lib.ptr(n_valid))
    bad = [dict(raster=None), dict(iy=None), dict(wy=None), dict(ix=None), dict(wx=None), dict(scratch=None), dict(mask=None),
           dict(n_valid=None), dict(C=0), dict(C=17), dict(src_h=0), dict(src_w=0), dict(grid_h=0), dict(grid_w=-1),
           dict(grid_h=1 << 15, grid_w=(1 << 13) + 1), dict(src_h=1 << 14, src_w=(1 << 14) + 1),
           dict(nodata=float("nan")), dict(nodata=float("inf"))]
    for change in bad:
        status = lib.fu_scene_valid_mask(*dict(good, **change).values(), _stream())
        assert status == _lib.FU_ERR_INVALID and lib.fu_last_error(), change
    assert lib.fu_scene_valid_mask(*dict(good, use_nodata=0, nodata=float("nan")).values(), _stream()) == _lib.FU_OK
    torch.cuda.synchronize()
    assert mask.all() and (mask == 1).all() and int(n_valid.item()) == dst[0] * dst[1]       # the good call wrote them
    mask.fill_(SENTINEL), n_valid.fill_(-7), scratch.fill_(SENTINEL)
    for change in bad:
        lib.fu_scene_valid_mask(*dict(good, **change).values(), _stream())
    torch.cuda.synchronize()
    assert (mask == SENTINEL).all() and (scratch == SENTINEL).all() and int(n_valid.item()) == -7


def test_rejected_census_calls_leave_the_counts_at_their_sentinel(census):
    m, dev, boxes, want = census
    lib = _lib.load()
    net = _net()
    counts = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    H, W = m.shape

    def call(entries, n=None, ctx=net._ctx, out=counts):
        table = (_lib.FuMaskBox * max(len(entries), 1))(*[_lib.FuMaskBox(*e) for e in entries])
        return lib.fu_mask_box_counts(ctx, len(entries) if n is None else n, table, _lib.ptr(out), _stream())

    p = dev.data_ptr()
    ok = (p, H, W, 0, 0, 10, 10)
    for entries, kw in [([ok], dict(n=0)), ([ok], dict(n=-1)), ([ok], dict(ctx=None)), ([ok], dict(out=None)),
                        ([(None, H, W, 0, 0, 10, 10)], {}), ([ok, (p, 0, W, 0, 0, 1, 1)], {}), ([(p, H, 0, 0, 0, 1, 1)], {}),
                        ([ok, (p, H, W, 0, 0, H + 1, 10)], {}), ([(p, H, W, 0, 0, 10, W + 1)], {}),
                        ([(p, H, W, -1, 0, 10, 10)], {}), ([(p, H, W, 0, -1, 10, 10)], {}), ([(p, H, W, 5, 5, 5, 9)], {}),
                        ([(p, H, W, 5, 5, 9, 4)], {}), ([(p, 1 << 14, (1 << 14) + 1, 0, 0, 1, 1)], {})]:
        assert call(entries, **kw) == _lib.FU_ERR_INVALID and lib.fu_last_error(), (entries, kw)
    assert lib.fu_mask_box_counts(net._ctx, 1, None, _lib.ptr(counts), _stream()) == _lib.FU_ERR_INVALID
    torch.cuda.synchronize()
    assert (counts == -7).all()
    assert call([ok]) == _lib.FU_OK and int(counts[0].item()) == int(m[:10, :10].sum()) and (counts[1:] == -7).all()


def test_rejected_masked_finalisations_leave_the_outputs_at_their_sentinel():
    lib = _lib.load()
    canvas, weight, valid = _canvas(12, 9, 3, seed=2)
    cv, wt, vd = (torch.from_numpy(t).to(DEV) for t in (canvas, weight, valid))
    cls = torch.full((12, 9), SENTINEL, dtype=torch.uint8, device=DEV)
    pr = torch.full((3, 12, 9), SENTINEL, dtype=torch.uint8, device=DEV)
    mg = torch.full((12, 9), SENTINEL, dtype=torch.uint8, device=DEV)
    cnt = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    values = (ctypes.c_uint8 * 3)(0, 255, 255)

    def call(class_values=values, nodata_value=127, h=12, w=9):
        return lib.fu_stitch_finalize_maps_masked(_lib.ptr(cv), _lib.ptr(wt), 3, h, w, 1e-5, 1, class_values, _lib.ptr(cls),
                                                  _lib.ptr(pr), _lib.ptr(mg), _lib.ptr(cnt), None, _lib.ptr(vd),
                                                  nodata_value, _stream())

    for kw in (dict(nodata_value=-1), dict(nodata_value=256), dict(class_values=None, nodata_value=2),
               dict(class_values=None, nodata_value=0), dict(nodata_value=255), dict(nodata_value=0),
               dict(h=1 << 14, w=(1 << 14) + 1), dict(h=0)):
        assert call(**kw) == _lib.FU_ERR_INVALID and lib.fu_last_error(), kw
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cv.cpu().numpy(), canvas)                  # not normalised either
    assert (cls == SENTINEL).all() and (pr == SENTINEL).all() and (mg == SENTINEL).all() and (cnt == -7).all()
    assert call(class_values=None, nodata_value=3) == _lib.FU_OK


# --------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """The recipe of test_gpu_infer's fixture: a one-epoch checkpoint of a 2-channel S1 model."""
    from floodplanet_code_amd import predict as P
    from floodplanet_code_amd.fit import SyntheticTiles, fit_model
    exp = str(tmp_path_factory.mktemp("exp"))
    ch = {"ms_image": 2}
    cfg = dict(lr=2e-3, n_epochs=1, batch_size=2, save_topk_models=1, ignore_index=0, crop_height=64, crop_width=64,
               crop_stride=32, eval_region=["RegA", "RegB"], n_workers=0,
               model=dict(name="ms_model", model_kwargs=dict(optimizer_name="adam", base_channels=8, precision="fp32")))
    ckpt = fit_model(cfg, SyntheticTiles(3, 2, ch, 64, 64, DEV, seed=1), SyntheticTiles(1, 2, ch, 64, 64, DEV, seed=2),
                     ch, 3, exp_dir=exp, device=DEV)
    return ckpt, P.resolve_cfg(exp, ckpt)


def _write(d, rasters):
    from tools.tiff_writer import write_tiff
    paths = []
    for i, a in enumerate(rasters):
        paths.append(os.path.join(d, "Scenes", f"S_{i:02d}.tif"))
        write_tiff(paths[-1], a, planar=2, rows_per_strip=7)
    return paths


def _s1(hw, seed):
    return (np.random.default_rng(seed).random((2,) + hw, dtype=np.float32) * 70 - 50).astype(np.float32)


def _files(rec):
    out = rec["output"]
    return {"class": read_tiff(out), "probs": read_tiff(I.side_output_path(out, "prob")),
            "margin": read_tiff(I.side_output_path(out, "margin"))}


SAME = dict(stride=32, batch_size=4, write_probs="u8", write_margin=True, keep_probabilities=True)


@pytest.fixture(scope="module")
def wedge_runs(trained, tmp_path_factory):
    """Two S1 scenes (100, 150), the first with a fill wedge (all bands exactly 0) and a few NaN pixels; the plain run and
    the run with nodata=0 that forwards the same batches."""
    ckpt, cfg = trained
    d = tmp_path_factory.mktemp("wedge")
    a, b = _s1((100, 150), 21), _s1((100, 150), 22)
    yy, xx = np.mgrid[:100, :150]
    a[:, xx > 60 + yy] = 0
    a[0, 80, 5] = a[1, 90, 30] = a[0, 91, 30] = np.nan
    paths = _write(str(d), [a, b])
    plain = I.infer(ckpt, paths, str(d / "plain"), cfg=cfg, **SAME)
    masked = I.infer(ckpt, paths, str(d / "masked"), cfg=cfg, nodata=0, skip_empty=False, write_valid=True, **SAME)
    return (a, b), paths, plain, masked, d


def test_infer_with_nodata_same_batches(wedge_runs):
    rasters, paths, plain, masked, d = wedge_runs
    assert masked["n_crops"] == plain["n_crops"] == 24 and masked["max_resident_scenes"] == plain["max_resident_scenes"]
    assert masked["nodata"] == {"value": 0.0, "out": 127, "skip_empty": False, "skipped_crops": 0,
                                "valid_pixels": sum(r["valid_pixels"] for r in masked["scenes"])}
    assert "nodata" not in plain and all("valid_pixels" not in r for r in plain["scenes"])
    assert json.load(open(d / "masked" / "summary.json"))["nodata"] == masked["nodata"]
    for a, rp, rm in zip(rasters, plain["scenes"], masked["scenes"]):
        valid = source_valid_host(a, 0)                       # identity tables: the grid's mask is the source's
        fp, fm = _files(rp), _files(rm)
        np.testing.assert_array_equal(read_tiff(rm["valid"]), valid)
        v = valid == 1
        for name in ("class", "margin"):
            np.testing.assert_array_equal(fm[name][v], fp[name][v])
            assert (fm[name][~v] == (127 if name == "class" else 0)).all()
        np.testing.assert_array_equal(fm["probs"][:, v], fp["probs"][:, v])
        assert not fm["probs"][:, ~v].any()
        kept_p, kept_m = plain["probabilities"][rp["output"]], masked["probabilities"][rm["output"]]
        np.testing.assert_array_equal(kept_m[v], kept_p[v])
        assert not kept_m[~v].any()
        assert rm["class_pixels"] == np.bincount(kept_p.argmax(-1)[v], minlength=3).tolist()
        assert rm["valid_pixels"] == int(valid.sum()) == sum(rm["class_pixels"])
        assert (rm["crops"], rm["skipped_crops"], rm["nodata"]) == (12, 0, 0.0)
        assert read_geotiff_tags(rm["output"])[42113].rstrip("\x00") == "127" and 42113 not in read_geotiff_tags(rp["output"])
    assert masked["scenes"][0]["valid_pixels"] < 100 * 150 - 3 and masked["scenes"][1]["valid_pixels"] == 100 * 150
    full_p, full_m = _files(plain["scenes"][1]), _files(masked["scenes"][1])  # the scene without fill: identical rasters
    for name in full_p:
        np.testing.assert_array_equal(full_m[name], full_p[name])


def test_infer_with_nodata_sieve_freezes_the_fill(trained, wedge_runs):
    ckpt, cfg = trained
    rasters, paths, plain, masked, d = wedge_runs
    sieved = I.infer(ckpt, paths, str(d / "sieved"), cfg=cfg, nodata=0, skip_empty=False, sieve=4, **SAME)
    for rm, rs in zip(masked["scenes"], sieved["scenes"]):
        want, stats = sieve_host(read_tiff(rm["output"]), 4, frozen_value=127)
        np.testing.assert_array_equal(read_tiff(rs["output"]), want)
        assert [rs["sieve"]["merged_components"], rs["sieve"]["changed_pixels"]] == stats.tolist()
        assert rs["class_pixels"] == rm["class_pixels"]


SKIP = dict(stride=64, batch_size=4, keep_probabilities=True, write_valid=True, nodata=0)


def test_infer_skips_the_crops_without_a_valid_pixel(trained, tmp_path):
    """Against the run that forwards every crop.  The two runs batch the crops differently, and the forward's bits are not
    pinned across batch compositions: canvases within atol = 1e-4 and class maps equal where top-1 minus top-2 exceeds 1e-4,
    the tolerance and the "decided" rule of test_infer_end_to_end_against_oracle.  Measured on an MI355X (the figures this
    test prints): maximum canvas difference on valid pixels 0, undecided pixels 0 of 12,288."""
    ckpt, cfg = trained
    a = _s1((128, 192), 31)
    a[:, :, 96:] = 0
    paths = _write(str(tmp_path), [a])
    boxes = I.crop_boxes(128, 192, 64, 64, 64)
    assert len(boxes) == 6 and sum(b[1] == 128 for b in boxes) == 2
    every = I.infer(ckpt, paths, str(tmp_path / "every"), cfg=cfg, skip_empty=False, **SKIP)
    skip = I.infer(ckpt, paths, str(tmp_path / "skip"), cfg=cfg, **SKIP)
    assert (every["n_crops"], every["nodata"]["skipped_crops"]) == (6, 0)
    assert (skip["n_crops"], skip["nodata"]["skipped_crops"], skip["scenes"][0]["crops"]) == (4, 2, 4)
    valid = source_valid_host(a, 0)
    v = valid == 1
    assert valid[:, :96].all() and not valid[:, 96:].any()
    re, rs = every["scenes"][0], skip["scenes"][0]
    for r in (re, rs):
        np.testing.assert_array_equal(read_tiff(r["valid"]), valid)
        assert (read_tiff(r["output"])[~v] == 127).all() and r["valid_pixels"] == 128 * 96 == sum(r["class_pixels"])
    pe, ps = every["probabilities"][re["output"]], skip["probabilities"][rs["output"]]
    srt = np.sort(pe, axis=-1)
    decided = ((srt[..., -1] - srt[..., -2]) > 1e-4) & v
    undecided = int(v.sum() - decided.sum())
    print(f"max |canvas difference| on valid pixels {np.abs(ps[v] - pe[v]).max():.3e}; "
          f"undecided {undecided} of {int(v.sum())}")
    assert undecided <= 0.01 * v.sum()
    np.testing.assert_allclose(ps[v], pe[v], rtol=0, atol=1e-4)
    assert not ps[~v].any() and not pe[~v].any()
    np.testing.assert_array_equal(read_tiff(rs["output"])[decided], read_tiff(re["output"])[decided])


def test_an_all_fill_scene_between_two_normal_ones(trained, tmp_path):
    ckpt, cfg = trained
    rasters = [_s1((100, 150), 41), np.zeros((2, 70, 90), dtype=np.float32), _s1((64, 64), 42)]
    paths = _write(str(tmp_path), rasters)
    kw = dict(stride=32, batch_size=4, nodata="auto", write_probs="u8", write_margin=True, sieve=4)
    out = I.infer(ckpt, paths, str(tmp_path / "three"), cfg=cfg, **kw)
    two = I.infer(ckpt, [paths[0], paths[2]], str(tmp_path / "two"), cfg=cfg, **kw)
    assert [r["input"] for r in out["scenes"]] == paths and out["n_scenes"] == 3      # three outputs, in order
    mid = out["scenes"][1]
    assert (mid["crops"], mid["valid_pixels"], mid["class_pixels"], mid["nodata"]) == (0, 0, [0, 0, 0], 0.0)
    assert mid["skipped_crops"] == len(I.crop_boxes(70, 90, 64, 64, 32)) == out["nodata"]["skipped_crops"]
    files = _files(mid)
    assert files["class"].shape == (70, 90) and (files["class"] == 127).all()
    assert not files["probs"].any() and files["probs"].shape == (3, 70, 90) and not files["margin"].any()
    assert read_geotiff_tags(mid["output"])[42113].rstrip("\x00") == "127"
    assert out["max_resident_scenes"] == two["max_resident_scenes"] and out["n_crops"] == two["n_crops"] == 12 + 4
    for r3, r2 in zip([out["scenes"][0], out["scenes"][2]], two["scenes"]):
        assert r3["class_pixels"] == r2["class_pixels"] and r3["crops"] == r2["crops"]
