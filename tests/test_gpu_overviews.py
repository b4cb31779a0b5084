"""GPU: fu_map_overviews (overviews.overviews_on_device) against the numpy statement overviews_host, bit for bit, for every
kind over shapes with odd sizes, partial edge tiles and a second launch; rejected calls leave dst untouched; infer with
--out_cog / --out_overviews writes files whose every image is the statement's level of the file's own first image."""
import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd import infer as I
from floodplanet_code_amd.datasets import geotiff as G
from floodplanet_code_amd.datasets import overviews as OV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
# 3 x 600: ten levels, so a second launch behind the first six; a partial edge tile; odd sizes in the cascade (75 -> 38,
# 19 -> 10).  130 x 200: several tiles in both directions.
SHAPES = [(1, 2), (2, 1), (3, 3), (65, 63), (67, 129), (130, 200), (3, 600)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.dtype(f"u{a.dtype.itemsize}"))


def make_raster(kind, k, H, W, seed=0):
    g = np.random.default_rng(seed + 1000 * H + 10 * W + k)
    shape = (H, W) if k == 1 else (k, H, W)
    if kind == "mode_u8":
        return g.choice(np.array([0, 127, 255], dtype=np.uint8), size=shape)      # ties and nodata both occur
    if kind == "mean_u8":
        return g.integers(0, 256, shape, dtype=np.uint8)
    if kind == "any_u8":
        return (g.random(shape) > 0.8).astype(np.uint8) * g.integers(1, 256, shape, dtype=np.uint8)
    # fp32: magnitudes far apart, so the order of the adds shows in the bits
    return (g.standard_normal(shape) * 10.0 ** g.integers(-3, 8, shape)).astype(np.float32)


def make_mask(H, W, seed=0):
    """Random, with 4 x 4 holes: blocks that are all invalid at level 1 and at level 2, next to ones that are not."""
    g = np.random.default_rng(seed + 7 * H + W)
    m = (g.random((H, W)) > 0.4).astype(np.uint8)
    holes = g.random((-(-H // 4), -(-W // 4))) > 0.6
    m[np.kron(holes, np.ones((4, 4), dtype=bool))[:H, :W]] = 0
    m[:2, :2] = 0                                                       # all invalid at level 1 ...
    if H > 2 and W > 2:
        m[2, 2] = 1                                                     # ... but not at level 2
    return m


def same(got, want):
    assert len(got) == len(want)
    for l, (g, w) in enumerate(zip(got, want), 1):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(bits(g), bits(w)), l


@pytest.mark.parametrize("kind", list(OV.KINDS))
def test_levels_equal_the_host_statement(kind):
    jobs = []
    for H, W in SHAPES:
        n = OV.max_levels(H, W)
        for k in (1, 3):
            a = make_raster(kind, k, H, W)
            variants = [dict()]
            if kind == "mode_u8":
                variants.append(dict(nodata_value=127))
            if kind in ("mean_u8", "mean_f32"):
                variants.append(dict(valid=make_mask(H, W)))
            for kw in variants:
                dev_kw = {key: torch.from_numpy(v).to(DEV) if key == "valid" else v for key, v in kw.items()}
                jobs.append((OV.overviews_on_device(torch.from_numpy(a).to(DEV), kind, n, **dev_kw), a, n, kw, (H, W, k)))
    torch.cuda.synchronize()
    for got, a, n, kw, case in jobs:
        want = OV.overviews_host(a, kind, n, **kw)
        if kind in ("mean_u8", "mean_f32"):
            same(got[0], want[0])
            assert (got[1] is None) == (want[1] is None) == ("valid" not in kw), case
            if want[1] is not None:
                same(got[1], want[1])
        else:
            same(got, want)
        assert len(want[0] if isinstance(want, tuple) else want) == n, case
    if kind in ("mean_u8", "mean_f32"):                                 # the hole pattern did what it is there for
        _, masks = OV.overviews_host(make_raster(kind, 1, 67, 129), kind, 2, valid=make_mask(67, 129))
        assert masks[0][0, 0] == 0 and masks[1][0, 0] == 1 and not masks[0].all() and masks[0].any()


@pytest.mark.parametrize("kind", ["mean_u8", "mean_f32", "mode_u8"])
def test_a_canvas_through_its_strides_gives_the_tensors_levels(kind):
    H, W, k = 67, 129, 3
    a = make_raster(kind, k, H, W, seed=3)
    khw = torch.from_numpy(a).to(DEV)
    canvas = torch.from_numpy(np.ascontiguousarray(a.transpose(1, 2, 0))).to(DEV)          # [H, W, k]
    view = canvas.permute(2, 0, 1)
    assert tuple(view.stride()) == (1, W * k, k)
    kw = dict(valid=torch.from_numpy(make_mask(H, W)).to(DEV)) if kind != "mode_u8" else dict(nodata_value=127)
    one, two = OV.overviews_on_device(khw, kind, 4, **kw), OV.overviews_on_device(view, kind, 4, **kw)
    padded = torch.zeros(k, H, W + 5, dtype=khw.dtype, device=DEV)      # rows that start off the 16-byte grid
    padded[:, :, :W] = khw
    three = OV.overviews_on_device(padded[:, :, :W], kind, 4, **kw)
    host_kw = {key: v.cpu().numpy() if key == "valid" else v for key, v in kw.items()}
    want = OV.overviews_host(a, kind, 4, **host_kw)
    if kind != "mode_u8":
        one, two, three, want = one[0], two[0], three[0], want[0]
    for got in (one, two, three):
        same(got, want)
    flat = OV.overviews_on_device(khw[0], kind, 2, **kw)                # [H, W] in: [h, w] levels out
    same(flat if kind == "mode_u8" else flat[0], [x[0] for x in want[:2]])


def test_bad_calls_are_rejected_and_leave_dst_untouched():
    lib = _lib.load()
    H, W, k, n = 17, 33, 3, 3
    a = make_raster("mean_u8", k, H, W)
    t = torch.from_numpy(a).to(DEV)
    valid = torch.from_numpy(make_mask(H, W)).to(DEV)
    pixels = sum(h * w for h, w in OV.overview_sizes(H, W, n))
    dst = torch.full((k * pixels + 64,), FILL, dtype=torch.uint8, device=DEV)
    vdst = torch.full((pixels + 64,), FILL, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(src=t.data_ptr(), strides=(H * W, W, 1), bands=k, h=H, w=W, kind=OV.KINDS["mean_u8"], mask=valid.data_ptr(),
             nodata=-1, levels=n, out=dst.data_ptr(), elems=k * pixels, mask_out=vdst.data_ptr()):
        return lib.fu_map_overviews(src, *strides, bands, h, w, kind, mask, nodata, levels, out, elems, mask_out, stream)

    cases = [(dict(out=None), "null"), (dict(src=None), "null"), (dict(elems=k * pixels - 1), "the levels hold"),
             (dict(mask_out=None), "go together"), (dict(mask=None), "go together"), (dict(bands=0), "bands"),
             (dict(bands=17), "bands"), (dict(kind=4), "unknown kind"), (dict(kind=-1), "unknown kind"),
             (dict(h=0), "empty"), (dict(strides=(-1, W, 1)), "negative"), (dict(levels=-1), "n_levels"),
             (dict(levels=7), "n_levels"), (dict(nodata=127), "only mode_u8"),
             (dict(kind=OV.KINDS["any_u8"]), "only the mean kinds"), (dict(kind=OV.KINDS["mode_u8"]), "only the mean kinds"),
             (dict(kind=OV.KINDS["mode_u8"], mask=None, mask_out=None, nodata=256), "nodata_value"),
             (dict(kind=OV.KINDS["mean_f32"], out=dst.data_ptr() + 1), "misaligned")]
    for kw, msg in cases:
        assert call(**kw) == _lib.FU_ERR_INVALID and msg.encode() in lib.fu_last_error(), msg
    assert call(levels=0) == _lib.FU_OK and call(levels=0, elems=0) == _lib.FU_OK      # nothing to do: no launch
    torch.cuda.synchronize()
    assert bool((dst == FILL).all()) and bool((vdst == FILL).all())     # nothing ran
    with pytest.raises(ValueError, match="uint8"):
        OV.overviews_on_device(t.to(torch.int32), "mean_u8", 1)
    with pytest.raises(ValueError, match="valid must be"):
        OV.overviews_on_device(t, "mean_u8", 1, valid=valid[:4])
    assert OV.overviews_on_device(t, "any_u8", 0) == [] and OV.overviews_on_device(t, "mean_u8", 0, valid=valid) == ([], [])
    assert call() == _lib.FU_OK
    torch.cuda.synchronize()
    want, masks = OV.overviews_host(a, "mean_u8", n, valid=valid.cpu().numpy())
    assert np.array_equal(dst[:k * pixels].cpu().numpy(), np.concatenate([x.reshape(-1) for x in want]))
    assert np.array_equal(vdst[:pixels].cpu().numpy(), np.concatenate([m.reshape(-1) for m in masks]))
    assert bool((dst[k * pixels:] == FILL).all()) and bool((vdst[pixels:] == FILL).all())


# --------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """The recipe of test_gpu_geotiff_write's fixture: a one-epoch checkpoint of a 2-channel S1 model."""
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


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """96 x 80, georeferenced, with a corner of fill; and a scene that is all fill."""
    from floodplanet_code_amd.datasets.synthetic import write_strip_tiff
    d = tmp_path_factory.mktemp("scenes")
    g = np.random.default_rng(22)
    a = (g.random((2, 96, 80), dtype=np.float32) * 70 - 50).astype(np.float32)
    a[:, :30, :25] = 0
    write_strip_tiff(str(d / "Scenes" / "S_00.tif"), a, rows_per_strip=7, extra_tags=GEO)
    write_strip_tiff(str(d / "Scenes" / "S_01.tif"), np.zeros((2, 40, 50), dtype=np.float32), extra_tags=GEO)
    return str(d / "Scenes"), d


GEO = [(33550, 12, [10.0, 10.0, 0.0]), (33922, 12, [0.0, 0.0, 0.0, 500000.0, 4000000.0, 0.0]),
       (34735, 3, [1, 1, 0, 1, 1024, 0, 1, 1])]
SIDE = dict(stride=32, batch_size=4, write_margin=True, nodata="0", write_valid=True, sieve=4)
FILES = {"output": "mode_u8", "margin": "mean_u8", "valid": "any_u8", "probabilities": None}


def check_files(rec, probs, n_levels):
    """Every image of every file of a record is the statement's level of the file's own first image."""
    valid = G.read_raster(rec["valid"])
    for key, kind in FILES.items():
        kind = kind or ("mean_u8" if probs == "u8" else "mean_f32")
        base = G.read_raster(rec[key])
        assert G.raster_ifds(rec[key]) == n_levels + 1, key
        if kind == "mode_u8":
            want = OV.overviews_host(base, kind, n_levels, nodata_value=127)
        elif kind == "any_u8":
            want = OV.overviews_host(base, kind, n_levels)
        else:
            want = OV.overviews_host(base, kind, n_levels, valid=valid)[0]
        for i, level in enumerate(want, 1):
            got = G.read_raster(rec[key], ifd=i)
            assert got.shape == level.shape and got.dtype == level.dtype and np.array_equal(bits(got), bits(level)), (key, i)
            assert (33550 in G._parse_ifd(G._map(rec[key]), keep=(33550,), ifd=i)[2]) is False
    for i in range(n_levels + 1):                                       # GDAL_NODATA on every IFD of the class map
        assert G._parse_ifd(G._map(rec["output"]), keep=(42113,), ifd=i)[2][42113] == "127"


def test_infer_with_out_cog_writes_the_statements_levels(trained, scenes):
    ckpt, cfg = trained
    src, d = scenes
    out = I.infer(ckpt, [src], str(d / "cog"), cfg=cfg, write_probs="u8", out_cog=True, out_tile=16, out_compress="deflate",
                  **SIDE)
    assert out["output_format"]["cog"] is True and out["output_format"]["overviews"] == 3 and out["output_format"]["tile"] == 16
    for rec, hw in zip(out["scenes"], ((96, 80), (40, 50))):
        n = OV.auto_levels(hw[0], hw[1], 16)
        assert rec["output_format"]["cog"] is True and rec["output_format"]["overviews"] == n == {96: 3, 40: 2}[hw[0]]
        check_files(rec, "u8", n)
        for key in FILES:
            assert G.cog_report(rec[key]) == [], key
            info = G.raster_info(rec[key], ifd=n)
            assert info["tiled"] and info["compression"] == 8 and max(info["height"], info["width"]) <= 16
    first = out["scenes"][0]
    assert 0 < first["valid_pixels"] < 96 * 80 and "sieve" in first
    assert (G.read_raster(first["output"]) == 127).any() and (G.read_raster(first["output"], ifd=1) == 127).any()


def test_infer_fp32_levels_bit_for_bit_and_the_untouched_default(trained, scenes):
    ckpt, cfg = trained
    src, d = scenes
    two = I.infer(ckpt, [src], str(d / "two"), cfg=cfg, write_probs="f32", out_overviews=2, **SIDE)
    assert two["output_format"]["overviews"] == 2 and two["output_format"]["cog"] is False
    for rec in two["scenes"]:
        assert rec["output_format"]["overviews"] == 2 and rec["output_format"]["cog"] is False
        check_files(rec, "f32", 2)
        assert not G.raster_info(rec["probabilities"], ifd=2)["tiled"] and G.raster_info(rec["probabilities"])["dtype"] == "float32"
    # only --out_compress deflate: one image per file, and the bytes of the same run with the pyramid's data taken off
    plain = I.infer(ckpt, [src], str(d / "plain"), cfg=cfg, write_probs="f32", out_compress="deflate", **SIDE)
    with_levels = I.infer(ckpt, [src], str(d / "with"), cfg=cfg, write_probs="f32", out_compress="deflate", out_overviews=0,
                          **SIDE)
    assert "overviews" not in plain["output_format"] and with_levels["output_format"]["overviews"] == 0
    for a, b in zip(plain["scenes"], with_levels["scenes"]):
        assert "overviews" not in a["output_format"]
        for key in FILES:
            assert G.raster_ifds(a[key]) == 1 == G.raster_ifds(b[key])
            assert open(a[key], "rb").read() == open(b[key], "rb").read(), key
    for a, b in zip(plain["scenes"], two["scenes"]):                    # and the first images of the pyramid run are those
        for key in FILES:
            assert np.array_equal(bits(G.read_raster(a[key])), bits(G.read_raster(b[key]))), key
