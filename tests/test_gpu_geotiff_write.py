"""GPU: fu_tiff_pack (geotiff_write.pack_on_device) against the numpy statement pack_host, byte for byte, over the grid of
the CPU round trip plus a strip row longer than one workgroup pass; rejected calls leave dst untouched; infer with the
out_* options writes files that decode to exactly what the default route writes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_geotiff_write_cpu import DTYPES, bits, grid, make_array, make_layout, predictors  # noqa: E402

from floodplanet_code_amd import _lib  # noqa: E402
from floodplanet_code_amd import infer as I  # noqa: E402
from floodplanet_code_amd.datasets import geotiff as G  # noqa: E402
from floodplanet_code_amd.datasets import geotiff_write as GW  # noqa: E402
from floodplanet_code_amd.datasets.tiff import read_tiff  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5


def _to_device(a, source):
    """make_array's array on the device with make_array's memory order (the strides are what is under test)."""
    k = 1 if a.ndim == 2 else a.shape[0]
    a3 = a if a.ndim == 3 else a[None]
    H, W = a3.shape[1:]
    if source == "hwk":
        t = torch.from_numpy(np.ascontiguousarray(a3.transpose(1, 2, 0))).to(DEV).permute(2, 0, 1)
    elif source == "padded":
        wide = np.zeros((k, H, W + 5), dtype=a.dtype)
        wide[:, :, :W] = a3
        t = torch.from_numpy(wide).to(DEV)[:, :, :W]
    else:
        t = torch.from_numpy(np.ascontiguousarray(a3)).to(DEV)
    assert tuple(t.stride()) == tuple(s // a.dtype.itemsize for s in a3.strides) or 1 in a3.shape
    return t if a.ndim == 3 else t[0]


def _pack_prefilled(t, L):
    """fu_tiff_pack into a dst pre-filled with 0xA5 -> (status, dst on the host)."""
    total = GW.check_pack_layout(L)
    dst = torch.full((total,), FILL, dtype=torch.uint8, device=DEV)
    t3 = t if t.dim() == 3 else t[None]
    st = _lib.load().fu_tiff_pack(t3.data_ptr(), *[int(s) for s in t3.stride()], G.layout_struct(L), dst.data_ptr(), total,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, dst.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_on_device_equals_the_host_statement(dtype):
    cases = list(grid(dtype)) + [(k, 9, 700, (0, rows, None), p, "khw") for k in (1, 3) for rows in (1, 16)
                                 for p in predictors(dtype)]       # a strip row longer than one workgroup pass
    cases += [(3, 33, 704, (0, 16, None), p, "hwk") for p in predictors(dtype)]   # ... and one that is whole groups
    got = []
    for k, H, W, seg, p, source in cases:
        a = make_array(dtype, k, H, W, source)
        L = make_layout(dtype, k, H, W, seg, p)
        got.append((GW.pack_on_device(_to_device(a, source), L), a, L, (k, H, W, seg, p, source)))
    torch.cuda.synchronize()
    for packed, a, L, case in got:
        want = GW.pack_host(a, L)
        assert packed.dtype == torch.uint8 and tuple(packed.shape) == want.shape, case
        assert np.array_equal(packed.cpu().numpy(), want), case


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_byte_of_dst_is_written(dtype):
    """From a dst that held 0xA5 everywhere the buffer equals pack_host's everywhere, also where a tile is all padding and
    where the last 16-byte group is short."""
    for k, H, W, seg, p in ((1, 5, 3, (1, 16, 16), 1), (3, 17, 33, (1, 32, 16), predictors(dtype)[1]),
                            (1, 1, 1, (0, 1, None), predictors(dtype)[1]), (3, 40, 70, (0, 7, None), predictors(dtype)[1]),
                            (1, 17, 33, (0, 16, None), 1)):
        a = make_array(dtype, k, H, W)
        L = make_layout(dtype, k, H, W, seg, p)
        st, dst = _pack_prefilled(_to_device(a, "khw"), L)
        assert st == _lib.FU_OK
        assert np.array_equal(dst, GW.pack_host(a, L)), (k, H, W, seg, p)
        back = G.unpack_on_device(dst, L, list(range(k)), DEV) if dtype == "u1" else None
        if back is not None:                                         # and fu_tiff_unpack takes it back
            assert np.array_equal(back.cpu().numpy(), np.float32(a if k > 1 else a[None]))


def test_bad_calls_are_rejected_and_leave_dst_untouched():
    lib = _lib.load()
    a = make_array("u1", 3, 17, 33)
    t = _to_device(a, "khw")
    good = make_layout("u1", 3, 17, 33, (1, 16, 16), 2)
    total = GW.check_pack_layout(good)
    dst = torch.full((total + 64,), FILL, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(layout, n_bytes=total, src=t.data_ptr(), out=dst.data_ptr(), strides=None):
        strides = [int(s) for s in t.stride()] if strides is None else strides
        return lib.fu_tiff_pack(src, *strides, G.layout_struct(layout), out, n_bytes, stream)

    cases = [(dict(n_bytes=total - 1), "the layout holds"), (dict(n_bytes=total + 16), "the layout holds"),
             (dict(layout=dict(good, predictor=3)), "predictor 3"), (dict(layout=dict(good, planar=0)), "chunky"),
             (dict(layout=dict(good, big_endian=1)), "big-endian"), (dict(layout=dict(good, seg_w=24)), "multiples of 16"),
             (dict(layout=dict(good, tiled=0)), "as wide as"), (dict(layout=dict(good, bytes_per_sample=8)), "bytes_per_sample"),
             (dict(layout=dict(good, samples=17)), "samples"), (dict(layout=dict(good, width=0)), "empty"),
             (dict(layout=dict(good, sample_kind=3)), "float"), (dict(src=None), "null"), (dict(out=None), "null"),
             (dict(out=dst.data_ptr() + 1), "misaligned"), (dict(strides=[-1, 33, 1]), "negative")]
    for kw, msg in cases:
        kw = dict(kw)
        layout = kw.pop("layout", good)
        assert call(layout, **kw) == _lib.FU_ERR_INVALID and msg.encode() in lib.fu_last_error(), msg
    f = torch.zeros(4, 4, device=DEV)
    L2 = GW.raster_layout("f4", 4, 4, predictor=2)
    assert lib.fu_tiff_pack(f.data_ptr(), 16, 4, 1, G.layout_struct(L2), dst.data_ptr(), 64, stream) == _lib.FU_ERR_INVALID
    assert b"predictor 2" in lib.fu_last_error()
    torch.cuda.synchronize()
    assert bool((dst == FILL).all())                                 # nothing ran
    for bad, exc in ((dict(good, predictor=3), ValueError), (dict(good, planar=0), ValueError)):
        with pytest.raises(exc):
            GW.pack_on_device(t, bad)
    with pytest.raises(ValueError, match="layout describes"):
        GW.pack_on_device(t.to(torch.int32), good)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        GW.pack_on_device(t.cpu(), good)
    assert call(good) == _lib.FU_OK
    torch.cuda.synchronize()
    assert np.array_equal(dst[:total].cpu().numpy(), GW.pack_host(a, good)) and bool((dst[total:] == FILL).all())


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


GEO = [(33550, 12, [10.0, 10.0, 0.0]), (33922, 12, [0.0, 0.0, 0.0, 500000.0, 4000000.0, 0.0]),
       (34735, 3, [1, 1, 0, 1, 1024, 0, 1, 1])]


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """100 x 90 (no multiple of the 16-pixel tile), georeferenced, with a corner of fill; and a scene that is all fill."""
    from floodplanet_code_amd.datasets.synthetic import write_strip_tiff
    d = tmp_path_factory.mktemp("scenes")
    g = np.random.default_rng(21)
    a = (g.random((2, 100, 90), dtype=np.float32) * 70 - 50).astype(np.float32)
    a[:, :30, :25] = 0
    write_strip_tiff(str(d / "Scenes" / "S_00.tif"), a, rows_per_strip=7, extra_tags=GEO)
    write_strip_tiff(str(d / "Scenes" / "S_01.tif"), np.zeros((2, 40, 50), dtype=np.float32), extra_tags=GEO)
    return str(d / "Scenes"), d


FILES = ("output", "margin", "valid", "probabilities")
SIDE = dict(stride=32, batch_size=4, write_margin=True, nodata="auto", write_valid=True)
_runs = {}


def _run(trained, scenes, probs, **out_kw):
    key = (probs,) + tuple(sorted(out_kw.items()))
    if key not in _runs:
        ckpt, cfg = trained
        src, d = scenes
        out_dir = str(d / ("run_" + "_".join(str(v) for v in key)))
        _runs[key] = I.infer(ckpt, [src], out_dir, cfg=cfg, write_probs=probs, **SIDE, **out_kw)
    return _runs[key]


@pytest.mark.parametrize("probs", ["u8", "f32"])
def test_infer_with_out_options_decodes_to_the_default_routes_files(trained, scenes, probs):
    plain = _run(trained, scenes, probs)
    packed = _run(trained, scenes, probs, out_compress="deflate", out_tile=16)
    assert "output_format" not in plain and all("output_format" not in r for r in plain["scenes"])
    assert packed["output_format"] == {"compress": "deflate", "level": 6, "predictor": "auto", "tile": 16, "bigtiff": False,
                                       "threads": 4}
    assert [r["crops"] for r in packed["scenes"]] == [r["crops"] for r in plain["scenes"]] and packed["scenes"][1]["crops"] == 0
    for a, b in zip(plain["scenes"], packed["scenes"]):
        assert b["output_format"]["bigtiff"] == {"class": False, "valid": False, "probabilities": False, "margin": False}
        assert {k: v for k, v in b.items() if k not in FILES + ("output_format",)} == \
            {k: v for k, v in a.items() if k not in FILES}
        for key in FILES:
            want, got = read_tiff(a[key]), G.read_raster(b[key])
            assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), key
            assert G.raster_geotiff_tags(b[key]) == G.raster_geotiff_tags(a[key]) and 33550 in G.raster_geotiff_tags(b[key])
            info = G.raster_info(b[key])
            assert info["tiled"] and (info["seg_h"], info["seg_w"]) == (16, 16) and info["compression"] == 8
            assert info["predictor"] == (3 if info["dtype"] == "float32" else 2) and not info["bigtiff"]
            assert not G.strict_reader_accepts(b[key])
        assert G.raster_geotiff_tags(b["output"])[42113] == "127" == G.raster_geotiff_tags(a["output"])[42113]
        assert 42113 not in G.raster_geotiff_tags(b["margin"])
        assert os.path.getsize(b["output"]) < os.path.getsize(a["output"])


def test_infer_with_forced_bigtiff_strips_and_vectors(trained, scenes):
    plain = _run(trained, scenes, "f32")
    big = _run(trained, scenes, "f32", out_bigtiff="yes", write_vectors=True)
    assert big["output_format"]["bigtiff"] is True and big["output_format"]["compress"] == "none"
    for a, b in zip(plain["scenes"], big["scenes"]):
        for key in FILES:
            info = G.raster_info(b[key])
            assert info["bigtiff"] and not info["tiled"] and info["compression"] == 1 and info["predictor"] == 1
            assert np.array_equal(bits(G.read_raster(b[key])), bits(read_tiff(a[key]))), key
            assert G.raster_geotiff_tags(b[key]) == G.raster_geotiff_tags(a[key])
        assert all(b["output_format"]["bigtiff"].values())
        assert os.path.exists(b["vectors"]["path"])                  # the raw class map rode along for the rings
    ckpt, cfg = trained
    src, d = scenes
    ref = I.infer(ckpt, [src], str(d / "vec_ref"), cfg=cfg, write_probs="f32", write_vectors=True, **SIDE)
    for a, b in zip(ref["scenes"], big["scenes"]):
        assert open(a["vectors"]["path"]).read() == open(b["vectors"]["path"]).read()
