"""GPU: fu_map_components / fu_map_sieve against the host statements of postprocess.py, bit for bit (integers: there is
nothing to tolerate), on maps chosen to break a tiled union-find rather than to resemble the workload; rejected calls;
infer with sieve= end to end."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd import postprocess as PP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------ the maps
def _spiral(H, W):
    """A one-pixel-wide rectangular spiral of 1s with one-pixel gaps: one component that winds through every tile."""
    m = np.zeros((H, W), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    moved = True
    while moved:
        moved = False
        for _ in range(2):                             # straight on, else one turn to the right
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < H and 0 <= nx < W and m[ny, nx] == 0 and not (0 <= ny2 < H and 0 <= nx2 < W and m[ny2, nx2]):
                y, x = ny, nx
                m[y, x] = 1
                moved = True
                break
            dy, dx = dx, -dy
    return m


def _serpentine(H, W):
    m = np.zeros((H, W), np.uint8)
    m[::2] = 1
    m[1::4, -1] = 1
    m[3::4, 0] = 1
    return m


def _comb(H, W):
    m = np.zeros((H, W), np.uint8)
    m[:, ::2] = 1
    m[-1] = 1                                           # the teeth join only along the last row
    return m


def _random(shape, seed, fill=0.5, n_values=2):
    g = np.random.default_rng(seed)
    if n_values == 2:
        return (g.random(shape) < fill).astype(np.uint8)
    return g.integers(0, n_values, shape).astype(np.uint8) * 40


MAPS = {
    "rand_1x1": lambda: _random((1, 1), 0),
    "rand_1x300": lambda: _random((1, 300), 1),
    "rand_300x1": lambda: _random((300, 1), 2),
    "rand_37x45": lambda: _random((37, 45), 3),
    "rand_70x53": lambda: _random((70, 53), 4),
    "rand_257x300": lambda: _random((257, 300), 5),
    "one_value_70x53": lambda: np.full((70, 53), 3, np.uint8),
    "one_value_257x300": lambda: np.full((257, 300), 255, np.uint8),
    "checkerboard_70x53": lambda: (np.indices((70, 53)).sum(0) % 2).astype(np.uint8),
    "spiral_129x131": lambda: _spiral(129, 131),
    "spiral_speckled_129x131": lambda: _spiral(129, 131) ^ _random((129, 131), 9, fill=0.02),   # cut into many arcs
    "serpentine_129x131": lambda: _serpentine(129, 131),
    "comb_70x53": lambda: _comb(70, 53),
    "comb_129x131": lambda: _comb(129, 131),
    "fill59_150x170": lambda: _random((150, 170), 6, fill=0.59),
    "fill41_150x170": lambda: _random((150, 170), 7, fill=0.41),
    "four_values_70x53": lambda: _random((70, 53), 8, n_values=4),
}


@functools.lru_cache(maxsize=None)
def host_map(name):
    m = MAPS[name]()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def host_labels(name, connectivity):
    out = PP.label_components_host(host_map(name), connectivity)
    out.setflags(write=False)
    return out


def dev_map(name):
    return torch.from_numpy(host_map(name).copy()).to(DEV)


# ------------------------------------------------------------------------------------------------------------ components
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_components_equal_the_host_statement(name, connectivity):
    want = host_labels(name, connectivity)
    got = PP.label_components(dev_map(name), connectivity)
    assert got.dtype == torch.int32 and got.device.type == "cuda"
    assert torch.equal(got.cpu(), torch.from_numpy(want.copy()))


def test_the_maps_are_what_they_are_meant_to_be():
    """The hard cases are hard: the checkerboard is all singletons under 4 and two components under 8; the spiral, the
    serpentine and the comb are one component of 1s that crosses tile seams."""
    cb = host_map("checkerboard_70x53")
    assert len(np.unique(host_labels("checkerboard_70x53", 4))) == cb.size
    assert len(np.unique(host_labels("checkerboard_70x53", 8))) == 2
    for name in ("spiral_129x131", "serpentine_129x131", "comb_129x131", "comb_70x53"):
        m, lab = host_map(name), host_labels(name, 4)
        assert len(np.unique(lab[m == 1])) == 1 and (m == 1).sum() > 1500, name
    assert len(np.unique(host_labels("one_value_70x53", 4))) == 1


# ------------------------------------------------------------------------------------------------------------ sieve
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_sieve_equals_the_host_statement(name, connectivity):
    m = host_map(name)
    md = dev_map(name)
    present = int(m.max())
    for min_pixels in (2, 5, 50):
        for frozen in (None, present):
            for passes in (1, 3):
                want, want_stats = PP.sieve_host(m, min_pixels, connectivity, frozen, passes)
                stats = torch.tensor([7, 11], dtype=torch.int64, device=DEV)           # the counts are ADDED
                out, stats2 = PP.sieve(md, min_pixels, connectivity, frozen, passes, stats=stats)
                case = (name, connectivity, min_pixels, frozen, passes)
                assert stats2 is stats and out.data_ptr() != md.data_ptr()
                assert torch.equal(out.cpu(), torch.from_numpy(want)), case
                assert torch.equal(stats.cpu(), torch.from_numpy(want_stats + np.array([7, 11]))), case
    assert torch.equal(md.cpu(), torch.from_numpy(m.copy()))                           # the input stays


@pytest.mark.parametrize("name", ["rand_257x300", "fill59_150x170", "four_values_70x53", "spiral_speckled_129x131"])
def test_in_place_equals_out_of_place_and_runs_repeat(name):
    md = dev_map(name)
    for connectivity, passes in ((4, 1), (8, 3)):
        a, sa = PP.sieve(md, 5, connectivity, passes=passes)
        b, sb = PP.sieve(md, 5, connectivity, passes=passes)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and torch.equal(sa, sb)     # two runs, the same bytes
        c = md.clone()
        c2, sc = PP.sieve(c, 5, connectivity, passes=passes, out=c)
        assert c2 is c and torch.equal(c, a) and torch.equal(sc, sa)
        assert int(sa[1]) > 0                           # something was sieved


def test_default_stats_start_at_zero_and_null_stats_are_allowed():
    name = "rand_70x53"
    m, md = host_map(name), dev_map(name)
    want, want_stats = PP.sieve_host(m, 5)
    out, stats = PP.sieve(md, 5)
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and stats.cpu().tolist() == want_stats.tolist()
    lib = _lib.load()
    H, W = m.shape
    ws = torch.empty(lib.fu_sieve_workspace_bytes(H, W), dtype=torch.uint8, device=DEV)
    out2 = torch.empty_like(md)
    _lib.check(lib.fu_map_sieve(md.data_ptr(), out2.data_ptr(), H, W, 4, 5, -1, 1, ws.data_ptr(), ws.numel(), None,
                                torch.cuda.current_stream().cuda_stream))
    assert torch.equal(out2, out)


@pytest.mark.parametrize("min_pixels", [0, 1])
def test_min_pixels_one_copies_the_map(min_pixels):
    md = dev_map("rand_257x300")
    stats = torch.tensor([7, 11], dtype=torch.int64, device=DEV)
    out, _ = PP.sieve(md, min_pixels, 8, passes=3, stats=stats)
    assert out.data_ptr() != md.data_ptr() and torch.equal(out, md) and stats.cpu().tolist() == [7, 11]
    same, _ = PP.sieve(md, min_pixels, out=md)
    assert same is md and torch.equal(md.cpu(), torch.from_numpy(host_map("rand_257x300").copy()))


# ------------------------------------------------------------------------------------------------------------ rejected calls
def test_rejected_calls_launch_nothing():
    lib = _lib.load()
    H, W = 40, 50
    md = dev_map("rand_70x53")[:H, :W].contiguous()
    out = torch.full((H, W), 0xAB, dtype=torch.uint8, device=DEV)
    labels = torch.full((H, W), -5, dtype=torch.int32, device=DEV)
    stats = torch.tensor([7, 11], dtype=torch.int64, device=DEV)
    nbytes = lib.fu_sieve_workspace_bytes(H, W)
    assert nbytes == 16 * H * W
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def sieve(map_=md.data_ptr(), out_=out.data_ptr(), h=H, w=W, conn=4, min_pixels=5, frozen=-1, passes=1,
              ws_=ws.data_ptr(), ws_bytes=nbytes, stats_=stats.data_ptr()):
        return lib.fu_map_sieve(map_, out_, h, w, conn, min_pixels, frozen, passes, ws_, ws_bytes, stats_, stream)

    bad = [dict(conn=6), dict(passes=0), dict(passes=9), dict(ws_bytes=nbytes - 1), dict(ws_=None), dict(map_=None),
           dict(out_=None), dict(h=1 << 15, w=1 << 14), dict(h=0), dict(w=-3), dict(frozen=256),
           dict(ws_=ws.data_ptr() + 4, ws_bytes=nbytes - 4)]
    for kw in bad:
        assert sieve(**kw) == _lib.FU_ERR_INVALID, kw
        assert b"fu_map_sieve" in lib.fu_last_error(), kw
    for kw in (dict(conn=6), dict(map_=None), dict(out_=None), dict(h=1 << 15, w=1 << 14), dict(h=0)):
        args = dict(map_=md.data_ptr(), out_=labels.data_ptr(), h=H, w=W, conn=4)
        args.update(kw)
        assert lib.fu_map_components(args["map_"], args["h"], args["w"], args["conn"], args["out_"],
                                     stream) == _lib.FU_ERR_INVALID, kw
        assert b"fu_map_components" in lib.fu_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()) and bool((labels == -5).all()) and stats.cpu().tolist() == [7, 11]
    assert sieve() == _lib.FU_OK                        # and the good call goes through
    want, want_stats = PP.sieve_host(md.cpu().numpy(), 5)
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and stats.cpu().tolist() == (want_stats + [7, 11]).tolist()
    for call, kw in ((PP.sieve, dict(min_pixels=5, connectivity=6)), (PP.sieve, dict(min_pixels=5, passes=9)),
                     (PP.sieve, dict(min_pixels=-1)), (PP.label_components, dict(connectivity=6))):
        with pytest.raises(ValueError):
            call(md, **kw)
    with pytest.raises(ValueError):
        PP.sieve(md.cpu(), 5)


# ------------------------------------------------------------------------------------------------------------ infer
@pytest.fixture(scope="module")
def tiny_checkpoint(tmp_path_factory):
    """A one-epoch checkpoint of a 2-channel S1 model at 32 x 32 crops.  ignore_index 2: the synthetic targets are {0, 1}, so
    the net learns both values of the written map (under ignore_index 0 it would only ever say 'water')."""
    from floodplanet_code_amd.fit import SyntheticTiles, fit_model
    exp = str(tmp_path_factory.mktemp("exp"))
    ch = {"ms_image": 2}
    cfg = dict(lr=1e-2, n_epochs=1, batch_size=8, save_topk_models=1, ignore_index=2, crop_height=32, crop_width=32,
               crop_stride=32, eval_region=["RegA"], n_workers=0,
               model=dict(name="ms_model", model_kwargs=dict(optimizer_name="adam", base_channels=8, precision="fp32")))
    ckpt = fit_model(cfg, SyntheticTiles(30, 8, ch, 32, 32, DEV, seed=1), SyntheticTiles(1, 8, ch, 32, 32, DEV, seed=2),
                     ch, 3, exp_dir=exp, device=DEV)
    return exp, ckpt


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_infer_with_sieve_end_to_end(tiny_checkpoint, tmp_path):
    from tools.tiff_writer import write_tiff
    from floodplanet_code_amd import infer as I
    from floodplanet_code_amd import predict as P
    from floodplanet_code_amd.datasets.tiff import read_tiff
    exp, ckpt = tiny_checkpoint
    cfg = P.resolve_cfg(exp, ckpt)
    g = np.random.default_rng(11)
    paths = []
    for i, (h, w) in enumerate([(70, 53), (33, 90)]):      # per-pixel noise in dB: the class map comes out speckled
        p = str(tmp_path / "Scenes" / f"S_{i:02d}.tif")
        write_tiff(p, (g.random((2, h, w), dtype=np.float32) * 70 - 50).astype(np.float32), planar=2, rows_per_strip=7)
        paths.append(p)
    common = dict(cfg=cfg, stride=16, batch_size=4, blend="hann", write_probs="u8", write_margin=True)
    plain = I.infer(ckpt, paths, str(tmp_path / "plain"), keep_probabilities=True, **common)
    N = 30
    sieved = I.infer(ckpt, paths, str(tmp_path / "sieved"), sieve=N, sieve_connectivity=8, sieve_passes=2, **common)
    assert "sieve" not in plain and all("sieve" not in r for r in plain["scenes"])
    assert "sieve" not in json.load(open(tmp_path / "plain" / "summary.json"))
    total = [0, 0]
    for a, b in zip(plain["scenes"], sieved["scenes"]):
        raw = read_tiff(a["output"])
        canvas = plain["probabilities"][a["output"]]
        np.testing.assert_array_equal(raw, (np.clip(canvas.argmax(-1), 0, 1) * 255).astype(np.uint8))   # as before
        want, want_stats = PP.sieve_host(raw, N, 8, None, 2)
        print(f"{os.path.basename(a['output'])}: water share {float((raw == 255).mean()):.3f}, components "
              f"{len(np.unique(PP.label_components_host(raw, 8)))}, sieve stats {want_stats.tolist()}")
        np.testing.assert_array_equal(read_tiff(b["output"]), want)
        assert b["sieve"] == {"min_pixels": N, "connectivity": 8, "passes": 2, "merged_components": int(want_stats[0]),
                              "changed_pixels": int(want_stats[1])}
        assert b["class_pixels"] == a["class_pixels"]   # what the network said, un-sieved
        for kind in ("probabilities", "margin"):
            assert _read(a[kind]) == _read(b[kind]), kind
        total[0] += int(want_stats[0])
        total[1] += int(want_stats[1])
    summary = json.load(open(tmp_path / "sieved" / "summary.json"))
    assert summary["sieve"] == {"min_pixels": N, "connectivity": 8, "passes": 2, "merged_components": total[0],
                                "changed_pixels": total[1]}
    assert [r["sieve"] for r in summary["scenes"]] == [r["sieve"] for r in sieved["scenes"]]
    assert total[1] > 0, "the scenes should hold something to sieve"
