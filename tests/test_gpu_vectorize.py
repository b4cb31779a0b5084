"""GPU: fu_map_edge_offsets / fu_map_edge_rings against the host statements of vectorize.py, bit for bit (integers: there
is nothing to tolerate), on maps chosen to break a tiled scan and the pointer doubling rather than to resemble the
workload; the capacity guard; rejected calls; infer with write_vectors= end to end."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd import postprocess as PP
from floodplanet_code_amd import vectorize as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = -0x5A5A5A5B


# ------------------------------------------------------------------------------------------------------------ the maps
def _spiral(H, W):
    """A one-pixel-wide rectangular spiral of 255 with one-pixel gaps: one ring that winds through the whole map."""
    m = np.zeros((H, W), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 255
    moved = True
    while moved:
        moved = False
        for _ in range(2):                             # straight on, else one turn to the right
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < H and 0 <= nx < W and m[ny, nx] == 0 and not (0 <= ny2 < H and 0 <= nx2 < W and m[ny2, nx2]):
                y, x = ny, nx
                m[y, x] = 255
                moved = True
                break
            dy, dx = dx, -dy
    return m


def _serpentine(H, W):
    m = np.zeros((H, W), np.uint8)
    m[::2] = 255
    m[1::4, -1] = 255
    m[3::4, 0] = 255
    return m


def _random(shape, seed, fill=0.5, n_values=2):
    g = np.random.default_rng(seed)
    if n_values == 2:
        return ((g.random(shape) < fill) * 255).astype(np.uint8)
    return (g.integers(0, n_values, shape) * 85).astype(np.uint8)      # 0, 85, 170, 255


MAPS = {
    "rand_1x1": lambda: np.full((1, 1), 255, np.uint8),
    "rand_1x300": lambda: _random((1, 300), 1),
    "rand_300x1": lambda: _random((300, 1), 2),
    "rand_37x45": lambda: _random((37, 45), 3),
    "rand_70x53": lambda: _random((70, 53), 4),
    "rand_257x300": lambda: _random((257, 300), 5),                  # several scan blocks, a multiple of no tile
    "one_value_70x53": lambda: np.full((70, 53), 255, np.uint8),      # one ring with 4 corners
    "checkerboard_70x53": lambda: ((np.indices((70, 53)).sum(0) % 2) * 255).astype(np.uint8),   # 4 edges per pixel
    "spiral_129x131": lambda: _spiral(129, 131),                     # one ring thousands of edges long: every round
    "serpentine_129x131": lambda: _serpentine(129, 131),             # of the doubling matters
    "four_values_70x53": lambda: _random((70, 53), 8, n_values=4),
}
SELECTS = {"all": np.ones(256, np.uint8), "255": V.select_flags([255]), "none": V.select_flags([])}


@functools.lru_cache(maxsize=None)
def host_map(name):
    m = MAPS[name]()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def host_offsets(name, select):
    return V.edge_offsets_host(host_map(name), SELECTS[select])


@functools.lru_cache(maxsize=None)
def host_rings(name, select, connectivity):
    return V.edge_rings_host(host_map(name), SELECTS[select], connectivity)


def dev_map(name):
    return torch.from_numpy(host_map(name).copy()).to(DEV)


def test_the_maps_are_what_they_are_meant_to_be():
    for name in ("spiral_129x131", "serpentine_129x131"):
        A = host_rings(name, "255", 4)
        assert A["start"].size > 8000 and len(np.unique(A["ring"])) == 1, name      # one ring: 13+ rounds of doubling
    assert len(np.unique(host_rings("one_value_70x53", "all", 4)["ring"])) == 1
    assert int((host_rings("one_value_70x53", "all", 4)["flags"] >> 2).sum()) == 4
    assert int(host_offsets("checkerboard_70x53", "all")[-1]) == 4 * 70 * 53
    assert 257 * 300 > 16 * 2048 and 257 * 300 % 2048 != 0                             # dozens of scan blocks, a ragged last one


# ------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("select", sorted(SELECTS))
@pytest.mark.parametrize("name", sorted(MAPS))
def test_edge_offsets_equal_the_host_statement(name, select):
    got = V.edge_offsets(dev_map(name), SELECTS[select])
    assert got.dtype == torch.int32 and got.device.type == "cuda"
    assert torch.equal(got.cpu(), torch.from_numpy(host_offsets(name, select).copy()))


def test_edge_offsets_carry_across_chunks_of_block_totals():
    """The totals of more than 256 scan blocks (2048 pixels each) are scanned in chunks with a carry: 600 x 900 has 264."""
    m = _random((600, 900), 12, fill=0.3)
    want = V.edge_offsets_host(m, SELECTS["all"])
    got = V.edge_offsets(torch.from_numpy(m).to(DEV), SELECTS["all"])
    assert torch.equal(got.cpu(), torch.from_numpy(want)) and int(want[-1]) > 500000


@pytest.mark.parametrize("select", sorted(SELECTS))
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_edge_rings_equal_the_host_statement(name, connectivity, select):
    want = host_rings(name, select, connectivity)
    got = V.edge_rings(dev_map(name), SELECTS[select], connectivity)
    assert sorted(got) == sorted(V.ARRAYS)
    for k in V.ARRAYS:
        assert got[k].dtype == torch.int32 and got[k].device.type == "cuda"
        assert np.array_equal(got[k].cpu().numpy(), want[k]), (name, connectivity, select, k)


def test_edge_rings_takes_labels_and_a_limit():
    name = "rand_70x53"
    md = dev_map(name)
    labels = PP.label_components(md, 8)
    got = V.edge_rings(md, SELECTS["all"], 8, labels=labels)
    for k in V.ARRAYS:
        assert np.array_equal(got[k].cpu().numpy(), host_rings(name, "all", 8)[k]), k
    n = int(host_offsets(name, "all")[-1])
    assert V.edge_rings(md, SELECTS["all"], 8, max_edges=n - 1) is None
    assert V.edge_rings(md, SELECTS["all"], 8, max_edges=n)["start"].numel() == n
    assert V.count_and_rings(md, SELECTS["all"], 8, max_edges=0) == (n, None)
    with pytest.raises(ValueError):
        V.edge_rings(md, SELECTS["all"], 5)
    with pytest.raises(ValueError):
        V.edge_rings(md, SELECTS["all"], 4, labels=labels.long())
    with pytest.raises(ValueError):
        V.edge_rings(md.cpu(), SELECTS["all"])


# ------------------------------------------------------------------------------------------------------------ raw calls
class Raw:
    """The two C calls on one map with poisoned outputs."""

    def __init__(self, name="rand_70x53", select="all", connectivity=4, capacity=None):
        self.lib = _lib.load()
        self.md = dev_map(name)
        self.H, self.W = self.md.shape
        self.select = V._select_bytes(SELECTS[select])
        self.connectivity = connectivity
        self.n = int(host_offsets(name, select)[-1])
        self.capacity = self.n if capacity is None else capacity
        self.labels = PP.label_components(self.md, connectivity)
        self.offsets = torch.full((self.H * self.W + 1,), POISON, dtype=torch.int32, device=DEV)
        self.out = {k: torch.full((max(self.capacity, 1),), POISON, dtype=torch.int32, device=DEV) for k in V.ARRAYS}
        self.ews_bytes = int(self.lib.fu_map_edges_workspace_bytes(self.H, self.W))
        self.rws_bytes = int(self.lib.fu_map_rings_workspace_bytes(max(self.capacity, 1)))
        self.ews = torch.empty(self.ews_bytes, dtype=torch.uint8, device=DEV)
        self.rws = torch.empty(self.rws_bytes, dtype=torch.uint8, device=DEV)
        self.stream = torch.cuda.current_stream().cuda_stream

    def edge_offsets(self, **kw):
        a = dict(map_=self.md.data_ptr(), h=self.H, w=self.W, select=self.select, out=self.offsets.data_ptr(),
                 ws=self.ews.data_ptr(), ws_bytes=self.ews_bytes)
        a.update(kw)
        return self.lib.fu_map_edge_offsets(a["map_"], a["h"], a["w"], a["select"], a["out"], a["ws"], a["ws_bytes"], self.stream)

    def edge_rings(self, **kw):
        a = dict(map_=self.md.data_ptr(), labels=self.labels.data_ptr(), h=self.H, w=self.W, select=self.select,
                 conn=self.connectivity, offsets=self.offsets.data_ptr(), capacity=self.capacity, ws=self.rws.data_ptr(),
                 ws_bytes=self.rws_bytes, **{k: self.out[k].data_ptr() for k in V.ARRAYS})
        a.update(kw)
        return self.lib.fu_map_edge_rings(a["map_"], a["labels"], a["h"], a["w"], a["select"], a["conn"], a["offsets"],
                                          a["capacity"], *(a[k] for k in V.ARRAYS), a["ws"], a["ws_bytes"], self.stream)

    def untouched(self, start=0):
        torch.cuda.synchronize()
        return all(bool((self.out[k][start:] == POISON).all()) for k in V.ARRAYS)


def test_workspace_sizes():
    lib = _lib.load()
    assert lib.fu_map_edges_workspace_bytes(1, 1) == 16 and lib.fu_map_edges_workspace_bytes(257, 300) == 160     # 38 + 1 ints
    assert lib.fu_map_edges_workspace_bytes(0, 5) == 0 and lib.fu_map_edges_workspace_bytes(1 << 15, 1 << 14) == 0
    assert lib.fu_map_rings_workspace_bytes(1) == 80 and lib.fu_map_rings_workspace_bytes(1000) == 20000
    assert lib.fu_map_rings_workspace_bytes(0) == 0 and lib.fu_map_rings_workspace_bytes(-1) == 0
    assert lib.fu_map_rings_workspace_bytes((1 << 30) + 1) == 0


def test_capacity_below_the_edge_count_writes_nothing():
    r = Raw()
    assert r.edge_offsets() == _lib.FU_OK
    r2 = Raw(capacity=r.n - 1)
    r2.offsets = r.offsets
    assert r2.edge_rings() == _lib.FU_OK and r2.untouched()


def test_capacity_above_the_edge_count_leaves_the_tail_untouched():
    r = Raw(connectivity=8)
    r = Raw(connectivity=8, capacity=r.n + 1000)
    assert r.edge_offsets() == _lib.FU_OK and r.edge_rings() == _lib.FU_OK
    assert r.untouched(start=r.n)
    want = host_rings("rand_70x53", "all", 8)
    for k in V.ARRAYS:
        assert np.array_equal(r.out[k][:r.n].cpu().numpy(), want[k]), k


def test_capacity_zero_launches_nothing():
    r = Raw(select="none")
    assert r.n == 0 and r.edge_offsets() == _lib.FU_OK
    assert int(r.offsets[-1]) == 0 and r.edge_rings(capacity=0, ws=None, ws_bytes=0) == _lib.FU_OK and r.untouched()


def test_rejected_calls_launch_nothing():
    r = Raw()
    lib = r.lib
    bad = [dict(map_=None), dict(select=None), dict(out=None), dict(ws=None), dict(h=1 << 15, w=1 << 14), dict(h=0), dict(w=-3),
           dict(ws_bytes=r.ews_bytes - 1), dict(ws=r.ews.data_ptr() + 4)]
    for kw in bad:
        assert r.edge_offsets(**kw) == _lib.FU_ERR_INVALID, kw
        assert b"fu_map_edge_offsets" in lib.fu_last_error(), kw
    torch.cuda.synchronize()
    assert bool((r.offsets == POISON).all())
    assert r.edge_offsets() == _lib.FU_OK
    bad = [dict(map_=None), dict(labels=None), dict(select=None), dict(offsets=None), dict(start=None), dict(comp=None),
           dict(ring=None), dict(rank=None), dict(flags=None), dict(ws=None), dict(h=1 << 15, w=1 << 14), dict(h=0), dict(conn=5),
           dict(capacity=-1), dict(capacity=(1 << 30) + 1), dict(ws_bytes=r.rws_bytes - 1), dict(ws=r.rws.data_ptr() + 4)]
    for kw in bad:
        assert r.edge_rings(**kw) == _lib.FU_ERR_INVALID, kw
        assert b"fu_map_edge_rings" in lib.fu_last_error(), kw
    assert r.untouched()
    assert r.edge_rings() == _lib.FU_OK                 # and the good call goes through
    torch.cuda.synchronize()
    for k in V.ARRAYS:
        assert np.array_equal(r.out[k].cpu().numpy(), host_rings("rand_70x53", "all", 4)[k]), k


# ------------------------------------------------------------------------------------------------------------ infer
@pytest.fixture(scope="module")
def tiny_checkpoint(tmp_path_factory):
    """test_gpu_sieve's: a one-epoch checkpoint of a 2-channel S1 model at 32 x 32 crops that says both classes."""
    from floodplanet_code_amd.fit import SyntheticTiles, fit_model
    exp = str(tmp_path_factory.mktemp("exp"))
    ch = {"ms_image": 2}
    cfg = dict(lr=1e-2, n_epochs=1, batch_size=8, save_topk_models=1, ignore_index=2, crop_height=32, crop_width=32,
               crop_stride=32, eval_region=["RegA"], n_workers=0,
               model=dict(name="ms_model", model_kwargs=dict(optimizer_name="adam", base_channels=8, precision="fp32")))
    ckpt = fit_model(cfg, SyntheticTiles(30, 8, ch, 32, 32, DEV, seed=1), SyntheticTiles(1, 8, ch, 32, 32, DEV, seed=2),
                     ch, 3, exp_dir=exp, device=DEV)
    return exp, ckpt


GEO = [(33550, 12, [8.0, 8.0, 0.0]), (33922, 12, [0.0, 0.0, 0.0, 500000.0, 4100000.0, 0.0]),
       (34735, 3, [1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633])]


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_infer_with_write_vectors_end_to_end(tiny_checkpoint, tmp_path):
    from floodplanet_code_amd import infer as I
    from floodplanet_code_amd import predict as P
    from floodplanet_code_amd.datasets.synthetic import write_strip_tiff
    from floodplanet_code_amd.datasets.tiff import read_tiff
    exp, ckpt = tiny_checkpoint
    cfg = P.resolve_cfg(exp, ckpt)
    g = np.random.default_rng(11)
    paths = []
    for i, (h, w) in enumerate([(70, 53), (33, 90)]):      # per-pixel noise in dB: the class map comes out speckled
        p = str(tmp_path / "Scenes" / f"S_{i:02d}.tif")
        os.makedirs(os.path.dirname(p), exist_ok=True)
        write_strip_tiff(p, (g.random((2, h, w), dtype=np.float32) * 70 - 50).astype(np.float32), rows_per_strip=7,
                         extra_tags=GEO)
        paths.append(p)
    common = dict(cfg=cfg, stride=16, batch_size=4, blend="hann", sieve=4, sieve_connectivity=8)
    plain = I.infer(ckpt, paths, str(tmp_path / "plain"), **common)
    vec = I.infer(ckpt, paths, str(tmp_path / "vec"), write_vectors=True, **common)
    assert "vectors" not in plain and all("vectors" not in r for r in plain["scenes"])
    assert "vectors" not in json.load(open(tmp_path / "plain" / "summary.json"))
    totals = dict(polygons=0, rings=0, edges=0)
    for a, b in zip(plain["scenes"], vec["scenes"]):
        assert _read(a["output"]) == _read(b["output"])                                # the same class map, byte for byte
        assert not os.path.exists(a["output"][:-4] + ".geojson")
        assert {k: v for k, v in b.items() if k not in ("vectors", "output")} == \
            {k: v for k, v in a.items() if k != "output"}
        m = read_tiff(b["output"])
        H, W = m.shape
        v = b["vectors"]
        assert v["path"] == b["output"][:-4] + ".geojson" and v["values"] == [255] and v["connectivity"] == 8
        doc = json.load(open(v["path"]))
        assert doc["crs"]["properties"]["name"] == "urn:ogc:def:crs:EPSG::32633"
        rings, pixels = [], 0
        for f in doc["features"]:
            assert f["properties"]["value"] == 255 and f["properties"]["area"] == f["properties"]["pixels"] * 64.0
            pixels += f["properties"]["pixels"]
            for coords in f["geometry"]["coordinates"]:
                c = np.asarray(coords)
                back = np.stack([(c[:, 0] - 500000.0) / 8.0, (4100000.0 - c[:, 1]) / 8.0], axis=1)
                assert np.array_equal(back, np.rint(back))
                rings.append(back[:-1].astype(np.int64))
        water = m == 255
        print(f"{os.path.basename(b['output'])}: water share {float(water.mean()):.3f}, {v}")
        assert np.array_equal(V.fill_even_odd(rings, (H, W)), water) and pixels == int(water.sum())
        labels = PP.label_components_host(m, 8)
        assert v["polygons"] == len(doc["features"]) == len(np.unique(labels[water])) and v["rings"] == len(rings)
        assert v["edges"] == int(V.edge_offsets_host(m, V.select_flags([255]))[-1])
        for k in totals:
            totals[k] += v[k]
    assert totals["polygons"] > 0, "the scenes should hold water"
    summary = json.load(open(tmp_path / "vec" / "summary.json"))
    assert summary["vectors"] == dict(values=[255], connectivity=8, max_edges=1 << 24, skipped_scenes=0, **totals)
    drop = ("vectors", "scenes", "seconds", "crops_per_s")
    plain_summary = json.load(open(tmp_path / "plain" / "summary.json"))
    assert {k: v for k, v in summary.items() if k not in drop} == {k: v for k, v in plain_summary.items() if k not in drop}
    # a scene over the limit is recorded and skipped; the run goes on
    over = I.infer(ckpt, paths[:1], str(tmp_path / "over"), write_vectors=True, vector_max_edges=3, **common)
    rec = over["scenes"][0]
    assert rec["vectors"] == {"skipped": f"{vec['scenes'][0]['vectors']['edges']} edges > 3"}
    assert not os.path.exists(rec["output"][:-4] + ".geojson") and _read(rec["output"]) == _read(vec["scenes"][0]["output"])
    assert over["vectors"]["skipped_scenes"] == 1 and over["vectors"]["polygons"] == 0
