"""CPU: the numpy statements of vectorize.py -- the invariants of the crack-edge successor rule against
label_components_host for both connectivities, polygons that fill back to the map, the GeoJSON writer under an exactly
representable transform, and the vector options of InferOptions.  Integers throughout: every comparison is ==."""
import functools
import json
import time

import numpy as np
import pytest

from floodplanet_code_amd import vectorize as V
from floodplanet_code_amd.infer_options import KEYWORDS, InferOptions
from floodplanet_code_amd.postprocess import label_components_host

ALL = np.ones(256, dtype=np.uint8)


def _random(shape, seed, fill):
    return ((np.random.default_rng(seed).random(shape) < fill) * 255).astype(np.uint8)


def _nested():
    """An island in a lake in an island: 9 x 9 of 255 inside a border of 0, a 5 x 5 lake of 0, one pixel of 255 in it."""
    m = np.zeros((11, 11), np.uint8)
    m[1:10, 1:10] = 255
    m[3:8, 3:8] = 0
    m[5, 5] = 255
    return m


MAPS = {"1x1": lambda: np.full((1, 1), 255, np.uint8), "1x7": lambda: _random((1, 7), 1, 0.5),
        "5x1": lambda: _random((5, 1), 2, 0.5),
        **{f"{h}x{w}_fill{int(f * 10)}": (lambda h=h, w=w, f=f: _random((h, w), h + int(f * 10), f))
           for h, w in ((13, 17), (37, 45)) for f in (0.1, 0.5, 0.9)},
        "three_values_20x23": lambda: (np.random.default_rng(3).integers(0, 3, (20, 23)) * 100).astype(np.uint8),
        "checkerboard_8x8": lambda: ((np.indices((8, 8)).sum(0) % 2) * 255).astype(np.uint8),
        "nested_11x11": _nested}
SELECTS = {"all": ALL, "255": V.select_flags([255]), "none": V.select_flags([])}


@functools.lru_cache(maxsize=None)
def host_map(name):
    m = MAPS[name]()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def host_labels(name, connectivity):
    return label_components_host(host_map(name), connectivity)


@pytest.mark.parametrize("select", sorted(SELECTS))
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_the_successor_rule_keeps_its_invariants(name, connectivity, select):
    m, sel = host_map(name), SELECTS[select]
    H, W = m.shape
    labels = host_labels(name, connectivity).ravel()
    offsets = V.edge_offsets_host(m, sel)
    owner, d, nxt = V._edges_host(m, sel, connectivity)
    n = int(offsets[-1])
    assert offsets.dtype == np.int32 and offsets.shape == (H * W + 1,) and offsets[0] == 0 and owner.size == n
    chosen = (sel[m] != 0).ravel()
    assert not np.any(np.diff(offsets)[~chosen]) and int(np.diff(offsets).max(initial=0)) <= 4
    assert np.array_equal(np.repeat(np.arange(H * W), np.diff(offsets)), owner)       # canonical order: by owner, then side
    assert n == 0 or bool(np.all((np.diff(owner) > 0) | (np.diff(d) > 0)))
    if select == "none":
        assert n == 0
    assert np.array_equal(np.sort(nxt), np.arange(n))                 # a permutation
    A = V.edge_rings_host(m, sel, connectivity)
    assert sorted(A) == sorted(V.ARRAYS) and all(a.dtype == np.int32 and a.shape == (n,) for a in A.values())
    assert np.array_equal(A["comp"], labels[owner]) and np.array_equal(A["comp"][nxt], A["comp"])    # one component
    assert np.array_equal(A["flags"] & 3, d)
    x, y = A["start"] % (W + 1), A["start"] // (W + 1)
    assert np.array_equal(x + V._DX[d], x[nxt]) and np.array_equal(y + V._DY[d], y[nxt])      # consecutive edges meet
    assert np.array_equal((A["flags"] >> 2)[nxt], (d != d[nxt]).astype(np.int32))
    # ring: the smallest index of the cycle; rank: steps from it -- walked here one step at a time, all cycles at once
    ring, at = np.arange(n), np.arange(n)
    for _ in range(n):                                                # no cycle is longer than n
        at = nxt[at]
        ring = np.minimum(ring, at)
    assert np.array_equal(A["ring"], ring)
    lead = A["ring"] == np.arange(n)
    assert bool(np.all(A["rank"][lead] == 0))
    assert np.array_equal(A["rank"][nxt][~lead[nxt]], A["rank"][~lead[nxt]] + 1)
    # signed areas: one outer ring per component, the rest holes, and together the component's pixels
    a2 = np.bincount(A["ring"], weights=x * (y + V._DY[d]) - (x + V._DX[d]) * y, minlength=n).astype(np.int64)[lead]
    comp_of_ring = A["comp"][lead]
    sizes = np.bincount(labels, minlength=H * W)
    for label in np.unique(labels[chosen]):
        mine = a2[comp_of_ring == label]
        assert int((mine > 0).sum()) == 1 and int((mine < 0).sum()) == mine.size - 1, (label, mine)
        assert int(mine.sum()) == 2 * sizes[label]
    assert set(comp_of_ring.tolist()) == set(np.unique(labels[chosen]).tolist())


def test_the_host_statement_is_vectorised():
    m = _random((257, 300), 5, 0.5)
    t0 = time.perf_counter()
    A = V.edge_rings_host(m, ALL, 4)
    seconds = time.perf_counter() - t0
    assert A["start"].size > 100000 and seconds < 1.0, seconds      # vectorised: no per-edge Python loop


def test_nested_rings_and_checkerboard_saddles():
    m = _nested()
    for connectivity in (4, 8):
        polys = V.rings_to_polygons(V.edge_rings_host(m, V.select_flags([255]), connectivity), m.shape, m)
        assert [(p["value"], p["label"], p["pixels"], len(p["rings"]), p["bbox_px"]) for p in polys] == \
            [(255, 12, 56, 2, [1, 1, 10, 10]), (255, 60, 1, 1, [5, 5, 6, 6])]
        assert [len(r) for r in polys[0]["rings"]] == [4, 4] and polys[0]["rings"][0].tolist() == [[1, 1], [10, 1], [10, 10], [1, 10]]
        polys = V.rings_to_polygons(V.edge_rings_host(m, ALL, connectivity), m.shape, m)
        assert [(p["value"], p["pixels"], len(p["rings"])) for p in polys] == [(0, 40, 2), (255, 56, 2), (0, 24, 2), (255, 1, 1)]
    cb = MAPS["checkerboard_8x8"]()
    four = V.rings_to_polygons(V.edge_rings_host(cb, ALL, 4), cb.shape, cb)
    assert len(four) == 64 and all(p["pixels"] == 1 and len(p["rings"]) == 1 and len(p["rings"][0]) == 4 for p in four)
    eight = V.rings_to_polygons(V.edge_rings_host(cb, ALL, 8), cb.shape, cb)        # every inner vertex is a saddle
    assert [(p["value"], p["pixels"]) for p in eight] == [(0, 32), (255, 32)]
    # a hole of one colour is a pixel of the other that does not lie on the map's border: 18 of the inner 6 x 6
    assert [len(p["rings"]) for p in eight] == [1 + 18, 1 + 18]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_polygons_fill_back_to_the_map(name, connectivity):
    m = host_map(name)
    labels = host_labels(name, connectivity)
    polys = V.rings_to_polygons(V.edge_rings_host(m, ALL, connectivity), m.shape, m)
    assert [p["label"] for p in polys] == np.unique(labels).tolist()
    for value in np.unique(m):
        rings = [r for p in polys if p["value"] == value for r in p["rings"]]
        assert np.array_equal(V.fill_even_odd(rings, m.shape), m == value)
    for p in polys:
        inside = V.fill_even_odd(p["rings"], m.shape)
        assert np.array_equal(inside, labels == p["label"]) and p["pixels"] == int(inside.sum())
        ys, xs = np.nonzero(inside)
        assert p["bbox_px"] == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1] and p["value"] == m.ravel()[p["label"]]
    assert V.rings_to_polygons(V.edge_rings_host(m, SELECTS["none"], connectivity), m.shape, m) == []


# ----------------------------------------------------------------------------------------------------------- GeoJSON
def _tags(point=False, epsg=(3072, 32633), matrix=False, south_up=False):
    keys = [1, 1, 0, 2, 1025, 0, 1, 2 if point else 1, epsg[0], 0, 1, epsg[1]]
    if matrix:
        return {34264: [0.5, 0.0, 0.0, 4096.0, 0.0, 0.25 if south_up else -0.25, 0.0, 8192.0, 0, 0, 0, 0, 0, 0, 0, 1], 34735: keys}
    return {33550: [0.5, 0.25, 0.0], 33922: [2.0, 4.0, 0.0, 4096.0, 8192.0, 0.0], 34735: keys}


def _features(path):
    with open(path) as fh:
        doc = json.load(fh)
    assert doc["type"] == "FeatureCollection"
    return doc, doc["features"]


def _shoelace(ring):
    r = np.asarray(ring)
    return float(np.sum(r[:-1, 0] * r[1:, 1] - r[1:, 0] * r[:-1, 1]))


@pytest.mark.parametrize("kind", ["scale", "scale_point", "matrix", "matrix_south_up", "pixel"])
def test_geojson_round_trips_exactly(tmp_path, kind):
    m = host_map("37x45_fill5")
    polys = V.rings_to_polygons(V.edge_rings_host(m, V.select_flags([255]), 8), m.shape, m)
    assert any(len(p["rings"]) > 1 for p in polys)
    tags = {} if kind == "pixel" else _tags(point=kind == "scale_point", matrix=kind.startswith("matrix"),
                                             south_up=kind == "matrix_south_up")
    tr = V.grid_transform(tags, m.shape, m.shape)
    assert tr["kind"] == kind.split("_")[0] and tr["pixel_area"] == (None if kind == "pixel" else 0.125)
    path = str(tmp_path / "a.geojson")
    V.write_geojson(path, polys, tr, V.crs_from_tags(tags))
    doc, features = _features(path)
    assert len(features) == len(polys)
    if kind == "pixel":
        assert "crs" not in doc
    else:
        assert doc["crs"] == {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::32633"}}
    shift = 0.5 if kind == "scale_point" else 0.0
    for f, p in zip(features, polys):
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon"
        assert f["properties"] == {"value": 255, "label": p["label"], "pixels": p["pixels"], "bbox_px": p["bbox_px"],
                                   "area": None if kind == "pixel" else p["pixels"] * 0.125}
        assert len(f["geometry"]["coordinates"]) == len(p["rings"])
        for k, (coords, ring) in enumerate(zip(f["geometry"]["coordinates"], p["rings"])):
            assert coords[0] == coords[-1] and len(coords) == len(ring) + 1           # closed
            c = np.asarray(coords)
            if kind == "pixel":
                x, y = c[:, 0], c[:, 1]
            elif kind.startswith("scale"):
                x, y = (c[:, 0] - 4096.0) / 0.5 + 2.0 + shift, (8192.0 - c[:, 1]) / 0.25 + 4.0 + shift
            else:
                x, y = (c[:, 0] - 4096.0) / 0.5, (c[:, 1] - 8192.0) / (0.25 if kind == "matrix_south_up" else -0.25)
            back = np.stack([x, y], axis=1)[:-1]
            assert np.array_equal(back, np.rint(back))                                 # grid vertices, exactly
            steps = {(tuple(a), tuple(b)) for a, b in zip(ring.tolist(), np.roll(ring, -1, axis=0).tolist())}
            walked = {(tuple(a), tuple(b)) for a, b in zip(back.astype(np.int64).tolist(),
                                                           np.roll(back, -1, axis=0).astype(np.int64).tolist())}
            same, turned = walked == steps, walked == {(b, a) for a, b in steps}       # the ring, or the ring reversed
            assert same != turned
            area2 = _shoelace(coords)                 # exterior counter-clockwise, holes clockwise, in world coordinates
            assert (area2 > 0) if k == 0 else (area2 < 0), (kind, k, area2)
            # with y down (pixel, south-up) the ring order of rings_to_polygons already is counter-clockwise in the world
            assert same == (kind in ("pixel", "matrix_south_up"))
    first = open(path, "rb").read()
    V.write_geojson(path, polys, tr, V.crs_from_tags(tags))
    assert open(path, "rb").read() == first                                            # deterministic


def test_pixel_is_point_shifts_by_half_a_pixel_and_crs_follows_the_geokeys(tmp_path):
    m = np.full((2, 3), 255, np.uint8)
    polys = V.rings_to_polygons(V.edge_rings_host(m, ALL, 4), m.shape, m)
    out = []
    for point in (False, True):
        path = str(tmp_path / f"p{int(point)}.geojson")
        V.write_geojson(path, polys, V.grid_transform(_tags(point=point), m.shape, m.shape), None)
        doc, features = _features(path)
        assert "crs" not in doc
        out.append(np.asarray(features[0]["geometry"]["coordinates"][0]))
    assert np.array_equal(out[1] - out[0], np.broadcast_to([-0.25, 0.125], out[0].shape))      # half of (0.5, -0.25)
    assert V.crs_from_tags(_tags(epsg=(3072, 32615))) == 32615 and V.crs_from_tags(_tags(epsg=(2048, 4326))) == 4326
    assert V.crs_from_tags(_tags(epsg=(3072, 32767))) is None and V.crs_from_tags({}) is None
    # on a resampled grid the transform is the grid's: twice the pixels, half the pixel size
    tr = V.grid_transform(_tags(), (10, 10), (20, 20))
    assert tr["scale"] == (0.25, 0.125) and tr["tie"] == (4.0, 8.0, 4096.0, 8192.0)
    path = str(tmp_path / "empty.geojson")
    V.write_geojson(path, [], tr, 32633)
    doc, features = _features(path)
    assert features == [] and doc["crs"]["properties"]["name"].endswith("::32633")


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_header_and_binding_name_the_new_symbols_and_checks_need_no_gpu():
    import os
    import re
    from floodplanet_code_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "floodunet.h")).read()
    assert int(re.search(r"#define\s+FU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5      # additive: no version bump
    lib = _lib.load()
    for name in ("fu_map_edges_workspace_bytes", "fu_map_edge_offsets", "fu_map_rings_workspace_bytes", "fu_map_edge_rings"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.fu_abi_version() == 5
    assert lib.fu_map_edges_workspace_bytes(1024, 1024) == 2064 and lib.fu_map_edges_workspace_bytes(0, 5) == 0   # 512 + 1 ints
    assert lib.fu_map_rings_workspace_bytes(1 << 20) == 20 << 20 and lib.fu_map_rings_workspace_bytes(-1) == 0
    # every check comes before anything is launched: a rejected call never opens the GPU
    select = V._select_bytes(ALL)
    assert lib.fu_map_edge_offsets(None, 4, 4, select, None, None, 0, None) == _lib.FU_ERR_INVALID
    assert b"fu_map_edge_offsets: null" in lib.fu_last_error()
    assert lib.fu_map_edge_rings(None, None, 4, 4, select, 4, None, 16, None, None, None, None, None, None, 0,
                                 None) == _lib.FU_ERR_INVALID
    assert b"fu_map_edge_rings: null" in lib.fu_last_error()


# ----------------------------------------------------------------------------------------------------------- options
def test_vector_options_defaults_and_values():
    assert {"write_vectors", "vector_values", "vector_connectivity", "vector_max_edges"} <= set(KEYWORDS)
    off = InferOptions.make()
    assert (off.write_vectors, type(off)) == (False, InferOptions)
    o = InferOptions.make(write_vectors=True)
    assert (o.write_vectors, o.vector_values, o.vector_connectivity, o.vector_max_edges) == (True, (255,), 4, 1 << 24)
    assert isinstance(o, InferOptions) and o != off and o.resolve(64, 64, 4).write_vectors
    assert InferOptions.make(write_vectors=True, sieve=9, sieve_connectivity=8).vector_connectivity == 8
    assert InferOptions.make(write_vectors=True, sieve=9, sieve_connectivity=8, vector_connectivity=4).vector_connectivity == 4
    o = InferOptions.make(write_vectors=True, vector_values=[255, 0, 255], vector_connectivity=8, vector_max_edges=1000,
                          nodata="auto", decode="device")
    assert (o.vector_values, o.vector_connectivity, o.vector_max_edges, o.nodata, o.decode) == ((0, 255), 8, 1000, "auto",
                                                                                                 "device")
    assert hash(o) == hash(InferOptions.make(write_vectors=True, vector_values=(0, 255), vector_connectivity=8,
                                             vector_max_edges=1000, nodata="auto", decode="device"))


@pytest.mark.parametrize("kw,message", [
    (dict(vector_values=[255]), "infer: --vector_values needs --write_vectors"),
    (dict(vector_connectivity=8), "infer: --vector_connectivity needs --write_vectors"),
    (dict(vector_max_edges=5), "infer: --vector_max_edges needs --write_vectors"),
    (dict(write_vectors=True, vector_values=[256]), "infer: vector_values must be integers in 0..255, got 256"),
    (dict(write_vectors=True, vector_values=[-1]), "infer: vector_values must be integers in 0..255, got -1"),
    (dict(write_vectors=True, vector_values=[1.5]), "infer: vector_values must be integers in 0..255, got 1.5"),
    (dict(write_vectors=True, vector_connectivity=5), "infer: vector_connectivity must be 4 or 8, got 5"),
    (dict(write_vectors=True, vector_max_edges=-1), "infer: vector_max_edges must be an integer >= 0, got -1"),
])
def test_vector_option_errors_come_before_any_gpu_work(kw, message, tmp_path, monkeypatch):
    import torch
    from floodplanet_code_amd import infer as I
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: pytest.fail("the GPU was touched"))
    with pytest.raises(ValueError) as e:
        InferOptions.make(**kw)
    assert str(e.value) == message
    cfg = dict(crop_height=64, crop_width=64, batch_size=4, norm_mode=None,
               dataset=dict(name="floodplanet", channels="ALL", sensor="S1", dataset_kwargs=None),
               model=dict(name="ms_model", model_kwargs=dict(base_channels=8)))
    with pytest.raises(ValueError) as e:
        I.infer(str(tmp_path / "missing.ckpt"), [str(tmp_path)], str(tmp_path / "out"), cfg=cfg, **kw)
    assert str(e.value) == message and not (tmp_path / "out").exists()


def test_command_line_gives_the_vector_keywords():
    from floodplanet_code_amd import infer as I
    base = ["e/checkpoints/c.ckpt", "scenes", "--out_dir", "o"]
    rows = [(["--write_vectors"], dict(write_vectors=True)),
            (["--write_vectors", "--vector_values", "255", "0", "--vector_connectivity", "8", "--vector_max_edges", "77",
              "--sieve", "5"], dict(write_vectors=True, vector_values=[0, 255], vector_connectivity=8, vector_max_edges=77,
                                    sieve=5))]
    for line, kw in rows:
        assert InferOptions.from_args(I.build_parser().parse_args(base + line)) == InferOptions.make(**kw)
    with pytest.raises(ValueError, match="needs --write_vectors"):
        InferOptions.from_args(I.build_parser().parse_args(base + ["--vector_values", "255"]))


def test_write_scene_vectors_records(tmp_path):
    """Host only: the record of a scene's vectors, the skipped scene, and the summary's totals."""
    from floodplanet_code_amd import infer as I
    m = _nested()
    options = InferOptions.make(write_vectors=True, vector_max_edges=100).resolve(64, 64, 4)
    scene = {"hw": m.shape, "src_hw": m.shape, "tags": _tags(), "n": 1}
    arrays = dict(V.edge_rings_host(m, V.select_flags([255]), 4), edges=60, counts=np.array([0, 0]))
    arrays["class"] = m
    out = str(tmp_path / "a.tif")
    rec = I.write_scene(arrays, scene, options, "in.tif", out)
    assert rec["vectors"] == {"path": str(tmp_path / "a.geojson"), "polygons": 2, "rings": 3, "edges": 60, "values": [255],
                              "connectivity": 4}
    assert len(_features(rec["vectors"]["path"])[1]) == 2
    over = {"class": m, "edges": 101, "counts": np.array([0, 0])}
    out2 = str(tmp_path / "b.tif")
    rec2 = I.write_scene(over, scene, options, "in2.tif", out2)
    assert rec2["vectors"] == {"skipped": "101 edges > 100"} and not (tmp_path / "b.geojson").exists()
    summary = I.run_summary([rec, rec2], 2, 1.0, 1, options, "raw")
    assert summary["vectors"] == {"values": [255], "connectivity": 4, "max_edges": 100, "polygons": 2, "rings": 3, "edges": 60,
                                  "skipped_scenes": 1}
    assert "vectors" not in I.run_summary([], 0, 1.0, 0, InferOptions.make().resolve(64, 64, 4), "raw")
    # a scene without a crop (all fill under --nodata) and a scene without a selected pixel: an empty FeatureCollection
    fill = InferOptions.make(write_vectors=True, nodata=0).resolve(64, 64, 4)
    empty = I.empty_scene_arrays({"hw": (5, 7)}, 3, fill)
    assert empty["edges"] == 0 and all(empty[k].shape == (0,) and empty[k].dtype == np.int32 for k in V.ARRAYS)
    rec3 = I.write_scene(empty, dict(scene, hw=(5, 7), src_hw=(5, 7), nodata=0.0, skipped=1, n=0), fill, "in3.tif",
                         str(tmp_path / "c.tif"))
    assert rec3["vectors"]["polygons"] == 0 and _features(rec3["vectors"]["path"])[1] == []
    dry = dict(V.edge_rings_host(np.zeros((4, 4), np.uint8), V.select_flags([255]), 4), edges=0, counts=np.array([16, 0]))
    dry["class"] = np.zeros((4, 4), np.uint8)
    rec4 = I.write_scene(dry, dict(scene, hw=(4, 4), src_hw=(4, 4)), options, "in4.tif", str(tmp_path / "d.tif"))
    assert rec4["vectors"]["edges"] == 0 and _features(rec4["vectors"]["path"])[1] == []
