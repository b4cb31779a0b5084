"""Polygons of a class map: crack edges, their rings, and a GeoJSON writer.

A class map's water bodies become polygons by walking the boundaries between pixels (the "cracks").  The *_host functions
below are the specification, in vectorised numpy, as postprocess.py's are; edge_offsets and edge_rings run the same on
device tensors (fu_map_edge_offsets, fu_map_edge_rings in include/floodunet.h) and return the same bits.  Everything is
integer work and canonical, so results compare with ==.  rings_to_polygons, grid_transform and write_geojson are host
only.  This is an extension; the reference has no vector output.

Crack edges.  Grid vertices are pixel corners (x, y), 0 <= x <= W, 0 <= y <= H, with index y * (W + 1) + x; x runs to the
right and y down.  A selected pixel (select[value] != 0) owns a directed unit edge on every side where the neighbour lies
outside the map or has another value, oriented so that the pixel is on the edge's right:

    side 0 top     heading 0 E   from (x, y)          side 2 bottom  heading 2 W   from (x + 1, y + 1)
    side 1 right   heading 1 S   from (x + 1, y)      side 3 left    heading 3 N   from (x, y + 1)

The canonical edge order is by owner pixel y * W + x, then by side.  The index of "pixel q's side s" is offsets[q] + the
number of q's emitted sides below s.

Successor.  Edge e of pixel p, heading d, ends at vertex v.  R is the pixel ahead-right of v (p's neighbour in direction
d), Lp the pixel ahead-left (R's neighbour across side d); "in" means inside the map and of p's value.

    R in, Lp in      Lp's side (d + 3) % 4    turn left
    R in, Lp out     R's side d               straight on
    R out, Lp in     connectivity 8: Lp's side (d + 3) % 4; connectivity 4: p's side (d + 1) % 4
    R out, Lp out    p's side (d + 1) % 4     turn right

next is a permutation of the edges; each of its cycles (a ring) stays inside one component of
postprocess.label_components_host(m, connectivity); with A2 = sum(x_i * y_{i+1} - x_{i+1} * y_i) over a ring's vertices in
ring order (twice the signed area), a component has exactly one ring with A2 > 0, its outer ring, the others are holes
with A2 < 0, and the A2 of a component's rings sum to twice its pixel count.
"""
from __future__ import annotations

import json
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .postprocess import MAX_PIXELS, _check_map, _check_map_tensor, _workspace, label_components_host

ARRAYS = ("start", "comp", "ring", "rank", "flags")      # what edge_rings_host / edge_rings return, int32 [n_edges] each
MAX_EDGES_DEFAULT = 1 << 24
_DY = np.array([0, 1, 0, -1], dtype=np.int64)            # headings E, S, W, N; side s heads s, its neighbour lies in
_DX = np.array([1, 0, -1, 0], dtype=np.int64)            # direction (s + 3) % 4
_START_DX = np.array([0, 1, 1, 0], dtype=np.int64)       # the start vertex of pixel (y, x)'s side s
_START_DY = np.array([0, 0, 1, 1], dtype=np.int64)
_POPCOUNT4 = np.array([bin(i).count("1") for i in range(16)], dtype=np.int64)


def select_flags(values: Sequence[int]) -> np.ndarray:
    """The 256 selection flags (uint8) that select exactly `values`."""
    select = np.zeros(256, dtype=np.uint8)
    for v in values:
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 255:
            raise ValueError(f"a selected value must be an integer in 0..255, got {v!r}")
        select[int(v)] = 1
    return select


def _check_select(select) -> np.ndarray:
    select = np.asarray(select)
    if select.shape != (256,):
        raise ValueError(f"select must hold 256 flags, one per map value, got shape {tuple(select.shape)}")
    return (select != 0).astype(np.uint8)


def _padded(m: np.ndarray) -> np.ndarray:
    P = np.full((m.shape[0] + 2, m.shape[1] + 2), -1, dtype=np.int16)
    P[1:-1, 1:-1] = m
    return P


def side_masks_host(m: np.ndarray, select) -> np.ndarray:
    """uint8 [H, W]: bit s is set where the pixel is selected and owns an edge on side s."""
    m = np.asarray(m)
    _check_map(m, 4)
    select = _check_select(select)
    P = _padded(m)
    c = P[1:-1, 1:-1]
    mask = ((P[:-2, 1:-1] != c).astype(np.uint8) | ((P[1:-1, 2:] != c).astype(np.uint8) << 1)
            | ((P[2:, 1:-1] != c).astype(np.uint8) << 2) | ((P[1:-1, :-2] != c).astype(np.uint8) << 3))
    return mask * select[m]


def edge_offsets_host(m: np.ndarray, select) -> np.ndarray:
    """int32 [H * W + 1]: the exclusive prefix sum of the per-pixel edge counts (0..4) in pixel order; the last element
    is n_edges."""
    mask = side_masks_host(m, select)
    if mask.size > MAX_PIXELS:
        raise ValueError(f"map {mask.shape[0]}x{mask.shape[1]} has more than 2^28 pixels")
    offsets = np.zeros(mask.size + 1, dtype=np.int64)
    np.cumsum(_POPCOUNT4[mask.ravel()], out=offsets[1:])
    return offsets.astype(np.int32)


def _edges_host(m: np.ndarray, select, connectivity: int):
    """-> (owner pixel, side, next edge) int64 [n_edges] each, in the canonical order."""
    H, W = m.shape
    mask = side_masks_host(m, select).ravel()
    offsets = edge_offsets_host(m, select).astype(np.int64)
    owner, d = np.nonzero((mask[:, None] >> np.arange(4, dtype=np.uint8)[None, :]) & 1)      # row-major: pixel, then side
    P = _padded(m)
    y, x = owner // W, owner % W
    ry, rx = y + _DY[d], x + _DX[d]
    dl = (d + 3) % 4
    ly, lx = ry + _DY[dl], rx + _DX[dl]
    v = P[y + 1, x + 1]
    r_in, l_in = P[ry + 1, rx + 1] == v, P[ly + 1, lx + 1] == v       # the border of P is -1: outside is never "in"
    left = l_in & (r_in | (connectivity == 8))
    straight = r_in & ~l_in
    q = np.where(left, ly * W + lx, np.where(straight, ry * W + rx, owner))
    s = np.where(left, dl, np.where(straight, d, (d + 1) % 4))
    nxt = offsets[q] + _POPCOUNT4[mask[q] & ((1 << s) - 1)]
    return owner, d, nxt


def _rounds(n: int) -> int:
    return int(max(n, 2) - 1).bit_length()               # ceil(log2(max(n, 2)))


def _ring_rank_host(nxt: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Pointer jumping, as the device does it: the smallest index on every cycle, and the steps from it."""
    n = nxt.size
    ident = np.arange(n, dtype=np.int64)
    ring, j = ident, nxt
    for _ in range(_rounds(n)):
        ring, j = np.minimum(ring, ring[j]), j[j]
    tail = nxt == ring                                   # the edge in front of its cycle's leader: the cycle is cut there
    dist, j = (~tail).astype(np.int64), np.where(tail, ident, nxt)
    for _ in range(_rounds(n)):
        dist, j = dist + dist[j], j[j]
    return ring, dist[ring] - dist                       # length - 1 - distance to the tail


def edge_rings_host(m: np.ndarray, select, connectivity: int = 4) -> Dict[str, np.ndarray]:
    """The crack edges of the selected values of a uint8 map [H, W] and their rings -> int32 [n_edges] arrays in the
    canonical edge order: "start" the start vertex index, "comp" the owner pixel's label in
    label_components_host(m, connectivity), "ring" the smallest edge index on the edge's cycle, "rank" the number of next
    steps from that edge (rank[ring[e]] == 0), "flags" heading | corner << 2, where corner says that the edge's predecessor
    has another heading, so that the edge's start vertex is a polygon vertex."""
    m = np.asarray(m)
    _check_map(m, connectivity)
    H, W = m.shape
    owner, d, nxt = _edges_host(m, select, connectivity)
    labels = label_components_host(m, connectivity).ravel()
    ring, rank = _ring_rank_host(nxt)
    corner = np.zeros(owner.size, dtype=np.int64)
    corner[nxt] = d != d[nxt]
    start = (owner // W + _START_DY[d]) * (W + 1) + owner % W + _START_DX[d]
    out = {"start": start, "comp": labels[owner], "ring": ring, "rank": rank, "flags": d | (corner << 2)}
    return {k: np.ascontiguousarray(a, dtype=np.int32) for k, a in out.items()}


# --------------------------------------------------------------------------------------------------- polygons (host only)
def rings_to_polygons(arrays: Dict[str, np.ndarray], m_shape: Tuple[int, int], m: Optional[np.ndarray] = None) -> List[dict]:
    """edge_rings' arrays -> one polygon per component, in ascending component label: {"value" (m's value at the label
    pixel; None without m), "label", "pixels" (from the rings' A2), "bbox_px" [x0, y0, x1, y1] in vertex coordinates,
    "rings": int64 [k, 2] arrays of (x, y) corner vertices in ring order, not closed -- the outer ring (A2 > 0) first, the
    holes (A2 < 0) behind it in ascending ring id}.  The edges are sorted by (ring, rank) and only corner vertices are
    kept.  With y down an outer ring runs clockwise on the screen and a hole counter-clockwise.
    Under connectivity 4 a ring may touch itself or a sibling ring at a vertex (two pixels that meet only diagonally are
    walked as two corners there), but rings never cross; gdal_polygonize behaves the same under its 8-connected mode, where
    a polygon's ring passes through such a vertex twice."""
    H, W = int(m_shape[0]), int(m_shape[1])
    start, comp, ring, rank, flags = (np.asarray(arrays[k]).astype(np.int64) for k in ARRAYS)
    if start.size == 0:
        return []
    order = np.lexsort((rank, ring))
    start, comp, ring, corner = start[order], comp[order], ring[order], (flags[order] >> 2) & 1
    x, y = start % (W + 1), start // (W + 1)
    first = np.flatnonzero(np.r_[True, ring[1:] != ring[:-1]])           # where each ring begins in the sorted order
    last = np.r_[first[1:], ring.size] - 1
    seg = np.cumsum(np.r_[True, ring[1:] != ring[:-1]]) - 1              # ring number of every edge
    nx_, ny_ = np.r_[x[1:], x[:1]], np.r_[y[1:], y[:1]]                  # the next vertex: the next edge's start, and at a
    nx_[last], ny_[last] = x[first], y[first]                            # ring's last edge the ring's first vertex
    a2 = np.bincount(seg, weights=(x * ny_ - nx_ * y).astype(np.float64), minlength=first.size).astype(np.int64)
    ring_id, ring_comp = ring[first], comp[first]
    x0 = np.minimum.reduceat(x, first); x1 = np.maximum.reduceat(x, first)
    y0 = np.minimum.reduceat(y, first); y1 = np.maximum.reduceat(y, first)
    keep = corner == 1
    corner_xy = np.stack([x[keep], y[keep]], axis=1)
    per_ring = np.split(corner_xy, np.cumsum(np.bincount(seg[keep], minlength=first.size))[:-1])
    by_comp = np.lexsort((ring_id, a2 < 0, ring_comp))                   # component, outer ring first, then ring id
    flat = None if m is None else np.asarray(m).ravel()
    polygons: List[dict] = []
    for r in by_comp:
        label = int(ring_comp[r])
        if not polygons or polygons[-1]["label"] != label:
            if a2[r] <= 0:
                raise ValueError(f"component {label} has no outer ring: the arrays are not edge_rings' of one map")
            polygons.append({"value": None if flat is None else int(flat[label]), "label": label, "pixels": 0,
                             "bbox_px": [int(x0[r]), int(y0[r]), int(x1[r]), int(y1[r])], "rings": []})
        elif a2[r] >= 0:
            raise ValueError(f"component {label} has two outer rings: the arrays are not edge_rings' of one map")
        polygons[-1]["pixels"] += int(a2[r])
        polygons[-1]["rings"].append(per_ring[r])
    for p in polygons:
        p["pixels"] //= 2
    return polygons


def fill_even_odd(rings: Sequence[np.ndarray], m_shape: Tuple[int, int]) -> np.ndarray:
    """bool [H, W]: the pixels inside an odd number of the given corner rings (rings_to_polygons' "rings", or closed
    rings in the same coordinates).  A pixel's parity is the number of vertical ring segments to its left (at x' <= x) that
    span its row."""
    H, W = int(m_shape[0]), int(m_shape[1])
    toggles = np.zeros((H, W + 1), dtype=np.int64)
    for ring in rings:
        r = np.asarray(ring).astype(np.int64)
        a, b = r, np.roll(r, -1, axis=0)
        for (xa, ya), (xb, yb) in zip(a[a[:, 0] == b[:, 0]], b[a[:, 0] == b[:, 0]]):
            toggles[min(ya, yb):max(ya, yb), xa] += 1
    return (np.cumsum(toggles, axis=1)[:, :W] & 1).astype(bool)


# ---------------------------------------------------------------------------------------------------- GeoJSON (host only)
def _geo_key(tags: dict, key: int) -> Optional[int]:
    keys = tags.get(34735) if tags else None
    if keys is None or len(keys) < 4:
        return None
    for i in range(int(keys[3])):
        k = keys[4 + 4 * i: 8 + 4 * i]
        if len(k) == 4 and int(k[0]) == key and int(k[1]) == 0:
            return int(k[3])
    return None


def crs_from_tags(tags: dict) -> Optional[int]:
    """The EPSG code of a raster's GeoKey directory: ProjectedCSType (3072), else GeographicType (2048); None when neither
    holds a code (0 undefined, 32767 user-defined)."""
    for key in (3072, 2048):
        code = _geo_key(tags, key)
        if code is not None and 0 < code < 32767:
            return code
    return None


def grid_transform(tags: dict, src_hw: Tuple[int, int], grid_hw: Tuple[int, int]) -> dict:
    """The map from a grid vertex (x, y) to the raster's CRS, from the source raster's GeoTIFF tags as
    infer.geo_tags_for_grid puts them on the output grid: ModelPixelScale (sx, sy) + ModelTiepoint (i, j, ., X0, Y0, .) give
    X = X0 + (x - i) * sx, Y = Y0 - (y - j) * sy; else ModelTransformation applied to (x, y); under PixelIsPoint (GeoKey 1025
    = 2) x - 0.5 and y - 0.5 take the place of x and y; without georeferencing, pixel coordinates.  -> {"kind": "scale" |
    "matrix" | "pixel", its numbers, "shift", "pixel_area" (|area of a pixel| in CRS units, None for "pixel")}.  There is no
    reprojection: coordinates stay in the raster's CRS."""
    from .infer import geo_tags_for_grid
    grid = {tag: values for tag, _, values in geo_tags_for_grid(tags or {}, src_hw, grid_hw)}
    shift = 0.5 if _geo_key(tags, 1025) == 2 else 0.0
    scale, tie, matrix = grid.get(33550), grid.get(33922), grid.get(34264)
    if scale is not None and tie is not None and len(tie) >= 6:
        sx, sy = float(scale[0]), float(scale[1])
        return {"kind": "scale", "scale": (sx, sy), "tie": (float(tie[0]), float(tie[1]), float(tie[3]), float(tie[4])),
                "shift": shift, "pixel_area": abs(sx * sy)}
    if matrix is not None and len(matrix) == 16:
        a, b, c, d, e, f = (float(matrix[k]) for k in (0, 1, 3, 4, 5, 7))
        return {"kind": "matrix", "matrix": (a, b, c, d, e, f), "shift": shift, "pixel_area": abs(a * e - b * d)}
    return {"kind": "pixel", "shift": 0.0, "pixel_area": None}


def apply_transform(transform: dict, x: np.ndarray, y: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Grid vertices -> world coordinates (float64) under a grid_transform."""
    x = np.asarray(x, dtype=np.float64) - transform["shift"]
    y = np.asarray(y, dtype=np.float64) - transform["shift"]
    if transform["kind"] == "scale":
        (sx, sy), (i, j, X0, Y0) = transform["scale"], transform["tie"]
        return X0 + (x - i) * sx, Y0 - (y - j) * sy
    if transform["kind"] == "matrix":
        a, b, c, d, e, f = transform["matrix"]
        return a * x + b * y + c, d * x + e * y + f
    return x, y


def _ring_text(ring: np.ndarray, transform: dict, exterior: bool) -> str:
    X, Y = apply_transform(transform, ring[:, 0], ring[:, 1])
    shoelace = float(np.sum(X * np.roll(Y, -1) - np.roll(X, -1) * Y))   # > 0: counter-clockwise in world coordinates
    if (shoelace > 0) != exterior:
        X, Y = X[::-1], Y[::-1]
    X, Y = X.tolist(), Y.tolist()
    return "[" + ",".join(f"[{a!r},{b!r}]" for a, b in zip(X + X[:1], Y + Y[:1])) + "]"


def write_geojson(path: str, polygons: List[dict], transform: dict, crs: Optional[int] = None) -> None:
    """rings_to_polygons' polygons as a GeoJSON FeatureCollection, one Polygon feature per component with the properties
    value, label, pixels, area (pixels times the transform's pixel area; null without georeferencing) and bbox_px.  Rings
    are closed (the first vertex repeated); exterior rings run counter-clockwise and holes clockwise in world
    coordinates, decided by the sign of the shoelace sum there, so a south-up raster is right too.  Coordinates are
    written with repr(float) in the raster's CRS; crs, an EPSG code, becomes the legacy "crs" member that GDAL and QGIS
    honour.  The bytes depend on the arguments alone."""
    area = transform["pixel_area"]
    features = []
    for p in polygons:
        props = {"value": p["value"], "label": p["label"], "pixels": p["pixels"],
                 "area": None if area is None else float(p["pixels"] * area), "bbox_px": p["bbox_px"]}
        rings = ",".join(_ring_text(r, transform, k == 0) for k, r in enumerate(p["rings"]))
        features.append('{"type": "Feature", "properties": ' + json.dumps(props) +
                        ', "geometry": {"type": "Polygon", "coordinates": [' + rings + "]}}")
    head = '{"type": "FeatureCollection", '
    if crs is not None:
        head += '"crs": {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::%d"}}, ' % int(crs)
    with open(path, "w") as fh:
        fh.write(head + '"features": [' + ("\n" + ",\n".join(features) + "\n" if features else "") + "]}\n")


# ---------------------------------------------------------------------------------------------------------- device side
def _select_bytes(select):
    import ctypes
    return (ctypes.c_uint8 * 256).from_buffer_copy(_check_select(select).tobytes())


def edge_offsets(map_t, select):
    """edge_offsets_host on a device tensor: uint8 [H, W] -> int32 [H * W + 1] on the same device (fu_map_edge_offsets, on
    the current stream: three launches, no host read), bit for bit."""
    import torch
    from . import _lib
    H, W = _check_map_tensor(map_t, "edge_offsets")
    lib = _lib.load()
    offsets = torch.empty(H * W + 1, dtype=torch.int32, device=map_t.device)
    nbytes = int(lib.fu_map_edges_workspace_bytes(H, W))
    ws = _workspace(map_t.device, nbytes)
    with torch.cuda.device(map_t.device):
        _lib.check(lib.fu_map_edge_offsets(map_t.data_ptr(), H, W, _select_bytes(select), offsets.data_ptr(), ws.data_ptr(),
                                           nbytes, torch.cuda.current_stream(map_t.device).cuda_stream))
    return offsets


def count_and_rings(map_t, select, connectivity: int = 4, labels=None, max_edges: Optional[int] = None):
    """edge_rings, and the edge count with it -> (n_edges, the arrays or None when n_edges > max_edges)."""
    import torch
    from . import _lib
    from .postprocess import label_components
    H, W = _check_map_tensor(map_t, "edge_rings")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    if labels is None:
        labels = label_components(map_t, connectivity)
    elif labels.shape != map_t.shape or labels.dtype != torch.int32 or labels.device != map_t.device or \
            not labels.is_contiguous():
        raise ValueError("edge_rings: labels must be a contiguous int32 tensor of the map's shape on the map's device")
    select_c = _select_bytes(select)
    offsets = edge_offsets(map_t, select)
    n = int(offsets[-1].item())                          # the one small read: 4 bytes
    if max_edges is not None and n > max_edges:
        return n, None
    out = {k: torch.empty(n, dtype=torch.int32, device=map_t.device) for k in ARRAYS}
    if n > 0:
        lib = _lib.load()
        nbytes = int(lib.fu_map_rings_workspace_bytes(n))
        ws = _workspace(map_t.device, nbytes)
        with torch.cuda.device(map_t.device):
            _lib.check(lib.fu_map_edge_rings(map_t.data_ptr(), labels.data_ptr(), H, W, select_c, int(connectivity),
                                             offsets.data_ptr(), n, *(out[k].data_ptr() for k in ARRAYS), ws.data_ptr(),
                                             nbytes, torch.cuda.current_stream(map_t.device).cuda_stream))
    return n, out


def edge_rings(map_t, select, connectivity: int = 4, labels=None, max_edges: Optional[int] = None):
    """edge_rings_host on a device tensor: uint8 [H, W] -> {"start", "comp", "ring", "rank", "flags"}, int32 [n_edges]
    tensors on the map's device, bit for bit; None when n_edges > max_edges.  Runs on the current stream:
    label_components unless labels (int32 [H, W], of the same connectivity) is given, fu_map_edge_offsets, ONE 4-byte
    device-to-host read (n_edges, which sizes the outputs), fu_map_edge_rings.  The workspace (20 B per edge) is
    cached per device and shared with postprocess.sieve's, which a stream orders; do not run two of these calls on one
    device from different streams at once."""
    return count_and_rings(map_t, select, connectivity, labels, max_edges)[1]
