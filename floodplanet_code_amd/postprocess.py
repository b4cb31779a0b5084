"""Post-processing of class maps: connected components and the connected-component sieve.

An inferred class map is the per-pixel argmax and so is speckled: single water pixels in dry land, pinholes in water
bodies.  The sieve merges every patch below a minimum mapping unit into its surroundings.  This is an extension; the
reference has no post-processing.  The *_host functions below are the specification, in numpy; label_components and
sieve run the same on device tensors (fu_map_components, fu_map_sieve in include/floodunet.h) and return the same bits.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

MAX_PASSES = 8
MAX_PIXELS = 1 << 28


def _check_map(m: np.ndarray, connectivity: int) -> None:
    if m.ndim != 2 or m.dtype != np.uint8:
        raise ValueError(f"a class map is uint8 [H, W], got {m.dtype} {tuple(m.shape)}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")


def check_sieve_options(min_pixels, connectivity=4, passes=1, frozen_value=None) -> None:
    """The option checks sieve_host, sieve and infer share (host only)."""
    if int(min_pixels) != min_pixels or min_pixels < 0:
        raise ValueError(f"sieve: min_pixels must be an integer >= 0, got {min_pixels!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"sieve: connectivity must be 4 or 8, got {connectivity!r}")
    if int(passes) != passes or not 1 <= passes <= MAX_PASSES:
        raise ValueError(f"sieve: passes must be in 1..{MAX_PASSES}, got {passes!r}")
    if frozen_value is not None and not 0 <= int(frozen_value) <= 255:
        raise ValueError(f"sieve: frozen_value must be None or in 0..255, got {frozen_value!r}")


def _neighbour_pairs(H: int, W: int, connectivity: int):
    """(a, b) index arrays [H, W] slices of every neighbour pair, each pair once."""
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    pairs = [(idx[:, 1:], idx[:, :-1]), (idx[1:, :], idx[:-1, :])]
    if connectivity == 8:
        pairs += [(idx[1:, 1:], idx[:-1, :-1]), (idx[1:, :-1], idx[:-1, 1:])]
    return [(a.ravel(), b.ravel()) for a, b in pairs]


def label_components_host(m: np.ndarray, connectivity: int = 4) -> np.ndarray:
    """Connected components of a uint8 map [H, W] -> int32 [H, W].  A component is a maximal set of pixels of equal value
    connected through 4-neighbours (connectivity=4) or 8-neighbours (8); the label of a pixel is the smallest linear
    index y * W + x in its component.  The form is canonical, so two labellings compare bit for bit with no relabelling."""
    m = np.asarray(m)
    _check_map(m, connectivity)
    H, W = m.shape
    v = m.ravel()
    L = np.arange(H * W, dtype=np.int64)
    edges = [(a[v[a] == v[b]], b[v[a] == v[b]]) for a, b in _neighbour_pairs(H, W, connectivity)]
    while True:                                    # hook the larger root under the smaller label, then flatten
        changed = False
        for a, b in edges:
            la, lb = L[a], L[b]
            lo, hi = np.minimum(la, lb), np.maximum(la, lb)
            d = lo < hi
            if d.any():
                np.minimum.at(L, hi[d], lo[d])
                changed = True
        if not changed:
            break
        while True:
            L2 = L[L]
            if np.array_equal(L2, L):
                break
            L = L2
    return L.astype(np.int32).reshape(H, W)


def _sieve_pass_host(m: np.ndarray, min_pixels: int, connectivity: int, frozen: int) -> Tuple[np.ndarray, int, int]:
    H, W = m.shape
    v = m.ravel().astype(np.int64)
    L = label_components_host(m, connectivity).ravel().astype(np.int64)
    size = np.bincount(L, minlength=H * W).astype(np.int64)          # at the roots
    small = (size[L] < min_pixels) & (v != frozen)                     # per pixel: its component is small
    key = np.zeros(H * W, dtype=np.int64)                              # at the roots of small components; 0 = no donor
    for a, b in _neighbour_pairs(H, W, 4):                             # pixel edges, under both connectivities
        for k, d in ((a, b), (b, a)):                                  # k's component takes an offer from d's
            ok = small[k] & ~small[d] & (v[d] != frozen) & (v[k] != v[d])
            np.maximum.at(key, L[k[ok]], (size[L[d[ok]]] << 8) | (255 - v[d[ok]]))
    kp = key[L]
    out = np.where(kp > 0, 255 - (kp & 255), v).astype(np.uint8).reshape(H, W)
    return out, int(np.count_nonzero(key)), int(np.count_nonzero(kp))


def sieve_host(m: np.ndarray, min_pixels: int, connectivity: int = 4, frozen_value: Optional[int] = None,
               passes: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """The connected-component sieve -> (out uint8 [H, W], stats int64 [2]).  One pass:
      * components (label_components_host, `connectivity`) and their sizes s(K) are taken from the pass's input;
      * K is small when s(K) < min_pixels and its value is not frozen_value;
      * a donor of a small K is a component D that is not small, whose value is not frozen_value, and that shares a pixel
        edge with K (edge adjacency under both connectivities);
      * K takes the value of the donor with the greatest size, ties going to the smallest value; a small component with no
        donor keeps its value; frozen pixels never change and never donate;
      * stats[0] += the number of components re-valued, stats[1] += the number of pixels changed.
    passes = P (1..8) applies the pass P times, each on the previous result; the stats accumulate.  min_pixels <= 1 is a
    copy with zero stats.
    This rule is the project's own: every small component is decided at once from the pass's input, so the result does not
    depend on any order of visiting, which makes it simpler than GDAL's iterative merge (smallest polygons first, each
    into its largest neighbour, sizes growing as it goes).  Parity with gdal_sieve is unpinned: GDAL is not available
    to this project's tests."""
    m = np.asarray(m)
    _check_map(m, connectivity)
    check_sieve_options(min_pixels, connectivity, passes, frozen_value)
    out = m.copy()
    stats = np.zeros(2, dtype=np.int64)
    if min_pixels <= 1:
        return out, stats
    frozen = -1 if frozen_value is None else int(frozen_value)
    for _ in range(int(passes)):
        out, merged, changed = _sieve_pass_host(out, int(min_pixels), connectivity, frozen)
        stats += (merged, changed)
    return out, stats


# ---------------------------------------------------------------------------------------------------------- device side
_workspaces: Dict[Tuple[str, int], "object"] = {}        # (device type, index) -> uint8 workspace, grown on demand


def _workspace(device, nbytes: int):
    import torch
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _workspaces[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def _check_map_tensor(map_t, who: str):
    import torch
    if map_t.dim() != 2 or map_t.dtype != torch.uint8 or not map_t.is_cuda or not map_t.is_contiguous():
        raise ValueError(f"{who}: the map must be a contiguous uint8 [H, W] tensor on the GPU, got {map_t.dtype} "
                         f"{tuple(map_t.shape)} on {map_t.device}")
    H, W = int(map_t.shape[0]), int(map_t.shape[1])
    if H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"{who}: map {H}x{W} is empty or has more than 2^28 pixels")
    return H, W


def label_components(map_t, connectivity: int = 4):
    """label_components_host on a device tensor: uint8 [H, W] -> int32 [H, W] on the same device (fu_map_components, on
    the current stream), bit for bit."""
    import torch
    from . import _lib
    H, W = _check_map_tensor(map_t, "label_components")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    labels = torch.empty(H, W, dtype=torch.int32, device=map_t.device)
    with torch.cuda.device(map_t.device):
        _lib.check(_lib.load().fu_map_components(map_t.data_ptr(), H, W, int(connectivity), labels.data_ptr(),
                                                 torch.cuda.current_stream(map_t.device).cuda_stream))
    return labels


def sieve(map_t, min_pixels: int, connectivity: int = 4, frozen_value: Optional[int] = None, passes: int = 1, out=None,
          stats=None):
    """sieve_host on a device tensor: -> (out uint8 [H, W], stats int64 [2]), both on the map's device and bit-identical
    to the host statement's (fu_map_sieve, on the current stream; no host read).  out: where the result goes (default: a
    new tensor; the map itself for in place).  stats: a device int64 [2] the two counts are ADDED to (default: a new
    zeroed one).  The workspace (16 B per pixel) is cached per device and shared by the calls on it, which a stream
    orders; do not run two sieves on one device from different streams at once."""
    import torch
    from . import _lib
    H, W = _check_map_tensor(map_t, "sieve")
    check_sieve_options(min_pixels, connectivity, passes, frozen_value)
    if out is None:
        out = torch.empty_like(map_t)
    elif out.shape != map_t.shape or out.dtype != torch.uint8 or out.device != map_t.device or not out.is_contiguous():
        raise ValueError("sieve: out must be a contiguous uint8 tensor of the map's shape on the map's device")
    if stats is None:
        stats = torch.zeros(2, dtype=torch.int64, device=map_t.device)
    elif stats.shape != (2,) or stats.dtype != torch.int64 or stats.device != map_t.device:
        raise ValueError("sieve: stats must be an int64 [2] tensor on the map's device")
    lib = _lib.load()
    nbytes = int(lib.fu_sieve_workspace_bytes(H, W))
    ws = _workspace(map_t.device, nbytes)
    with torch.cuda.device(map_t.device):
        _lib.check(lib.fu_map_sieve(map_t.data_ptr(), out.data_ptr(), H, W, int(connectivity), int(min_pixels),
                                    -1 if frozen_value is None else int(frozen_value), int(passes), ws.data_ptr(), nbytes,
                                    stats.data_ptr(), torch.cuda.current_stream(map_t.device).cuda_stream))
    return out, stats
