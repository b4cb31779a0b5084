"""Test-time augmentation (TTA) over the symmetries of the square tile.

A view code c in 0..7 is a bit set: 1 = hflip (W axis), 2 = vflip (H axis), 4 = transpose (H <-> W, square tiles only).
The view of an image t is, in this order,

    if c & 4: t = t.transpose(-1, -2)
    if c & 1: t = t.flip(-1)
    if c & 2: t = t.flip(-2)

and the inverse applies the same three steps in reverse order.  Codes 0..7 are the eight elements of the dihedral group
D4: 3 = rot180, 5 and 6 = the two 90-degree rotations, 7 = anti-transpose.  The TTA prediction of a crop is the mean, in
view order, of invert_view(softmax(logits of the view), code) (HipUNet.forward_views / merge_views, include/floodunet.h).

apply_view / invert_view are the torch reference semantics; the device path never materialises a transformed batch.
"""
from __future__ import annotations

from typing import TYPE_CHECKING, List, Optional, Sequence, Tuple, Union

if TYPE_CHECKING:                    # annotations only: the views are tensor methods, and view_codes is host arithmetic
    import torch

HFLIP, VFLIP, TRANSPOSE = 1, 2, 4

VIEW_SETS = {
    "hflip": (0, 1),
    "flips": (0, 1, 2, 3),          # any tile shape
    "d4": (0, 1, 2, 3, 4, 5, 6, 7),  # square tiles only
}


def view_codes(spec: Union[str, Sequence[int]], H: int, W: int) -> Tuple[int, ...]:
    """A set name of VIEW_SETS or a list of codes -> validated tuple of codes for an H x W tile.  Raises ValueError for
    unknown names, codes outside 0..7, repeated codes, more than 8 views and transposing codes on a non-square tile."""
    if isinstance(spec, str):
        if spec not in VIEW_SETS:
            raise ValueError(f"unknown view set {spec!r}; known: {sorted(VIEW_SETS)}")
        codes = VIEW_SETS[spec]
    else:
        codes = tuple(int(c) for c in spec)
    if not 1 <= len(codes) <= 8:
        raise ValueError(f"1..8 views, got {len(codes)}")
    if any(c < 0 or c > 7 for c in codes):
        raise ValueError(f"view codes must lie in 0..7, got {list(codes)}")
    if len(set(codes)) != len(codes):
        raise ValueError(f"view codes must be distinct, got {list(codes)}")
    if H != W and any(c & TRANSPOSE for c in codes):
        raise ValueError(f"view codes {[c for c in codes if c & TRANSPOSE]} transpose the tile, which needs a square tile; "
                         f"got {H}x{W} (use 'flips' or 'hflip')")
    return tuple(codes)


def recorded(spec: Union[None, str, Sequence[int]], codes: Optional[Sequence[int]]) -> Union[None, str, List[int]]:
    """What a summary.json / metrics.json / calibration.json holds under "tta": None, the set's name, or the list of codes."""
    return spec if spec is None or isinstance(spec, str) else list(codes)


def apply_view(t: torch.Tensor, code: int) -> torch.Tensor:
    """View `code` of t (last two dimensions H, W)."""
    if code & TRANSPOSE:
        t = t.transpose(-1, -2)
    if code & HFLIP:
        t = t.flip(-1)
    if code & VFLIP:
        t = t.flip(-2)
    return t


def invert_view(t: torch.Tensor, code: int) -> torch.Tensor:
    """Inverse of apply_view: invert_view(apply_view(t, c), c) == t."""
    if code & VFLIP:
        t = t.flip(-2)
    if code & HFLIP:
        t = t.flip(-1)
    if code & TRANSPOSE:
        t = t.transpose(-1, -2)
    return t
