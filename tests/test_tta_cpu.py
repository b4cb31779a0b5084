"""CPU: test-time augmentation's view codes (floodplanet_code_amd.tta) -- the eight views are the dihedral group D4 and
invert exactly, the named sets, view_codes' checks, the --tta option of predict, and the argument checks of the new C
entries that need no context."""
import ctypes
import itertools

import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd import predict as P
from floodplanet_code_amd import tta

CODES = range(8)


def _grid(h, w):
    return torch.arange(h * w).view(h, w)


def test_eight_codes_are_eight_distinct_permutations_that_invert():
    x = _grid(5, 5)
    views = [tta.apply_view(x, c) for c in CODES]
    for c, v in zip(CODES, views):
        assert sorted(v.reshape(-1).tolist()) == list(range(25))          # a permutation of the pixels
        assert torch.equal(tta.invert_view(v, c), x), c
    for a, b in itertools.combinations(CODES, 2):
        assert not torch.equal(views[a], views[b]), (a, b)
    y = torch.randn(2, 3, 6, 6)                                           # batch and class dims are carried along
    for c in CODES:
        assert torch.equal(tta.invert_view(tta.apply_view(y, c), c), y)
    z = torch.randn(2, 4, 5)                                              # non-square: the flips invert too
    for c in tta.VIEW_SETS["flips"]:
        assert tta.apply_view(z, c).shape == z.shape
        assert torch.equal(tta.invert_view(tta.apply_view(z, c), c), z)


def _matrix(code):
    """The view as a 2x2 integer matrix on pixel coordinates centred on the tile (columns x, rows y): an independent
    statement of the contract's transpose -> flip(-1) -> flip(-2) order."""
    m = torch.eye(2, dtype=torch.int64)
    if code & 4:
        m = torch.tensor([[0, 1], [1, 0]]) @ m
    if code & 1:
        m = torch.tensor([[-1, 0], [0, 1]]) @ m
    if code & 2:
        m = torch.tensor([[1, 0], [0, -1]]) @ m
    return m


def test_composition_table_is_d4():
    x = _grid(6, 6)
    table = {}
    for a in CODES:
        for b in CODES:
            ab = tta.apply_view(tta.apply_view(x, a), b)
            hits = [c for c in CODES if torch.equal(tta.apply_view(x, c), ab)]
            assert len(hits) == 1, (a, b, hits)
            table[a, b] = hits[0]
    # the same table from the matrices: composition is closed, 0 is the identity, every view has an inverse
    mats = {c: _matrix(c) for c in CODES}
    for (a, b), c in table.items():
        assert torch.equal(mats[b] @ mats[a], mats[c]), (a, b, c)
    assert all(table[0, c] == c == table[c, 0] for c in CODES)
    assert all(any(table[a, b] == 0 for b in CODES) for a in CODES)
    assert any(table[a, b] != table[b, a] for a in CODES for b in CODES)  # not abelian: D4, not Z2^3
    # named elements: 3 = rot180, 5 / 6 = the two quarter turns, 4 = transpose, 7 = anti-transpose
    assert torch.equal(tta.apply_view(x, 3), torch.rot90(x, 2, (-2, -1)))
    assert {torch.equal(tta.apply_view(x, 5), torch.rot90(x, k, (-2, -1))) for k in (1, 3)} == {True, False}
    assert {torch.equal(tta.apply_view(x, 6), torch.rot90(x, k, (-2, -1))) for k in (1, 3)} == {True, False}
    assert not torch.equal(tta.apply_view(x, 5), tta.apply_view(x, 6))
    assert table[5, 5] == table[6, 6] == 3
    assert torch.equal(tta.apply_view(x, 4), x.t())
    assert torch.equal(tta.apply_view(x, 7), x.flip(0).flip(1).t())


def test_named_sets():
    assert tta.VIEW_SETS == {"hflip": (0, 1), "flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def test_view_codes_checks_shapes_and_codes():
    assert tta.view_codes("flips", 48, 64) == (0, 1, 2, 3)
    assert tta.view_codes("hflip", 48, 64) == (0, 1)
    assert tta.view_codes("d4", 64, 64) == tuple(range(8))
    assert tta.view_codes([5, 0, 3], 32, 32) == (5, 0, 3)
    with pytest.raises(ValueError, match="square"):
        tta.view_codes("d4", 48, 64)
    with pytest.raises(ValueError, match="square"):
        tta.view_codes([0, 6], 64, 48)
    with pytest.raises(ValueError, match="distinct"):
        tta.view_codes([1, 1], 32, 32)
    with pytest.raises(ValueError, match="0..7"):
        tta.view_codes([0, 8], 32, 32)
    with pytest.raises(ValueError, match="1..8"):
        tta.view_codes([], 32, 32)
    with pytest.raises(ValueError, match="unknown view set"):
        tta.view_codes("rot", 32, 32)


def test_cli_parses_tta_and_defaults_to_none():
    ap = P.build_parser()
    assert ap.parse_args(["e/checkpoints/m.ckpt", "--data_root", "d"]).tta is None
    for name in ("hflip", "flips", "d4"):
        assert ap.parse_args(["e/checkpoints/m.ckpt", "--data_root", "d", "--tta", name]).tta == name
    with pytest.raises(SystemExit):
        ap.parse_args(["e/checkpoints/m.ckpt", "--data_root", "d", "--tta", "rot45"])


def test_predict_rejects_d4_on_non_square_crops_before_any_work(tmp_path):
    cfg = dict(crop_height=48, crop_width=64, crop_stride=32)
    with pytest.raises(ValueError, match="square"):      # the data root does not exist: nothing was read or launched
        P.predict(cfg, str(tmp_path), str(tmp_path / "checkpoints" / "m.ckpt"), "floodplanet",
                  data_root=str(tmp_path / "missing"), tta="d4")


def test_new_entries_reject_a_null_context():
    lib = _lib.load()
    x = ctypes.c_void_p(16)
    srcs, chs, codes = (ctypes.c_void_p * 1)(x), (ctypes.c_int32 * 1)(2), (ctypes.c_int32 * 2)(0, 1)
    assert lib.fu_forward_views(None, srcs, chs, 1, 1, 2, codes, None, None) == _lib.FU_ERR_INVALID
    assert b"null context" in lib.fu_last_error()
    assert lib.fu_merge_views(None, None, None, -100, None, None) == _lib.FU_ERR_INVALID
    table = (_lib.FuStitchEntry * 1)()
    assert lib.fu_stitch_add_batch_probs(None, 1, table, None, 1, None) == _lib.FU_ERR_INVALID
    assert b"fu_stitch_add_batch_probs" in lib.fu_last_error()
