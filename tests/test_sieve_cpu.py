"""CPU: the host statements of postprocess.py (label_components_host against scipy, sieve_host against hand-written
cases), infer's sieve options, and the new symbols in the header and the binding."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from floodplanet_code_amd import _lib
from floodplanet_code_amd import infer as I
from floodplanet_code_amd import postprocess as PP


def grid(text):
    """A map typed out as rows of digits ('.' = 0)."""
    rows = [r.strip() for r in text.strip().splitlines()]
    return np.array([[0 if c == "." else int(c) for c in r] for r in rows], dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape,n_values,seed", [((37, 45), 2, 0), ((64, 50), 4, 1), ((1, 40), 2, 2), ((40, 1), 3, 3),
                                                 ((70, 53), 2, 4)])
def test_labels_equal_scipy_partition_with_min_index_labels(shape, n_values, seed, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(seed)
    m = g.integers(0, n_values, shape).astype(np.uint8)
    got = PP.label_components_host(m, connectivity)
    assert got.dtype == np.int32 and got.shape == m.shape
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    part = np.zeros(shape, dtype=np.int64)             # scipy's partition, all values together
    n_parts = 0
    for v in np.unique(m):
        lab, n = ndi.label(m == v, structure=structure)
        part[lab > 0] = lab[lab > 0] + n_parts
        n_parts += n
    assert part.min() == 1
    idx = np.arange(m.size, dtype=np.int64)
    min_idx = np.full(n_parts + 1, m.size, dtype=np.int64)
    np.minimum.at(min_idx, part.ravel(), idx)
    np.testing.assert_array_equal(got.ravel(), min_idx[part.ravel()])      # same partition, min-index labels
    assert len(np.unique(got)) == n_parts


def test_labels_of_typed_out_maps():
    m = grid("""
        1.1
        .1.
        1.1""")
    np.testing.assert_array_equal(PP.label_components_host(m, 4), np.arange(9).reshape(3, 3))
    np.testing.assert_array_equal(PP.label_components_host(m, 8), [[0, 1, 0], [1, 0, 1], [0, 1, 0]])
    with pytest.raises(ValueError):
        PP.label_components_host(m, 6)
    with pytest.raises(ValueError):
        PP.label_components_host(m.astype(np.int32), 4)


# ------------------------------------------------------------------------------------------------------------ sieve
def test_tie_on_donor_size_goes_to_the_smaller_value():
    m = grid("""
        3337111
        3338111
        3337111
        3338111
        3337111""")
    want = grid("""
        3331111
        3331111
        3331111
        3331111
        3331111""")
    out, stats = PP.sieve_host(m, 2)
    np.testing.assert_array_equal(out, want)
    assert stats.dtype == np.int64 and stats.tolist() == [5, 5]
    m2 = m.copy()
    m2[:, 3] = 7                                        # one component of 5 pixels, small below 6
    out, stats = PP.sieve_host(m2, 6)
    np.testing.assert_array_equal(out, want)
    assert stats.tolist() == [1, 5]
    np.testing.assert_array_equal(PP.sieve_host(m2, 5)[0], m2)             # 5 pixels are not below 5


def test_the_greater_donor_wins_over_the_smaller_value():
    m = grid("""
        33337111
        33337111
        33337111
        33337111
        33337111""")
    out, stats = PP.sieve_host(m, 6)
    assert (out[:, 4] == 3).all() and stats.tolist() == [1, 5]
    np.testing.assert_array_equal(np.delete(out, 4, axis=1), np.delete(m, 4, axis=1))


def test_small_component_among_small_ones_waits_for_a_donor():
    m = grid("""
        .......
        .......
        ..111..
        ..121..
        ..111..
        .......
        .......""")
    after_1 = grid("""
        .......
        .......
        .......
        ...2...
        .......
        .......
        .......""")
    out, stats = PP.sieve_host(m, 9)
    np.testing.assert_array_equal(out, after_1)         # the centre's only neighbours were small: unchanged
    assert stats.tolist() == [1, 8]
    out, stats = PP.sieve_host(m, 9, passes=2)
    np.testing.assert_array_equal(out, np.zeros((7, 7), np.uint8))
    assert stats.tolist() == [2, 9]
    out3, stats3 = PP.sieve_host(m, 9, passes=3)        # nothing left to do
    np.testing.assert_array_equal(out3, out)
    assert stats3.tolist() == [2, 9]


def test_no_donor_even_after_more_passes():
    m = grid("""
        1122211
        1122211
        3332211
        3332211
        3332211""")
    for passes in (1, 2, 8):
        out, stats = PP.sieve_host(m, 36, passes=passes)                   # every component is small
        np.testing.assert_array_equal(out, m)
        assert stats.tolist() == [0, 0]


def test_frozen_pixels_neither_change_nor_donate():
    m = grid("""
        ....99999
        .9..99999
        ...599999
        ....99499
        ....99999
        ....99999""")
    unfrozen = grid("""
        ....99999
        ....99999
        ...999999
        ....99999
        ....99999
        ....99999""")
    frozen = grid("""
        ....99999
        .9..99999
        ....99999
        ....99499
        ....99999
        ....99999""")
    out, stats = PP.sieve_host(m, 3)
    np.testing.assert_array_equal(out, unfrozen)        # the 9s are the largest component
    assert stats.tolist() == [3, 3]
    out, stats = PP.sieve_host(m, 3, frozen_value=9)
    np.testing.assert_array_equal(out, frozen)          # the 5 goes to the 0s, the lone 9 stays, the 4 has no donor
    assert stats.tolist() == [1, 1]


def test_diagonal_contact_joins_under_8_only():
    m = grid("""
        .......
        .1.....
        ..1....
        .......
        .......""")
    out, stats = PP.sieve_host(m, 2, connectivity=4)
    np.testing.assert_array_equal(out, np.zeros((5, 7), np.uint8))
    assert stats.tolist() == [2, 2]
    out, stats = PP.sieve_host(m, 2, connectivity=8)
    np.testing.assert_array_equal(out, m)
    assert stats.tolist() == [0, 0]
    out, stats = PP.sieve_host(m, 3, connectivity=8)    # one component of two pixels; its donor comes across edges
    np.testing.assert_array_equal(out, np.zeros((5, 7), np.uint8))
    assert stats.tolist() == [1, 2]


@pytest.mark.parametrize("min_pixels", [0, 1])
def test_min_pixels_one_is_the_identity(min_pixels):
    m = np.random.default_rng(5).integers(0, 3, (9, 9)).astype(np.uint8)
    out, stats = PP.sieve_host(m, min_pixels, passes=3)
    np.testing.assert_array_equal(out, m)
    assert out is not m and stats.tolist() == [0, 0]


@pytest.mark.parametrize("kw", [dict(min_pixels=-1), dict(min_pixels=2.5), dict(min_pixels=2, connectivity=6),
                                dict(min_pixels=2, passes=0), dict(min_pixels=2, passes=9),
                                dict(min_pixels=2, frozen_value=256)])
def test_sieve_host_rejects_bad_options(kw):
    with pytest.raises(ValueError):
        PP.sieve_host(np.zeros((3, 3), np.uint8), **kw)


# ------------------------------------------------------------------------------------------------------------ infer
def test_infer_parser_accepts_and_validates_the_sieve_options():
    ap = I.build_parser()
    base = ["x/checkpoints/a.ckpt", "scenes", "--out_dir", "out"]
    a = ap.parse_args(base)
    assert a.sieve is None and a.sieve_connectivity == 4 and a.sieve_passes == 1
    a = ap.parse_args(base + ["--sieve", "25", "--sieve_connectivity", "8", "--sieve_passes", "3"])
    assert (a.sieve, a.sieve_connectivity, a.sieve_passes) == (25, 8, 3)
    for bad in (["--sieve", "x"], ["--sieve_connectivity", "6"], ["--sieve_passes", "0"], ["--sieve_passes", "9"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + bad)
    text = re.sub(r"\s+", "", ap.format_help())         # argparse wraps at blanks and hyphens
    assert "--sieveN" in text and "un-sieved" in text


@pytest.mark.parametrize("kw", [dict(sieve=-3), dict(sieve=5, sieve_connectivity=6), dict(sieve=5, sieve_passes=0),
                                dict(sieve=5, sieve_passes=9)])
def test_infer_rejects_sieve_options_before_any_other_work(kw, tmp_path):
    with pytest.raises(ValueError, match="sieve"):      # no checkpoint, no inputs: the options are looked at first
        I.infer(str(tmp_path / "exp" / "checkpoints" / "none.ckpt"), [str(tmp_path / "nothing")], str(tmp_path / "out"),
                **kw)
    assert not os.path.exists(tmp_path / "out")


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_header_and_binding_name_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "floodunet.h")).read()
    assert int(re.search(r"#define\s+FU_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5      # additive: no version bump
    lib = _lib.load()
    for name in ("fu_sieve_workspace_bytes", "fu_map_components", "fu_map_sieve"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.fu_sieve_workspace_bytes(1024, 1024) == 16 << 20 and lib.fu_sieve_workspace_bytes(3, 5) == 240
    assert lib.fu_sieve_workspace_bytes(0, 5) == 0 and lib.fu_sieve_workspace_bytes(1 << 15, 1 << 14) == 0
