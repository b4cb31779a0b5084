"""CPU: the fp64 restatement that the GPU resampling tests compare against (tests/tools/resample_ref.py) is ATen's operator.

torch on the CPU in fp32 -- F.pad(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)) and its autograd --
must agree with the restatement elementwise within 8 * 2^-24 * mag on every shape the GPU tests use (mag = the same product on
absolute values).  The restatement has torch's float32 weights and sums in float64, so what is left is torch's own rounding:
one per weight product and one per add of four taps forward, up to sixteen scattered taps backward; torch alone measures at
most 3.8 (forward) and 5.0 (backward) * 2^-24 * mag on these shapes.  A restatement with another weight (a pure fp64 lambda is ~1e-5 away) fails this."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
from tools.resample_ref import (ROWS4, SHAPES, axis_matrix, axis_taps, rows4_workgroups, upsample_bwd_ref,   # noqa: E402
                                 upsample_ref, worst_ratio)

CAP = 8 * 2.0 ** -24


def torch_up(x, oh, ow):
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    dy, dx = oh - up.shape[2], ow - up.shape[3]
    return F.pad(up, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_is_aten_forward_and_backward(shape):
    B, C, H, W, oh, ow = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, H, W, generator=g, requires_grad=True)
    gy = torch.randn(B, C, oh, ow, generator=g)          # non-zero in the pad as well: autograd drops it there
    y = torch_up(x, oh, ow)
    y.backward(gy)
    ref, mag = upsample_ref(x.detach().numpy(), oh, ow)
    r_f = worst_ratio(y.detach().numpy(), ref, CAP * mag)
    bref, bmag = upsample_bwd_ref(gy.numpy(), H, W)
    r_b = worst_ratio(x.grad.numpy(), bref, CAP * bmag)
    print(f"{shape}: torch fp32 vs restatement, units of 2^-24 mag: fwd {8 * r_f:.2f} bwd {8 * r_b:.2f}")
    assert r_f <= 1 and r_b <= 1
    py0, px0 = (oh - 2 * H) // 2, (ow - 2 * W) // 2
    pad = np.ones((oh, ow), bool)
    pad[py0:py0 + 2 * H, px0:px0 + 2 * W] = False
    assert (ref[:, :, pad] == 0).all() and (mag[:, :, pad] == 0).all()


def test_wrong_restatements_are_not_aten():
    """The cap separates: torch misses it against the two deliberately wrong references of the GPU negative control."""
    B, C, H, W, oh, ow = SHAPES[3]
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, C, H, W, generator=g)
    y = torch_up(x, oh, ow).numpy().astype(np.float64)
    for kw in (dict(px0=2), dict(swap=True)):
        bad, bad_mag = upsample_ref(x.numpy(), oh, ow, **kw)
        assert (np.abs(y - bad) > CAP * bad_mag).any(), kw


def test_the_rows_meant_for_the_four_row_variant_reach_its_threshold():
    """Host arithmetic of launch_upsample2 (fu_resample.hip): ceil(outW * CV / 256) * ceil(outH / 4) * B >= 2048 selects
    k_upsample2<T, 4>.  The 16-bit runs double C on these rows, so CV (channel vectors per pixel) is 16 in every precision."""
    for shape in ROWS4:
        assert rows4_workgroups(shape, 4) >= 2048, shape
        B, C, H, W, oh, ow = shape
        assert rows4_workgroups((B, 2 * C, H, W, oh, ow), 8) == rows4_workgroups(shape, 4)
        assert oh % 4 != 0                                # the tail of the store loop
    assert (ROWS4[1][4] - 2 * ROWS4[1][2]) // 2 == 1      # py0 = 1 under four rows per thread
    assert all(c % 8 == 0 for _, c, *_ in SHAPES)


def test_axis_matrix_rows_and_columns():
    for n in range(1, 301):
        m = axis_matrix(n)
        i0, i1, l0, l1 = axis_taps(n)
        assert m.shape == (2 * n, n) and (m >= 0).all()
        assert l0.dtype == np.float32 and l1.dtype == np.float32
        assert (i0 >= 0).all() and (i1 <= n - 1).all() and ((i1 - i0) | 1 == 1).all()
        # the corners are copied (align_corners) and every row is a convex pair up to one float32 rounding of 1 - l1
        assert m[0, 0] == 1.0 and m[-1, -1] == 1.0
        assert np.abs(m.sum(1) - 1.0).max() <= 2.0 ** -24
        # the backward gathers a column: at most 4 output rows feed one input row, which is why the kernel's list of
        # UP_BWD_MAX = 6 entries per input index never overflows and why its bound counts 4 x 4 taps
        assert int((m != 0).sum(0).max()) <= 4, n
