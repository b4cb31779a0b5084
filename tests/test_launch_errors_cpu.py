"""Host-side error paths of the precision-dispatched launchers: they reject a bad shape before any HIP call, so the
library can be asked without a GPU."""
import pytest

from floodplanet_code_amd import _lib


@pytest.mark.parametrize("precision", [_lib.FU_F32, _lib.FU_BF16, _lib.FU_F16])
def test_maxpool_rejects_a_channel_count_off_the_vector_width(precision):
    lib = _lib.load()
    # C = 6 is a multiple of neither 4 (fp32) nor 8 (bf16 / fp16) channels per 16-byte vector
    status = lib.fu_op_maxpool2(precision, None, None, None, None, 1, 8, 8, 6, None)
    assert status == _lib.FU_ERR_INVALID
    assert b"maxpool: unsupported shape (C=6" in lib.fu_last_error()


def test_maxpool_rejects_an_unknown_precision():
    lib = _lib.load()
    assert lib.fu_op_maxpool2(7, None, None, None, None, 1, 8, 8, 8, None) == _lib.FU_ERR_INVALID
    assert b"unknown precision" in lib.fu_last_error()


# the resampling test hooks check every argument before their first HIP call.  The pointers are never dereferenced on a
# rejected call: any non-null value stands in for a device buffer.
RESAMPLE_HOOKS = ["fu_op_upsample2_bwd", "fu_op_depth_to_space", "fu_op_space_to_depth"]
FAKE = 0x1000
PRECISIONS = [_lib.FU_F32, _lib.FU_BF16, _lib.FU_F16]


@pytest.mark.parametrize("hook", RESAMPLE_HOOKS)
def test_resample_hooks_reject_an_unknown_precision(hook):
    lib = _lib.load()
    assert getattr(lib, hook)(7, FAKE, FAKE, 1, 4, 4, 8, 8, 8, None) == _lib.FU_ERR_INVALID
    assert b"unknown precision" in lib.fu_last_error()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("hook", RESAMPLE_HOOKS)
def test_resample_hooks_reject_null_pointers(hook, precision):
    lib = _lib.load()
    for a, b in ((None, FAKE), (FAKE, None)):
        assert getattr(lib, hook)(precision, a, b, 1, 4, 4, 8, 8, 8, None) == _lib.FU_ERR_INVALID
        assert hook.encode() + b": null argument" in lib.fu_last_error()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("hook", RESAMPLE_HOOKS)
def test_resample_hooks_reject_a_target_smaller_than_twice_the_source(hook, precision):
    lib = _lib.load()
    # outH = 7 < 2 * 4 would make the top pad offset negative (a read in front of the buffer); likewise outW
    for oh, ow in ((7, 8), (8, 7)):
        assert getattr(lib, hook)(precision, FAKE, FAKE, 1, 4, 4, 8, oh, ow, None) == _lib.FU_ERR_INVALID
        assert b"smaller than 2x the source" in lib.fu_last_error()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("hook", RESAMPLE_HOOKS)
def test_resample_hooks_reject_a_channel_count_off_the_vector_width(hook, precision):
    lib = _lib.load()
    # C = 6 is a multiple of neither 4 (fp32 rows, the shuffles in every precision) nor 8 (16-bit rows)
    assert getattr(lib, hook)(precision, FAKE, FAKE, 1, 4, 4, 6, 8, 8, None) == _lib.FU_ERR_INVALID
    assert b"C=6 is not a multiple of" in lib.fu_last_error()


@pytest.mark.parametrize("precision", [_lib.FU_BF16, _lib.FU_F16])
def test_upsample_bwd_16bit_needs_eight_channels_per_vector(precision):
    lib = _lib.load()
    assert lib.fu_op_upsample2_bwd(precision, FAKE, FAKE, 1, 4, 4, 12, 8, 8, None) == _lib.FU_ERR_INVALID
    assert b"C=12 is not a multiple of the 8 channels" in lib.fu_last_error()


# the head's test hooks likewise: precision, class count, the width rule of the head kernels (C = V, 2V, 4V, 8V or 16V with V
# = 4 fp32 / 8 16-bit channels per vector), null operands and empty shapes are answered before the first HIP call
def head_fwd(lib, precision, C=64, ncls=3, y=FAKE, w=FAKE, bias=FAKE, out=FAKE, a=None, b=None, B=1, H=4, W=4):
    return lib.fu_op_head_fwd(precision, y, a, b, w, bias, C, ncls, B, H, W, out, None, None)


def head_bwd(lib, precision, C=64, ncls=3, dl=FAKE, y=FAKE, w=FAKE, g=FAKE, dw=FAKE, db=FAKE, a=None, b=None, npix=16,
             sums=(None, None, None, None)):
    return lib.fu_op_head_bwd(precision, dl, y, a, b, w, C, ncls, npix, g, dw, db, *sums, None)


HEAD_HOOKS = {"fu_op_head_fwd": head_fwd, "fu_op_head_bwd": head_bwd}


@pytest.mark.parametrize("hook", HEAD_HOOKS)
def test_head_hooks_reject_an_unknown_precision(hook):
    lib = _lib.load()
    assert HEAD_HOOKS[hook](lib, 7) == _lib.FU_ERR_INVALID
    assert b"unknown precision" in lib.fu_last_error()


@pytest.mark.parametrize("precision,C", [(_lib.FU_F32, 24), (_lib.FU_BF16, 24), (_lib.FU_F16, 24), (_lib.FU_F32, 128),
                                         (_lib.FU_BF16, 256), (_lib.FU_F16, 256), (_lib.FU_F32, 0), (_lib.FU_BF16, 4),
                                         (_lib.FU_F32, -4)])
@pytest.mark.parametrize("hook", HEAD_HOOKS)
def test_head_hooks_reject_a_width_off_the_lane_rule(hook, precision, C):
    lib = _lib.load()
    # 24 = 6 (3) lanes per pixel: no power of two; 128 (fp32) and 256 (16-bit) = 32 lanes: more than a DPP row of 16
    assert HEAD_HOOKS[hook](lib, precision, C=C) == _lib.FU_ERR_INVALID
    msg = lib.fu_last_error()
    assert msg.startswith(hook.encode() + b": C must be") and f"(got {C})".encode() in msg


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("ncls", [0, 9, -1])
@pytest.mark.parametrize("hook", HEAD_HOOKS)
def test_head_hooks_reject_a_class_count_outside_1_to_8(hook, ncls, precision):
    lib = _lib.load()
    assert HEAD_HOOKS[hook](lib, precision, ncls=ncls) == _lib.FU_ERR_INVALID
    assert hook.encode() + b": n_classes must be 1..8" in lib.fu_last_error()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_head_hooks_reject_null_operands(precision):
    lib = _lib.load()
    for name in ("y", "w", "bias", "out"):
        assert head_fwd(lib, precision, **{name: None}) == _lib.FU_ERR_INVALID, name
        assert b"fu_op_head_fwd: null argument" in lib.fu_last_error()
    for name in ("dl", "y", "w", "g", "dw", "db"):
        assert head_bwd(lib, precision, **{name: None}) == _lib.FU_ERR_INVALID, name
        assert b"fu_op_head_bwd: null argument" in lib.fu_last_error()
    # the BatchNorm coefficients come as a pair, the four operands of the fused sums as a set, and the sums need the pair
    for hook in HEAD_HOOKS.values():
        for a, b in ((FAKE, None), (None, FAKE)):
            assert hook(lib, precision, a=a, b=b) == _lib.FU_ERR_INVALID
            assert b"bn_a and bn_b go together" in lib.fu_last_error()
    assert head_bwd(lib, precision, a=FAKE, b=FAKE, sums=(FAKE, FAKE, FAKE, None)) == _lib.FU_ERR_INVALID
    assert b"fu_op_head_bwd: mean, invstd, sum_gm and sum_gmx go together" in lib.fu_last_error()
    assert head_bwd(lib, precision, sums=(FAKE,) * 4) == _lib.FU_ERR_INVALID
    assert b"fu_op_head_bwd: the BatchNorm-backward sums need bn_a and bn_b" in lib.fu_last_error()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_head_hooks_reject_empty_shapes(precision):
    lib = _lib.load()
    for dims in (dict(B=0), dict(H=0), dict(W=0), dict(B=-1)):
        assert head_fwd(lib, precision, **dims) == _lib.FU_ERR_INVALID
        assert b"fu_op_head_fwd: empty shape" in lib.fu_last_error()
    for npix in (0, -5, 2 ** 31):
        assert head_bwd(lib, precision, npix=npix) == _lib.FU_ERR_INVALID
        assert b"fu_op_head_bwd: npix must be" in lib.fu_last_error()


def test_head_backward_sums_are_unsupported_in_fp32_before_any_hip_call():
    lib = _lib.load()
    assert head_bwd(lib, _lib.FU_F32, a=FAKE, b=FAKE, sums=(FAKE,) * 4) == _lib.FU_ERR_UNSUPPORTED
    assert b"fu_op_head_bwd: the head-backward kernel does not emit the sums in this precision" in lib.fu_last_error()
