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
