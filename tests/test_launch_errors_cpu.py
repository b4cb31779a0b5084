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
