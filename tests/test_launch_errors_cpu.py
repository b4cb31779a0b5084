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


# the BatchNorm test hooks and the max-pool hook likewise: every check comes before the first allocation or HIP call
def bn_bwd(lib, precision, C=64, B=1, H=4, W=4, g=FAKE, y=FAKE, a=FAKE, b=FAKE, mean=FAKE, invstd=FAKE, g_pool=None,
           dgamma=FAKE, dbeta=FAKE, ext=None, rows=0, dl=None, w=None, ncls=0, two_level=0):
    return lib.fu_op_bn_bwd_ex(precision, g, y, C, B, H, W, a, b, mean, invstd, g_pool, dgamma, dbeta, ext, rows, dl, w, ncls,
                               None, None, None, two_level, None)


def bn_stats(lib, partials=FAKE, n_part=4, C=8, count=64, gamma=FAKE, beta=FAKE, mean=FAKE, invstd=FAKE, a=FAKE, b=FAKE,
             rmean=None, rvar=None):
    return lib.fu_op_bn_stats(partials, n_part, C, count, None, gamma, beta, 1e-5, 0.1, mean, invstd, a, b, rmean, rvar, None,
                              None)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C", [0, 2, 6, -4, 1028, 2048])
def test_bn_backward_hooks_reject_a_bad_channel_count_and_survive(precision, C):
    lib = _lib.load()
    # C < 4 used to end the process with SIGFPE in bn_bwd_partial_elems (256 / (C >> 2)); C = 6 reached hipMalloc first
    assert bn_bwd(lib, precision, C=C) == _lib.FU_ERR_INVALID
    assert b"fu_op_bn_bwd: channels must be a multiple of 4 in 4..1024" in lib.fu_last_error()
    assert lib.fu_op_bn_bwd(precision, FAKE, FAKE, C, 1, 4, 4, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, None) == _lib.FU_ERR_INVALID
    assert b"fu_op_bn_bwd: channels must be a multiple of 4 in 4..1024" in lib.fu_last_error()


@pytest.mark.parametrize("C", [0, 2, 6])
def test_bn_stats_hook_takes_any_positive_channel_count_but_not_zero(C):
    lib = _lib.load()
    # the forward has a form for every C >= 1 (two-level when C % 4 != 0); C = 0, and nulls at C = 2 and 6, are answered on the host
    if C == 0:
        assert bn_stats(lib, C=0) == _lib.FU_ERR_INVALID
        assert b"fu_op_bn_stats: n_part, C and count must be >= 1" in lib.fu_last_error()
    else:
        assert bn_stats(lib, C=C, partials=None) == _lib.FU_ERR_INVALID
        assert b"fu_op_bn_stats: null argument" in lib.fu_last_error()


def test_bn_stats_hook_rejects_bad_calls():
    lib = _lib.load()
    for name in ("partials", "gamma", "beta", "mean", "invstd", "a", "b"):
        assert bn_stats(lib, **{name: None}) == _lib.FU_ERR_INVALID, name
        assert b"fu_op_bn_stats: null argument" in lib.fu_last_error()
    for rm, rv in ((FAKE, None), (None, FAKE)):
        assert bn_stats(lib, rmean=rm, rvar=rv) == _lib.FU_ERR_INVALID
        assert b"rmean and rvar go together" in lib.fu_last_error()
    for bad in (dict(n_part=0), dict(C=0), dict(count=0), dict(n_part=-1), dict(C=-8)):
        assert bn_stats(lib, **bad) == _lib.FU_ERR_INVALID, bad
        assert b"must be >= 1" in lib.fu_last_error()


def test_bn_backward_hook_rejects_an_unknown_precision():
    lib = _lib.load()
    assert bn_bwd(lib, 7) == _lib.FU_ERR_INVALID
    assert b"unknown precision" in lib.fu_last_error()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bn_backward_hook_rejects_nulls_partial_groups_and_empty_shapes(precision):
    lib = _lib.load()
    for name in ("g", "y", "a", "b", "mean", "invstd", "dgamma", "dbeta"):
        assert bn_bwd(lib, precision, **{name: None}) == _lib.FU_ERR_INVALID, name
        assert b"fu_op_bn_bwd: null argument" in lib.fu_last_error()
    for ext, rows in ((FAKE, 0), (None, 3), (FAKE, -1)):
        assert bn_bwd(lib, precision, ext=ext, rows=rows) == _lib.FU_ERR_INVALID
        assert b"external sums and their row count go together" in lib.fu_last_error()
    for dl, w in ((FAKE, None), (None, FAKE)):
        assert bn_bwd(lib, precision, dl=dl, w=w, ncls=2, ext=FAKE, rows=1) == _lib.FU_ERR_INVALID
        assert b"head_dl and head_w go together" in lib.fu_last_error()
    for dims in (dict(B=0), dict(H=0), dict(W=0), dict(H=-2)):
        assert bn_bwd(lib, precision, **dims) == _lib.FU_ERR_INVALID
        assert b"fu_op_bn_bwd: empty shape" in lib.fu_last_error()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bn_backward_hook_rejects_what_the_pooled_and_head_routes_cannot_do(precision):
    lib = _lib.load()
    assert bn_bwd(lib, precision, C=12, g_pool=FAKE) == _lib.FU_ERR_INVALID          # 256 % 3 != 0
    assert b"(pooled): C / 4 must divide 256" in lib.fu_last_error()
    assert bn_bwd(lib, precision, g_pool=FAKE, ext=FAKE, rows=2) == _lib.FU_ERR_INVALID
    assert b"(pooled): neither external sums nor a recomputed head gradient" in lib.fu_last_error()
    head = dict(dl=FAKE, w=FAKE, ncls=2, ext=FAKE, rows=1)
    if precision == _lib.FU_F32:
        assert bn_bwd(lib, precision, **head) == _lib.FU_ERR_INVALID
        assert b"(head): 16-bit precisions only" in lib.fu_last_error()
        return
    for C in (12, 24, 520):                                                           # off the vector; 256 % 3; 256 % 65
        assert bn_bwd(lib, precision, C=C, **head) == _lib.FU_ERR_INVALID, C
        assert b"(head): C / 8 must divide 256" in lib.fu_last_error()
    for ncls in (0, 9, -1):
        assert bn_bwd(lib, precision, **dict(head, ncls=ncls)) == _lib.FU_ERR_INVALID
        assert b"(head): n_classes must be 1..8" in lib.fu_last_error()
    assert bn_bwd(lib, precision, dl=FAKE, w=FAKE, ncls=2) == _lib.FU_ERR_INVALID
    assert b"(head): the recomputed head gradient needs the external sums" in lib.fu_last_error()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_maxpool_hook_rejects_nulls_half_a_prologue_and_maps_without_a_window(precision):
    lib = _lib.load()
    for src, dst in ((None, FAKE), (FAKE, None)):
        assert lib.fu_op_maxpool2(precision, src, None, None, dst, 1, 8, 8, 8, None) == _lib.FU_ERR_INVALID
        assert b"fu_op_maxpool2: null argument" in lib.fu_last_error()
    for a, b in ((FAKE, None), (None, FAKE)):
        assert lib.fu_op_maxpool2(precision, FAKE, a, b, FAKE, 1, 8, 8, 8, None) == _lib.FU_ERR_INVALID
        assert b"bn_a and bn_b go together" in lib.fu_last_error()
    for B, H, W in ((1, 1, 8), (1, 8, 1), (0, 8, 8), (1, 0, 8)):       # H = 1 used to ask for a grid with a zero dimension
        assert lib.fu_op_maxpool2(precision, FAKE, None, None, FAKE, B, H, W, 8, None) == _lib.FU_ERR_INVALID
        assert b"fu_op_maxpool2: no complete 2x2 window" in lib.fu_last_error()
