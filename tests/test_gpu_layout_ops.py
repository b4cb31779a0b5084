"""GPU: the layout, gather and channel-copy kernels of fu_layout.hip on their own, through their fu_op_* test hooks, bit for bit
against tests/tools/layout_ref.py (pinned to torch's CPU casts and indexing by tests/test_layout_ref_cpu.py) -- never against
another run of the code under test.  These are index-and-round operations: every comparison is torch.equal on the integer view
of the bits.  The one thing forgiven is a NaN's payload; +0.0 and -0.0 differ.

GUARD BANDS.  Every destination lies between two bands of 64 elements (a multiple of 16 bytes: the destination keeps its
alignment), and bands and destination are filled beforehand with a sentinel no result can equal (a negative NaN with a payload
of its own; the inputs' only NaN is positive).  After the call both bands are untouched, every element the operation owns is
overwritten (compared raw with the sentinel, no NaN forgiveness), the padding channels hold +0.0 bits, and for copy_channels
the channels outside the window still hold the sentinel.

WHAT REACHES WHAT in fu_layout.hip:
  k_nchw_to_nhwc<T>              fp32 at every shape; 16-bit at c_pad % 8 != 0; 2 x 9 x 300 x 300 x 12 > 8192 * 256 elements: a
                                 second trip of the grid-stride loop; ElemIO<T>::store1
  k_nchw_to_nhwc_v8<T>           16-bit, c_pad % 8 == 0: C / c_pad in 1/8, 7/8, 8/8, 9/16, 12/16 (an octet partly, wholly and not
                                 at all padding), H * W of 221, 256, 323 (under one block, exactly one, a ragged second), B 1 / 3
  src_channels / offset          windows [0, 8) and [8, 10) of 10 channels and [5, 12) of 12, through both kernels
  k_nhwc_to_nchw<T>              the same C / c_pad pairs, NaN in the source's padding channels
  k_gather_nchw_to_nhwc<T>       splits (10), (8, 1, 1), (5, 6), (3, 2) and 8 x 1, the whole concatenation and windows that start
                                 and end inside a source (source boundaries inside a 4- / 8-channel vector), c_pad at and above
                                 the rounded-up C (whole vectors of padding), H * W 221 / 323, B 2
  k_gather_views_nchw_to_nhwc<T> all eight codes at 17 x 17, the flips at 13 x 17 and 19 x 17, 1 / 3 / 8 views in unsorted order
                                 (the 3-bit packing), B 2 (n = v * B + b), two sources with ch_off != 0; code 0 == plain gather
  k_copy_channels<T, V>          window at the start, the end and the middle of source / destination, npix 1, 255, 4099, plain
                                 and with relu(a * x + b) (a negative, zero and positive, b of both signs)
  k_center_to_w3 / _from_w3      n 1, 7, 4096 and beyond one trip of the capped grid (4096 * 256 threads)
Unreached: the 64-bit index range (tensors of 2^31 elements and more).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_layout_ref_cpu import bad_hook_calls          # noqa: E402
from tools import layout_ref as L                       # noqa: E402

from floodplanet_code_amd import _lib                   # noqa: E402
from floodplanet_code_amd._lib import check             # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
BAND = 64
CODE = {"fp32": _lib.FU_F32, "bf16": _lib.FU_BF16, "fp16": _lib.FU_F16}
IDT = {"fp32": torch.int32, "bf16": torch.int16, "fp16": torch.int16}            # the integer view of the bits
NPI = {"fp32": np.int32, "bf16": np.int16, "fp16": np.int16}
# a negative NaN with a payload of its own in every type
SENTINEL = {"fp32": int(np.uint32(0xFFA5A5A5).view(np.int32)), "bf16": int(np.uint16(0xFFA5).view(np.int16)),
            "fp16": int(np.uint16(0xFFA5).view(np.int16))}
NAN_FIELDS = {"fp32": (0x7F800000, 0x007FFFFF, 0x7FC00000), "bf16": (0x7F80, 0x007F, 0x7FC0), "fp16": (0x7C00, 0x03FF, 0x7E00)}
SIXTEEN = ("bf16", "fp16")
PAIRS = [(1, 8), (7, 8), (8, 8), (9, 16), (12, 16)]                               # C, c_pad
HWS = [(13, 17), (16, 16), (17, 19)]                                              # 221, 256, 323 pixels


def stream():
    return torch.cuda.current_stream().cuda_stream


def signed(bits, prec):
    """numpy raw codes (uint) -> the int tensor torch compares"""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=L.BITS_DTYPE[prec]).reshape(-1).view(NPI[prec]))


def dev_f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).to(DEV)


def dev_bits(bits, prec):
    return signed(bits, prec).to(DEV)


class Guarded:
    """n elements of `prec` on the device between two bands, all of it sentinel (or `fill` in the middle)"""

    def __init__(self, n, prec):
        self.n, self.prec = n, prec
        self.t = torch.full((n + 2 * BAND,), SENTINEL[prec], dtype=IDT[prec], device=DEV)
        assert (BAND * self.t.element_size()) % 16 == 0 and self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + BAND * self.t.element_size()

    def read(self):
        torch.cuda.synchronize()
        return self.t.cpu()


def canonical(t, prec):
    """int codes with every NaN replaced by one code: the payload is the one thing forgiven"""
    exp, man, nan = NAN_FIELDS[prec]
    return t.masked_fill(((t & exp) == exp) & ((t & man) != 0), nan)


def failures(buf, want, prec, owned=None):
    """The one check of this file.  buf: the whole guarded buffer read back (int tensor); want: raw codes of everything
    between the bands; owned: mask of the elements the operation writes (default: all of them).  -> list of complaints."""
    want = signed(want, prec)
    n = want.numel()
    assert buf.numel() == n + 2 * BAND and buf.dtype == want.dtype
    band = torch.full((BAND,), SENTINEL[prec], dtype=IDT[prec])
    lo, mid, hi = buf[:BAND], buf[BAND:BAND + n], buf[BAND + n:]
    out = []
    if not torch.equal(lo, band):
        out.append(f"the band in front was written at {torch.nonzero(lo != band).flatten().tolist()[:8]}")
    if not torch.equal(hi, band):
        out.append(f"the band behind was written at {torch.nonzero(hi != band).flatten().tolist()[:8]}")
    own = torch.ones(n, dtype=torch.bool) if owned is None else torch.from_numpy(np.ascontiguousarray(owned).reshape(-1))
    if bool((mid[own] == SENTINEL[prec]).any()):
        out.append(f"{int((mid[own] == SENTINEL[prec]).sum())} owned elements were not written")
    if not torch.equal(mid[~own], want[~own]):                       # raw: the sentinel is a NaN, and must still be that NaN
        out.append("an element outside the window was written")
    g, w = canonical(mid, prec), canonical(want, prec)
    if not torch.equal(g, w):
        bad = torch.nonzero(g != w).flatten()
        out.append(f"{bad.numel()} of {n} elements differ, first at {bad[:8].tolist()}: got "
                   f"{[hex(int(v) & 0xFFFFFFFF) for v in mid[bad[:8]]]} want {[hex(int(v) & 0xFFFFFFFF) for v in want[bad[:8]]]}")
    return out


def passes(buf, want, prec, owned=None):
    bad = failures(buf, want, prec, owned)
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------------------
# the hooks
# ----------------------------------------------------------------------------------------------------------------------
def run_to_nhwc(prec, xd, B, C_, H, W, c_pad, srcC=0, off=0, hook="window"):
    dst = Guarded(B * H * W * c_pad, prec)
    lib = _lib.load()
    if hook == "window":
        check(lib.fu_op_nchw_to_nhwc_window(CODE[prec], xd.data_ptr(), dst.ptr, B, C_, H, W, c_pad, srcC, off, stream()))
    else:
        assert srcC == 0 and off == 0
        check(lib.fu_op_nchw_to_nhwc(CODE[prec], xd.data_ptr(), dst.ptr, B, C_, H, W, c_pad, stream()))
    return dst.read()


def run_gather(prec, srcs_d, B, C_, H, W, c_pad, off, codes=None):
    n = len(srcs_d)
    ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in srcs_d])
    chans = (C.c_int32 * n)(*[s.shape[1] for s in srcs_d])
    nv = 0 if codes is None else len(codes)
    vc = None if codes is None else (C.c_int32 * nv)(*codes)
    dst = Guarded(max(nv, 1) * B * H * W * c_pad, prec)
    check(_lib.load().fu_op_gather_nchw_to_nhwc(CODE[prec], ptrs, chans, n, dst.ptr, B, C_, H, W, c_pad, off, nv, vc, stream()))
    return dst.read()


def round_up(a, b):
    return -(-a // b) * b


# ----------------------------------------------------------------------------------------------------------------------
# NCHW -> NHWC
# ----------------------------------------------------------------------------------------------------------------------
FLAT = [("fp32", (1, 1, 1, 1, 4)), ("fp32", (2, 9, 13, 17, 12)), ("fp32", (3, 4, 16, 16, 4)), ("fp32", (2, 9, 300, 300, 12)),
        ("bf16", (2, 3, 13, 17, 4)), ("fp16", (2, 3, 13, 17, 4))]


@pytest.mark.parametrize("prec,shape", FLAT, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_flat_kernel(prec, shape):
    """k_nchw_to_nhwc<T>; the 300 x 300 case makes every thread of the capped grid take a second trip"""
    B, C_, H, W, c_pad = shape
    assert prec == "fp32" or c_pad % 8 != 0                 # else launch_nchw_to_nhwc takes the octet kernel
    if H == 300:
        assert B * H * W * c_pad > 8192 * 256
    x = L.edge_input((B, C_, H, W), 100)
    xd = dev_f32(x)
    want = L.nchw_to_nhwc(x, C_, c_pad, prec)
    for hook in ("window", "whole"):                        # fu_op_nchw_to_nhwc_window and fu_op_nchw_to_nhwc: one launcher
        passes(run_to_nhwc(prec, xd, B, C_, H, W, c_pad, hook=hook), want, prec)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}of{p[1]}")
@pytest.mark.parametrize("prec", SIXTEEN)
def test_octet_kernel(prec, pair):
    """k_nchw_to_nhwc_v8<T>: the 16-bit training path"""
    C_, c_pad = pair
    for (H, W) in HWS:
        for B in (1, 3):
            x = L.edge_input((B, C_, H, W), 110 + B)
            passes(run_to_nhwc(prec, dev_f32(x), B, C_, H, W, c_pad), L.nchw_to_nhwc(x, C_, c_pad, prec), prec)


@pytest.mark.parametrize("prec", L.PRECS)
def test_channel_window(prec):
    """src_channels / src_channel_offset, as forward_impl passes them for every encoder of a late-fusion net: c_pad % 8 == 0
    takes the octet kernel in the 16-bit types, the other c_pad the flat one"""
    B, H, W = 2, 17, 19
    for srcC, lo, hi in ((10, 0, 8), (10, 8, 10), (12, 5, 12)):
        x = L.edge_input((B, srcC, H, W), 120 + lo)
        xd = dev_f32(x)
        C_ = hi - lo
        for c_pad in (round_up(C_, 8), round_up(C_, 8) + 4):
            passes(run_to_nhwc(prec, xd, B, C_, H, W, c_pad, srcC, lo), L.nchw_to_nhwc(x, C_, c_pad, prec, lo), prec)


@pytest.mark.parametrize("prec", SIXTEEN)
def test_the_three_store_paths_round_alike(prec):
    """ElemIO::store1 (flat kernel), VecIO::store in the octet kernel and in the gather, on one input full of ties, fp16
    subnormals and overflow: the same bits (each also equals the reference, by the tests around this one)"""
    B, C_, H, W = 2, 3, 13, 17
    x = np.resize(np.asarray(L.EDGES, dtype=f32), (B, C_, H, W)).copy()      # nothing but edge values
    xd = dev_f32(x)
    flat = run_to_nhwc(prec, xd, B, C_, H, W, 4)[BAND:-BAND].view(B * H * W, 4)[:, :C_]
    octet = run_to_nhwc(prec, xd, B, C_, H, W, 8)[BAND:-BAND].view(B * H * W, 8)[:, :C_]
    gath = run_gather(prec, [xd], B, C_, H, W, 8, 0)[BAND:-BAND].view(B * H * W, 8)[:, :C_]
    want = signed(L.nchw_to_nhwc(x, C_, C_, prec), prec).view(B * H * W, C_)
    for got in (flat, octet, gath):
        assert torch.equal(canonical(got, prec), canonical(want, prec))
    assert torch.equal(canonical(flat, prec), canonical(octet, prec)) and torch.equal(canonical(octet, prec), canonical(gath, prec))


# ----------------------------------------------------------------------------------------------------------------------
# NHWC -> NCHW
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}of{p[1]}")
@pytest.mark.parametrize("prec", L.PRECS)
def test_nhwc_to_nchw(prec, pair):
    """k_nhwc_to_nchw<T>; the source's padding channels hold NaN, which must not leak"""
    C_, c_pad = pair
    lib = _lib.load()
    for (H, W) in (HWS[0], HWS[2]):
        for B in (1, 3):
            src = L.to_bits(L.edge_input((B, H, W, c_pad), 130 + B), prec)
            src[..., C_:] = L.to_bits(f32(np.nan), prec).reshape(-1)[0]
            sd = dev_bits(src, prec)
            dst = Guarded(B * C_ * H * W, "fp32")
            check(lib.fu_op_nhwc_to_nchw(CODE[prec], sd.data_ptr(), dst.ptr, B, C_, H, W, c_pad, stream()))
            passes(dst.read(), L.nhwc_to_nchw(src, C_, prec), "fp32")


# ----------------------------------------------------------------------------------------------------------------------
# gathers
# ----------------------------------------------------------------------------------------------------------------------
# split -> windows (ch_off, C): the whole concatenation, and one that starts and ends inside a source
SPLITS = {(10,): [(0, 10), (3, 5)], (8, 1, 1): [(0, 10), (5, 4), (7, 3)], (5, 6): [(0, 11), (3, 6)], (3, 2): [(0, 5), (1, 3)],
          (1,) * 8: [(0, 8), (2, 5)]}


@pytest.mark.parametrize("split", list(SPLITS), ids=lambda s: "+".join(map(str, s)))
@pytest.mark.parametrize("prec", L.PRECS)
def test_plain_gather(prec, split):
    """k_gather_nchw_to_nhwc<T>"""
    B, V = 2, L.VEC[prec]
    for (H, W) in (HWS[0], HWS[2]):
        srcs = [L.edge_input((B, c, H, W), 140 + k) for k, c in enumerate(split)]
        srcs_d = [dev_f32(s) for s in srcs]
        for off, C_ in SPLITS[split]:
            for c_pad in (round_up(C_, V), round_up(C_, V) + V):
                passes(run_gather(prec, srcs_d, B, C_, H, W, c_pad, off), L.gather(srcs, C_, c_pad, prec, off), prec)


ALL8 = (5, 0, 7, 2, 4, 1, 6, 3)
VIEW_CASES = [(17, 17, ALL8), (17, 17, (6, 1, 4)), (17, 17, (7,)), (17, 17, (0,)),
              (13, 17, (3, 0, 2)), (13, 17, (1,)), (19, 17, (2, 3, 1)), (19, 17, (0,)), (19, 17, (1, 3, 0, 2, 2, 1, 0, 3))]


@pytest.mark.parametrize("prec", L.PRECS)
def test_views_gather(prec):
    """k_gather_views_nchw_to_nhwc<T>: two sources of 5 and 6 channels, channels [3, 9) and the whole concatenation"""
    B, V = 2, L.VEC[prec]
    for H, W, codes in VIEW_CASES:
        srcs = [L.edge_input((B, 5, H, W), 150), L.edge_input((B, 6, H, W), 151)]
        srcs_d = [dev_f32(s) for s in srcs]
        for off, C_ in ((3, 6), (0, 11)):
            c_pad = round_up(C_, V)
            got = run_gather(prec, srcs_d, B, C_, H, W, c_pad, off, codes)
            passes(got, L.gather(srcs, C_, c_pad, prec, off, codes), prec)
            if codes == (0,):                               # the identity view is the plain gather, on the device's own bits
                assert torch.equal(got, run_gather(prec, srcs_d, B, C_, H, W, c_pad, off))


# ----------------------------------------------------------------------------------------------------------------------
# copy_channels
# ----------------------------------------------------------------------------------------------------------------------
COPIES = [(8, 0, 24, 8, 8), (24, 16, 8, 0, 8), (16, 8, 32, 24, 8)]               # srcC, src_off, dstC, dst_off, C


def copy_cases(prec):
    return COPIES + ([tuple(v // 2 for v in c) for c in COPIES] if prec == "fp32" else [])


def coefficients(C_, seed):
    """a with a zero, a negative and positive entries, b of both signs: the ReLU cuts some elements and not others"""
    rng = np.random.default_rng(seed)
    a = (rng.random(C_) + 0.5).astype(f32)
    b = (rng.standard_normal(C_) * 0.5).astype(f32)
    a[0], a[1] = 0.0, -1.25
    b[0], b[1], b[2], b[3] = 0.5, 0.25, -0.75, 0.125
    return a, b


def run_copy(prec, src_bits, src_off, dstC, dst_off, C_, a, b):
    npix, srcC = src_bits.shape
    sd = dev_bits(src_bits, prec)
    ad, bd = (None, None) if a is None else (dev_f32(a), dev_f32(b))
    dst = Guarded(npix * dstC, prec)
    check(_lib.load().fu_op_copy_channels(CODE[prec], sd.data_ptr(), srcC, src_off, None if a is None else ad.data_ptr(),
                                          None if a is None else bd.data_ptr(), dst.ptr, dstC, dst_off, C_, npix, stream()))
    return dst.read()


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bnrelu"])
@pytest.mark.parametrize("prec", L.PRECS)
def test_copy_channels(prec, bn):
    """k_copy_channels<T, V>: the late-fusion concat (with the producer's BN + ReLU) and the split of its gradient"""
    for srcC, src_off, dstC, dst_off, C_ in copy_cases(prec):
        a, b = coefficients(C_, 160) if bn else (None, None)
        for npix in (1, 255, 4099):
            src = L.to_bits(L.edge_input((npix, srcC), 161 + npix), prec)
            before = np.full((npix, dstC), SENTINEL[prec], dtype=NPI[prec]).view(L.BITS_DTYPE[prec])
            want = L.copy_channels(src, src_off, before, dst_off, C_, prec, a, b)
            owned = np.zeros((npix, dstC), bool)
            owned[:, dst_off:dst_off + C_] = True
            passes(run_copy(prec, src, src_off, dstC, dst_off, C_, a, b), want, prec, owned)
            if bn and npix > 1:                             # the ReLU cut some elements and kept others
                win = want[:, dst_off:dst_off + C_]
                assert (win == 0).any() and (win != 0).any()


# ----------------------------------------------------------------------------------------------------------------------
# centre tap
# ----------------------------------------------------------------------------------------------------------------------
TRIP = 4096 * 256                                           # threads of the capped grid of the two centre-tap kernels


@pytest.mark.parametrize("n", [1, 7, 4096, TRIP // 9 + 100, TRIP + 5])
def test_centre_tap(n):
    lib = _lib.load()
    dw3 = L.edge_input((n * 9,), 170)
    keep = dw3.reshape(n, 9)[:, 4].copy()
    dw3[:] = np.nan                                         # every other tap: NaN, which must not leak
    dw3.reshape(n, 9)[:, 4] = keep
    d3 = dev_f32(dw3)
    dst = Guarded(n, "fp32")
    check(lib.fu_op_center_from_w3(d3.data_ptr(), n, dst.ptr, stream()))
    passes(dst.read(), L.center_from_w3(dw3), "fp32")
    if n > TRIP:                                            # center_to_w3's second trip starts at n * 9 > 4096 * 256
        return
    w = L.edge_input((n,), 171)
    wd = dev_f32(w)
    dst3 = Guarded(n * 9, "fp32")
    check(lib.fu_op_center_to_w3(wd.data_ptr(), n, dst3.ptr, stream()))
    got = dst3.read()
    passes(got, L.center_to_w3(w), "fp32")
    taps = got[BAND:-BAND].view(n, 9)
    assert bool((taps[:, [0, 1, 2, 3, 5, 6, 7, 8]] == 0).all())                  # all-zero bits off the centre
    assert torch.equal(canonical(taps[:, 4], "fp32"), canonical(signed(L.to_bits(w, "fp32"), "fp32"), "fp32"))


# ----------------------------------------------------------------------------------------------------------------------
# rejected calls, and the check itself
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", L.PRECS)
def test_rejected_calls_launch_nothing(prec):
    lib = _lib.load()
    buf = dev_f32(L.edge_input((4096,), 180))
    dst = Guarded(4096, prec)
    for what, call, msg in bad_hook_calls(lib, CODE[prec], buf.data_ptr(), dst.ptr):
        assert call() == _lib.FU_ERR_INVALID, what
        assert msg in lib.fu_last_error(), (what, lib.fu_last_error())
    assert bool((dst.read() == SENTINEL[prec]).all())       # bands and destination: nothing was launched
    # and a good call goes through: two sources of 3 + 2 channels, channels [1, 4), 4 x 5 pixels
    V = L.VEC[prec]
    srcs = [L.edge_input((2, 3, 4, 5), 181), L.edge_input((2, 2, 4, 5), 182)]
    got = run_gather(prec, [dev_f32(s) for s in srcs], 2, 3, 4, 5, V, 1)
    passes(got, L.gather(srcs, 3, V, prec, 1), prec)


@pytest.mark.parametrize("prec", L.PRECS)
def test_wrong_references_fail_the_same_check(prec):
    """Negative control: on the kernels' outputs, failures() is empty against the reference and not against one with a
    single deliberate defect -- one element one ulp of T off, one channel shifted by one, two view codes exchanged, a padding
    element -0.0 instead of +0.0, one guard-band element changed; for copy_channels also a write outside the window."""
    B, H, W, V = 2, 17, 17, L.VEC[prec]
    C_, c_pad, off, codes = 6, round_up(6, V) + V, 3, (6, 1, 4)
    srcs = [L.edge_input((B, 5, H, W), 190), L.edge_input((B, 6, H, W), 191)]
    srcs_d = [dev_f32(s) for s in srcs]
    got = run_gather(prec, srcs_d, B, C_, H, W, c_pad, off, codes)
    want = L.gather(srcs, C_, c_pad, prec, off, codes)
    assert not failures(got, want, prec)

    ulp = want.copy()
    flat = ulp.reshape(-1, c_pad)
    vals = np.abs(L.from_bits(flat[:, 1].copy(), prec))
    i = int(np.flatnonzero((vals > 0.01) & (vals < 100.0))[0])                               # an ordinary finite value
    flat[i, 1] += 1                                         # the next code: one ulp of T
    assert failures(got, ulp, prec)
    assert failures(got, L.gather(srcs, C_, c_pad, prec, off + 1, codes), prec)              # every channel one further
    shifted = want.copy()
    shifted[..., 2] = want[..., 3]                          # one channel takes its neighbour's values
    assert failures(got, shifted, prec)
    assert failures(got, L.gather(srcs, C_, c_pad, prec, off, (1, 6, 4)), prec)              # two view codes exchanged
    negz = want.copy()
    assert negz[0, 0, 0, C_] == 0
    negz[0, 0, 0, C_] = L.to_bits(f32(-0.0), prec).reshape(-1)[0]
    assert failures(got, negz, prec)
    for at in (BAND - 1, BAND + want.size, 0, got.numel() - 1):                              # one guard-band element changed
        touched = got.clone()
        touched[at] ^= 1
        assert failures(touched, want, prec)
    unwritten = got.clone()
    unwritten[BAND + 7] = SENTINEL[prec]                    # an owned element left as it was
    assert failures(unwritten, want, prec)

    # the same for the check with a window (copy_channels) and for the flat and octet conversions
    npix, srcC, src_off, dstC, dst_off, Cw = 255, 2 * V, V, 3 * V, V, V
    a, b = coefficients(Cw, 192)
    src = L.to_bits(L.edge_input((npix, srcC), 193), prec)
    before = np.full((npix, dstC), SENTINEL[prec], dtype=NPI[prec]).view(L.BITS_DTYPE[prec])
    owned = np.zeros((npix, dstC), bool)
    owned[:, dst_off:dst_off + Cw] = True
    gotc = run_copy(prec, src, src_off, dstC, dst_off, Cw, a, b)
    wantc = L.copy_channels(src, src_off, before, dst_off, Cw, prec, a, b)
    assert not failures(gotc, wantc, prec, owned)
    assert failures(gotc, L.copy_channels(src, src_off - 1, before, dst_off, Cw, prec, a, b), prec, owned)   # channel shift
    assert failures(gotc, L.copy_channels(src, src_off, before, dst_off, Cw, prec, np.roll(a, 1), np.roll(b, 1)), prec, owned)
    spill = gotc.clone()
    spill[BAND + dst_off + Cw] = gotc[BAND + dst_off]       # a write one element past the window
    assert failures(spill, wantc, prec, owned)
    nanspill = gotc.clone()
    nanspill[BAND] = NAN_FIELDS[prec][2]                    # another NaN outside the window is not forgiven
    assert failures(nanspill, wantc, prec, owned)
    x = L.edge_input((B, 7, H, W), 194)
    gotn = run_to_nhwc(prec, dev_f32(x), B, 7, H, W, 8)
    wantn = L.nchw_to_nhwc(x, 7, 8, prec)
    assert not failures(gotn, wantn, prec)
    assert failures(gotn, L.nchw_to_nhwc(np.roll(x, 1, axis=1), 7, 8, prec), prec)
    negz = wantn.copy()
    negz[1, 2, 3, 7] = L.to_bits(f32(-0.0), prec).reshape(-1)[0]
    assert failures(gotn, negz, prec)
