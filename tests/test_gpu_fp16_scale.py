"""GPU: the fp16 loss scale and overflow guard, one operator at a time and on every path that carries them.

  a  k_absmax_partial + k_loss_grad_eff (fu_op_loss_grad_eff) against tests/tools/loss_scale_ref.py: the output bit for bit,
     scale[0] and scale[1] exactly, at sizes around the workgroup, one / two partials and the 256-partial cap, with the
     maximum at the first, the last and the 4097th element, at both ends of [32, 64), with non-finite entries, every
     upstream factor, every back-off; the clamp at +-60; the arm without a scale; the input never written.
  b  k_grad_finite_check (fu_op_fp16_guard, book = 0): one bad element at the first / last index and on both sides of the
     head | body | tail seams, for inf, -inf, NaN and the first float above 3.0e38; 3.0e38 itself and zeros are clean; the
     flag is an OR; guard[1..3] stay; a buffer 1, 2 and 3 floats past a 16-byte boundary; nothing outside g is examined.
  c  k_guard_book: the scripted sequence of the CPU test, every call's four integers against guard_book_ref.
  d  the 1/S of every parameter-gradient writer, on the architectures no other fp16 test runs: the ConvTranspose net
     (launch_colsum_partials, the one-tap wgrad, k_convT_grad_from_w3) and the late-fusion nets (the one-tap wgrads and
     their bias partials, k_center_from_w3; two encoders at base 64: the two-destination dgrad; base 8, two and three
     encoders: the gcat + k_copy_channels split).  fp16 gradients per tensor against the fp32 net of the same weights and
     batch with the criteria test_unscale_isolation_between_contexts states -- S is 2^16 here, a writer without the
     unscale is off by almost five orders of magnitude -- and once more with the back-off exponent set to 3: S exactly 8 times
     smaller, the same criteria (a writer with a stale 1/S is off by 8).
  e  the state a real step leaves: S * max|dlogits| in [32, 64), S a power of two; guard == [0, 1, 1, 0] after a skipped
     step; the next backward's S one power of two below the rule's.
  f  the captured-graph trainer in fp16 equals the eager one bit for bit, with ordinary weights and with steps that overflow
     and are skipped: the skip flag and the scale are device memory, so a replay follows them."""
import ctypes as C
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import case_inputs, is_dead_bias, load_golden
from floodplanet_code_amd import _lib
from floodplanet_code_amd.latefusion import HipLateFusion
from floodplanet_code_amd.unet import HipUNet
from oracle import unet_oracle as O
from test_gpu_unet import LOWP_TOL
from tools import loss_scale_ref as R
from tools.hip_mem import memcpy_dtod

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
ABOVE = np.nextafter(F32(3.0e38), F32(np.inf))               # 3.0000002e38: finite and bad
SENTINEL = -7.0


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ------------------------------------------------------------------------------------------- a. scale + effective gradient
def run_eff(x, up=None, backoff=None, scaled=True):
    """fu_op_loss_grad_eff on x (numpy fp32) -> (out, scale or None, partials), all numpy; asserts that the input and the
    guard are not written."""
    lib = _lib.load()
    xd = dev(x)
    keep = xd.clone()
    out = torch.full_like(xd, SENTINEL)
    partials = torch.full((256,), SENTINEL, dtype=torch.float32, device=DEV)
    scale = torch.full((2,), SENTINEL, dtype=torch.float32, device=DEV) if scaled else None
    guard = None if backoff is None else torch.tensor([0, 5, backoff, 9], dtype=torch.int32, device=DEV)
    upd = None if up is None else torch.tensor([up], dtype=torch.float32, device=DEV)
    _lib.check(lib.fu_op_loss_grad_eff(xd.data_ptr(), out.data_ptr(), xd.numel(), _lib.ptr(upd), partials.data_ptr(),
                                       _lib.ptr(scale), _lib.ptr(guard), stream()))
    torch.cuda.synchronize()
    assert torch.equal(xd.view(torch.int32), keep.view(torch.int32)), "dlogits was written"
    if guard is not None:
        assert guard.tolist() == [0, 5, backoff, 9], "the guard was written"
    return out.cpu().numpy(), None if scale is None else scale.cpu().numpy(), partials.cpu().numpy()


def check_eff(x, up, backoff, note):
    out, scale, _ = run_eff(x, up, backoff)
    want, S, inv = R.loss_grad_eff_ref(x, up, backoff or 0)
    assert (float(scale[0]), float(scale[1])) == (float(S), float(inv)), (note, scale, S, inv)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out), nan), note
    assert np.array_equal(bits(out)[~nan], bits(want)[~nan]), (note, int((bits(out) != bits(want)).sum()))
    return float(S)


def body_with_max(n, maximum, pos, seed, negative=False):
    """n floats of magnitude in [maximum / 1024, maximum / 2], random signs, and +-maximum at pos: the maximum is a known
    float, and every product with a factor that takes it into [32, 64) (times an |up| >= 0.3) is a normal float."""
    rng = np.random.RandomState(seed)
    x = (rng.uniform(1.0 / 1024, 0.5, n) * rng.choice([-1.0, 1.0], n)).astype(F32) * F32(maximum)
    x[pos] = -F32(maximum) if negative else F32(maximum)
    return x


P2M13 = F32(2.0 ** -13)
MAXIMA = [P2M13, np.nextafter(P2M13, F32(0)), F32(65504.0), F32(1e-4)]
UPS = [None, 1.0, 4.0, 0.3, -2.0, 0.0]
BACKOFFS = [0, 3, 14]
SIZES = [1, 255, 256, 257, 4096, 4097, 256 * 4096 + 1]


@pytest.mark.parametrize("n", SIZES)
def test_loss_grad_eff_equals_the_reference_bit_for_bit(n):
    positions = sorted({0, n - 1} | ({4096} if n > 4096 else set()))
    # every maximum, upstream factor and back-off at least once at every position ...
    rows = [(MAXIMA[0], None, None), (MAXIMA[1], 1.0, 3), (MAXIMA[2], 4.0, 14), (MAXIMA[3], 0.3, 0), (MAXIMA[0], -2.0, 3),
            (MAXIMA[1], 0.0, 0)]
    cases = [(m, up, bo, pos) for pos in positions for (m, up, bo) in rows]
    # ... and, below the largest size, the full cross product with the maximum at the last element
    if n <= 4097:
        cases += [(m, up, bo, n - 1) for m in MAXIMA for up in UPS for bo in BACKOFFS]
    seen = set()
    for k, (m, up, bo, pos) in enumerate(cases):
        x = body_with_max(n, m, pos, seed=k, negative=bool(k & 1))
        S = check_eff(x, up, bo, (n, float(m), up, bo, pos))
        seen.add(S)
        if up in (None, 1.0) and not bo:
            assert 32.0 <= S * float(m) < 64.0                            # the rule itself, not only the reference
    assert len(seen) > 3


@pytest.mark.parametrize("n", [257, 4097, 256 * 4096 + 1])
def test_loss_grad_eff_zeros_and_non_finite_entries(n):
    out, scale, _ = run_eff(np.zeros(n, dtype=F32))
    assert scale.tolist() == [1.0, 1.0] and not bits(out).any()
    for k, (up, bo) in enumerate([(None, 0), (0.3, 3), (-2.0, None)]):
        x = body_with_max(n, F32(1e-4), n // 2, seed=10 + k)
        for j, v in enumerate((np.inf, np.nan, ABOVE)):                   # spread over the partials, and at both ends
            x[[0, n - 1, n // 3][(j + k) % 3]] = v
        assert float(R.absmax(x)) == float(F32(1e-4))
        S = check_eff(x, up, bo, (n, up, bo))
        assert S == math.ldexp(1.0, R.scale_exponent(np.array([1e-4], dtype=F32), up, bo or 0))
    out, scale, _ = run_eff(np.array([np.inf, np.nan, -ABOVE] * 3, dtype=F32)[:min(n, 9)])
    assert scale.tolist() == [1.0, 1.0]                                   # nothing to measure: S = 1


def test_loss_grad_eff_clamps_the_exponent_at_60():
    for m, e in ((F32(1e-45), 60), (np.frombuffer(np.uint32(0x00800000).tobytes(), dtype=F32)[0], 60), (F32(3.0e38), -60)):
        for bo in (None, 3):
            x = np.zeros(4097, dtype=F32)
            x[4096] = m
            _, scale, _ = run_eff(x, None, bo)
            assert scale.tolist() == [math.ldexp(1.0, e), math.ldexp(1.0, -e)], (float(m), bo, scale)
    x = np.zeros(300, dtype=F32)                                          # the back-off reaches below the lower clamp too
    x[7] = F32(3.0e38)
    _, scale, _ = run_eff(x, None, 14)
    assert scale.tolist() == [math.ldexp(1.0, -60), math.ldexp(1.0, 60)]


@pytest.mark.parametrize("n", [1, 257, 4097])
def test_loss_grad_eff_without_a_scale(n):
    x = body_with_max(n, F32(0.37), n - 1, seed=3)
    for up in (0.3, None):
        out, scale, partials = run_eff(x, up, None, scaled=False)
        want, S, inv = R.loss_grad_eff_ref(x, up, 0, scaled=False)
        assert scale is None and S is None
        assert np.array_equal(bits(out), bits(want))
        assert (partials == SENTINEL).all(), "partials written without a scale"
    assert np.array_equal(bits(out), bits(x))                             # no factor at all: a copy


# ------------------------------------------------------------------------------------------- b. the finite check
def seams(n, shift):
    """the indices where the kernel's parts meet, for a buffer `shift` floats past a 16-byte boundary"""
    head = min((4 - shift) % 4, n)
    nvec = (n - head) // 4
    tail0 = head + 4 * nvec
    idx = {0, n - 1}
    if head:
        idx |= {head - 1}                                                 # last of the head
    if nvec:
        idx |= {head, tail0 - 1}                                          # first and last of the 16-byte body
    if tail0 < n:
        idx |= {tail0}                                                    # first of the tail
    if nvec > 256:
        idx |= {head + 4 * 256, head + 4 * 255 + 3}                       # the second turn of a lane
    return sorted(idx)


@pytest.mark.parametrize("n, shift", [(n, 0) for n in (1, 2, 3, 4, 5, 1023, 1024, 1025, 4099)] + [(4099, s) for s in (1, 2, 3)])
def test_grad_finite_check_sees_every_position(n, shift):
    lib = _lib.load()
    base = torch.zeros(n + 16, dtype=torch.float32, device=DEV)
    g = base[4 + shift:4 + shift + n]
    assert g.data_ptr() % 16 == 4 * shift
    base[4 + shift - 1] = float("inf")                                    # just outside g on both sides: never examined
    base[4 + shift + n] = float("nan")
    idx = seams(n, shift)
    if shift == 0:
        assert {0, n - 1, 4 * (n // 4) - 1 if n >= 4 else 0, min(4 * (n // 4), n - 1)} <= set(idx)
    bad_values = [float("inf"), float("-inf"), float("nan"), float(ABOVE)]
    cases = [(i, v, 0, 1) for i in idx for v in bad_values]               # (index, value, flag before, flag after)
    cases += [(i, s * 3.0e38, 0, 0) for i in idx for s in (1.0, -1.0)]    # the largest clean value
    cases += [(None, 0.0, 0, 0), (None, 0.0, 1, 1), (idx[-1], float("nan"), 1, 1)]        # zeros; the flag is an OR
    guards = torch.zeros(len(cases), 4, dtype=torch.int32, device=DEV)
    guards[:, 1], guards[:, 2], guards[:, 3] = 5, 7, 9
    guards[:, 0] = torch.tensor([c[2] for c in cases], dtype=torch.int32, device=DEV)
    for k, (i, v, _, _) in enumerate(cases):
        g.zero_()
        if i is not None:
            g[i] = v
        _lib.check(lib.fu_op_fp16_guard(g.data_ptr(), n, guards[k].data_ptr(), 0, stream()))
    torch.cuda.synchronize()
    got = guards.cpu().tolist()
    for k, (i, v, _, after) in enumerate(cases):
        assert got[k] == [after, 5, 7, 9], (n, shift, i, v, got[k])


def test_grad_finite_check_large_buffer_every_workgroup():
    """more floats than one turn of the capped grid (2048 workgroups x 1024): one NaN deep inside, then none"""
    lib = _lib.load()
    n = 2048 * 1024 * 2 + 4099
    base = torch.zeros(n + 16, dtype=torch.float32, device=DEV)
    guards = torch.zeros(6, 4, dtype=torch.int32, device=DEV)
    for k, (shift, i) in enumerate([(0, 2048 * 1024 + 77), (3, n - 2), (1, None), (0, None), (2, 2048 * 1024 * 2 + 5), (1, 0)]):
        g = base[4 + shift:4 + shift + n]
        base.zero_()
        if i is not None:
            g[i] = float("nan")
        _lib.check(lib.fu_op_fp16_guard(g.data_ptr(), n, guards[k].data_ptr(), 0, stream()))
    torch.cuda.synchronize()
    assert guards[:, 0].tolist() == [1, 1, 0, 0, 1, 1] and not guards[:, 1:].any()


# ------------------------------------------------------------------------------------------- c. the book
def test_guard_book_follows_the_reference_call_by_call():
    lib = _lib.load()
    for seq, start in ((R.book_script(), [0, 0, 0, 0]), ([False] * 64, [0, 0, 0, 0]), ([False] * 3, [1, 2, 3, 40])):
        guard = torch.tensor(start, dtype=torch.int32, device=DEV)
        clean = torch.full((5,), 0.5, dtype=torch.float32, device=DEV)
        dirty = clean.clone()
        dirty[4] = float("inf")                                           # in the tail
        log = torch.zeros(len(seq), 4, dtype=torch.int32, device=DEV)
        for k, bad in enumerate(seq):
            _lib.check(lib.fu_op_fp16_guard((dirty if bad else clean).data_ptr(), 5, guard.data_ptr(), 1, stream()))
            log[k].copy_(guard)
        torch.cuda.synchronize()
        got, st = log.cpu().tolist(), list(start)
        for k, bad in enumerate(seq):
            st = R.guard_book_ref(st, bad)
            assert got[k] == st, (k, bad, got[k], st)
    assert st == [0, 3, 4, 2]


# ------------------------------------------------------------------------------------------- d. the unscale on every architecture
def fp16_state(net):
    sc, gd = (C.c_float * 2)(), (C.c_int32 * 4)()
    _lib.check(_lib.load().fu_test_fp16_state(net._ctx, sc, gd))
    return (float(sc[0]), float(sc[1])), list(gd)


def one_backward(net, x, tgt, backoff=None):
    """training forward, loss, backward into a zeroed gradient buffer -> the flat gradient (a clone)"""
    net._forward_raw(x, True, want_logits=False)
    net._loss_raw(tgt, 0, DEV)
    if backoff is not None:
        _lib.check(_lib.load().fu_test_set_fp16_backoff(net._ctx, backoff, 0, net._stream(DEV)))
    net._flat_grad.zero_()
    net._backward_raw(None, DEV)
    torch.cuda.synchronize()
    return net._flat_grad.detach().clone()


def assert_tracks_fp32(net, g16, g32, note):
    """the criteria of test_unscale_isolation_between_contexts (test_gpu_launch_state.py)"""
    assert torch.isfinite(g16).all() and g16.abs().max() > 0, note
    cos, ratios = [], []
    for name, _, off, n in net._table:
        if is_dead_bias(name):
            continue
        a, b = g16[off:off + n].cpu().double(), g32[off:off + n].cpu().double()
        ref_norm = b.norm().item()
        if ref_norm >= 1e-5:
            ratios.append((a.norm().item() / ref_norm, name))
        if n >= 64:
            cos.append((a @ b / (a.norm() * b.norm() + 1e-30)).item())
    assert ratios and cos
    print("%s: fp16 / fp32 gradient norm ratios min %.4f (%s) max %.4f (%s); median cosine %.4f over %d tensors"
          % ((note,) + min(ratios) + max(ratios) + (float(np.median(cos)), len(cos))))
    for ratio, name in ratios:
        assert 0.5 <= ratio <= 2.0, (note, name, ratio)
    assert np.median(cos) >= LOWP_TOL["fp16"]["cos"], (note, np.median(cos))


def make_convT(prec):
    meta, _ = load_golden("f_convT_c4_32")
    batch, st = case_inputs(meta)
    assert (meta["B"], meta["H"], meta["W"], meta["n_in"]) == (2, 32, 32, 4)
    net = HipUNet(4, 3, bilinear=False, base_channels=64, precision=prec)
    net.load_state_dict(st)
    return net.to(DEV).train(), batch["image"].to(DEV), batch["target"].to(DEV)


def make_lf(in_ch, base, prec):
    in_ch = OrderedDict(in_ch)
    st = O.lf_make_state(in_ch, 3, base, seed=2)
    batch = O.make_batch(2, in_ch["ms_image"], 32, 32, seed=4, extra=tuple(k for k in in_ch if k != "ms_image"))
    net = HipLateFusion(in_ch, 3, base_channels=base, precision=prec)
    net.load_state_dict(st)
    net = net.to(DEV).train()
    x = torch.cat([batch[O.LF_BATCH_KEY.get(k, k)] for k in net.encoder_names], dim=1)
    return net, x.to(DEV), batch["target"].to(DEV)


ARCHS = {
    "convT_base64": lambda prec: make_convT(prec),
    "lf2_base64": lambda prec: make_lf([("ms_image", 8), ("dem", 1)], 64, prec),
    "lf2_base8": lambda prec: make_lf([("ms_image", 8), ("dem", 1)], 8, prec),
    "lf3_base8": lambda prec: make_lf([("ms_image", 4), ("dem", 1), ("slope", 1)], 8, prec),
}


@pytest.mark.parametrize("arch", sorted(ARCHS))
def test_fp16_gradients_are_unscaled_by_every_writer(arch):
    ref, x, tgt = ARCHS[arch]("fp32")
    g32 = one_backward(ref, x, tgt)
    del ref
    net, x, tgt = ARCHS[arch]("fp16")
    g16 = one_backward(net, x, tgt)
    (S, inv), guard = fp16_state(net)
    assert guard == [0, 0, 0, 0]
    assert S > 0 and math.frexp(S)[0] == 0.5 and S * inv == 1.0, (S, inv)
    assert_tracks_fp32(net, g16, g32, arch)
    g16b = one_backward(net, x, tgt, backoff=3)
    (Sb, invb), guard = fp16_state(net)
    print("%s: S = 2^%d, with back-off 3: 2^%d" % (arch, math.frexp(S)[1] - 1, math.frexp(Sb)[1] - 1))
    assert guard == [0, 0, 3, 0]
    assert Sb * 8.0 == S and Sb * invb == 1.0, (S, Sb, invb)
    assert_tracks_fp32(net, g16b, g32, arch + " (back-off 3)")


# ------------------------------------------------------------------------------------------- e. the state of a real step
def max_abs_dlogits(net):
    lib = _lib.load()
    lg, dl, n = C.c_void_p(), C.c_void_p(), C.c_int64()
    _lib.check(lib.fu_test_loss_buffers(net._ctx, C.byref(lg), C.byref(dl), C.byref(n)))
    torch.cuda.synchronize()
    t = torch.empty(n.value, dtype=torch.float32, device=DEV)
    memcpy_dtod(t.data_ptr(), dl.value, 4 * n.value)
    assert torch.isfinite(t).all()
    return float(t.abs().max().item())


def base16_net(outconv=None):
    st = O.make_state(8, 3, 16, True, seed=1)
    if outconv is not None:
        st["outc.conv.weight"][:] = st["outc.conv.weight"].sign() * outconv
    batch = O.make_batch(2, 8, 64, 64, seed=2)
    net = HipUNet(8, 3, base_channels=16, precision="fp16")
    net.load_state_dict(st)
    return net.to(DEV).train(), batch["image"].to(DEV), batch["target"].to(DEV)


def test_fp16_state_after_a_clean_and_after_a_skipped_step():
    lib = _lib.load()
    net, x, t = base16_net()
    net.train_step(x, t, 0)
    (S, inv), guard = fp16_state(net)
    m = max_abs_dlogits(net)
    assert guard == [0, 0, 0, 0]
    assert math.frexp(S)[0] == 0.5 and S * inv == 1.0                     # a power of two and its inverse
    assert 32.0 <= S * m < 64.0, (S, m)
    net.adam_step(1e-3, 1)
    assert fp16_state(net)[1] == [0, 0, 0, 1]                             # one clean step booked
    for bad in (-1, 15):
        assert lib.fu_test_set_fp16_backoff(net._ctx, bad, 0, None) == _lib.FU_ERR_INVALID
        assert lib.fu_test_set_fp16_backoff(net._ctx, 0, 64 if bad > 0 else -1, None) == _lib.FU_ERR_INVALID

    net, x, t = base16_net(outconv=3.0e3)
    net.train_step(x, t, 0)
    torch.cuda.synchronize()
    assert not torch.isfinite(net.flat_grads()).all()                     # the scenario really overflows
    net.adam_step(1e-3, 1)
    (S1, _), guard = fp16_state(net)
    assert guard == [0, 1, 1, 0]
    net.train_step(x, t, 0)
    (S2, inv2), guard = fp16_state(net)
    m = max_abs_dlogits(net)
    assert guard == [0, 1, 1, 0]
    assert S2 == math.ldexp(1.0, 6 - math.frexp(m)[1] - 1) and S2 * inv2 == 1.0, (S2, m)

    n32 = HipUNet(8, 3, base_channels=16).to(DEV).train()                 # not fp16: zeros, and the setter refuses
    n32.train_step(x, t, 0)
    assert fp16_state(n32) == ((0.0, 0.0), [0, 0, 0, 0])
    assert lib.fu_test_set_fp16_backoff(n32._ctx, 1, 0, None) == _lib.FU_ERR_INVALID


# ------------------------------------------------------------------------------------------- f. the captured step in fp16
def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                      b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("outconv", [None, 3.0e3], ids=["ordinary", "overflow"])
def test_captured_hipgraph_step_equals_eager_step_fp16(outconv):
    from floodplanet_code_amd.distributed import DataParallelTrainer
    st = O.make_state(8, 3, 16, True, seed=4)
    if outconv is not None:
        st["outc.conv.weight"][:] = st["outc.conv.weight"].sign() * outconv
    batches = [O.make_batch(2, 8, 64, 64, seed=40 + i) for i in range(3)]
    outs = []
    for graph in (False, True):
        net = HipUNet(8, 3, base_channels=16, precision="fp16")
        net.load_state_dict(st)
        net.to(DEV).train()
        tr = DataParallelTrainer(net, lr=1e-3, graph=graph)
        losses = []
        for it in range(6):
            b = batches[it % 3]
            losses.append(tr.step(b["image"].to(DEV), b["target"].to(DEV), 0))
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph
        outs.append(([l.item() for l in losses], [t.clone() for t in (net.flat_parameters(), net.adam_state()[0], net.adam_state()[1],
                                                                     net._flat_rm, net._flat_rv, net._flat_nbt, net.flat_grads())],
                     fp16_state(net), net.fp16_guard_state()))
    (la, ta, sa, ga), (lb, tb, sb, gb) = outs
    print("losses", la, "fp16 state", sa, "skipped / back-off", ga)
    assert np.array_equal(np.array(la), np.array(lb), equal_nan=True)
    assert outconv is not None or all(math.isfinite(v) for v in la)
    for k, (u, v) in enumerate(zip(ta, tb)):
        assert same_bits(u, v), k
    assert sa == sb and ga == gb
    skipped, backoff = ga
    if outconv is None:
        assert (skipped, backoff) == (0, 0) and sa[1] == [0, 0, 0, 6]
        assert torch.isfinite(ta[0]).all() and ta[1].abs().max() > 0
    else:
        assert skipped >= 1 and sa[1][1] == skipped and sa[1][2] == backoff
        assert torch.isfinite(ta[0]).all() and torch.isfinite(ta[1]).all()
