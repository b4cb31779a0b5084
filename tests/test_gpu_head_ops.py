"""GPU: the 1x1 head (fu_head.hip) on its own, through the fu_op_head_fwd / fu_op_head_bwd test hooks, element by element against
the fp64 reference and the analytic bounds of tests/tools/head_ref.py (derived there; test_head_ref_cpu.py holds a float32
restatement of the kernels' arithmetic to them) -- never against the code under test.

  k_head_fwd<T, NC, 4>           fu_op_head_fwd   logits = bias + relu(a*y+b) . w^T (or y . w^T), NHWC and optional NCHW copy
  k_head_bwd<T, NC, 4, BNB>      fu_op_head_bwd   g = dl . w, dW = dl^T . z, db = sum dl, with BNB the BatchNorm-backward sums
  k_head_bwd<.., true, false>    whole net only   the skip_g form: g recomputed by k_bn_bwd_apply_head (tiny nets below)

Every precision x every legal width (lanes per pixel 1, 2, 4, 8, 16: each another path through the DPP reduction and another
pixels-per-block) x class counts 1..4 (specialised), 5 and 8 (generic instantiation).  Every output buffer is prefilled with
NaN and followed by one row of a sentinel that must survive; every case runs twice and must give the same bits.  A pass is
err / bound <= 1 for EVERY element; an element whose bound is 0 (an all-masked pixel, a zero gradient row) must be exact.

MEASURED worst err / bound per output and precision (MI355X, this file's cases; a pass is <= 1):
              logits   g       dW      db      s1      s2
  fp32        0.575    0.999   0.187   0.058   -       -        (no fused sums in fp32: FU_ERR_UNSUPPORTED)
  bf16        0.524    0.996   0.242   0.086   0.143   0.158
  fp16        0.451    1.000   0.234   0.086   0.156   0.182
  grid cap (133333 pixels): dW 0.034 / 0.034 / 0.049, db 0.003, s1 0.001, s2 0.025 / 0.015; single-pixel dW 0.47 / 0.33 / 0.58.
g sits at 1 by construction (one class: a single product against gamma(1); 16-bit: the store rounding reaches the type's unit
roundoff); the float32 restatement of test_head_ref_cpu.py measures the same figures to the third digit, i.e. the kernels'
error IS their arithmetic's.  Recomputed vs stored head gradient on the tiny nets: 5.0e-3 - 5.8e-3 of the 7.8e-3 (bf16),
6.1e-4 - 7.2e-4 of the 9.8e-4 (fp16).  The whole file takes about 11 s.
Before the two-pass LDS reduction of k_head_bwd every bf16 / fp16 case with 8 classes failed with "head_bwd: LDS request too
large".
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from tools import head_ref as R   # noqa: E402

from floodplanet_code_amd import _lib   # noqa: E402
from floodplanet_code_amd._lib import check, ptr   # noqa: E402
from floodplanet_code_amd.unet import HipUNet   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
CODE = {"fp32": _lib.FU_F32, "bf16": _lib.FU_BF16, "fp16": _lib.FU_F16}
SENTINEL = 1024.0                     # exact in every element type
SMALL_WIDTH = {"fp32": 16, "bf16": 32, "fp16": 16}     # the width of the shapes below one block: 4, 4 and 2 lanes per pixel


@pytest.fixture(params=list(R.PREC))
def prec(request):
    return request.param


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def out_buf(n, row, dt=torch.float32):
    """n elements of NaN followed by one row of the sentinel"""
    t = torch.full((n + row,), float("nan"), device=DEV, dtype=dt)
    t[n:] = SENTINEL
    return t


def intact(t, n):
    return bool((t[n:].float() == SENTINEL).all())


def to_dev(ops):
    """the operands of make_operands (8 classes) on the device; y in the element type"""
    d = {k: torch.from_numpy(ops[k]).to(DEV) for k in ("a", "b", "mean", "invstd", "w", "bias", "dl")}
    d["y"] = torch.from_numpy(ops["y"]).to(R.PREC[ops["prec"]]["dt"]).to(DEV)
    return d


def run_fwd(prec, d, C_, ncls, B, H, W, bn, nchw):
    n = B * H * W * ncls
    nh, nc = out_buf(n, ncls), (out_buf(n, ncls) if nchw else None)
    a, b = (d["a"], d["b"]) if bn else (None, None)
    check(_lib.load().fu_op_head_fwd(CODE[prec], ptr(d["y"]), ptr(a), ptr(b), ptr(d["w"]), ptr(d["bias"]), C_, ncls, B, H, W,
                                     ptr(nh), ptr(nc), stream()))
    torch.cuda.synchronize()
    return nh, nc


def run_bwd(prec, d, dl, C_, ncls, npix, bn, sums, expect=_lib.FU_OK):
    """{name: (buffer, payload elements)}; dl [npix, ncls] contiguous on the device"""
    dt = R.PREC[prec]["dt"]
    out = {"g": (out_buf(npix * C_, C_, dt), npix * C_), "dw": (out_buf(ncls * C_, C_), ncls * C_),
           "db": (out_buf(ncls, ncls), ncls)}
    if sums:
        out["s1"], out["s2"] = (out_buf(C_, C_), C_), (out_buf(C_, C_), C_)
    a, b = (d["a"], d["b"]) if bn else (None, None)
    sp = [ptr(d["mean"]), ptr(d["invstd"]), ptr(out["s1"][0]), ptr(out["s2"][0])] if sums else [None] * 4
    st = _lib.load().fu_op_head_bwd(CODE[prec], ptr(dl), ptr(d["y"]), ptr(a), ptr(b), ptr(d["w"]), C_, ncls, npix,
                                    ptr(out["g"][0]), ptr(out["dw"][0]), ptr(out["db"][0]), *sp, stream())
    torch.cuda.synchronize()
    assert st == expect, (st, _lib.load().fu_last_error())
    return out


def payload(out, name, shape):
    t, n = out[name]
    return t[:n].float().cpu().numpy().reshape(shape)


class Worst(dict):
    def take(self, name, got, ref, bound, case):
        r = R.worst_ratio(got, ref, bound)
        self[name] = max(self.get(name, 0.0), r)
        assert r <= 1.0, (case, name, r)

    def report(self, what):
        print(f"MEASURED {what}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(self.items())))


# ---- forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bn", [True, False], ids=["bnrelu", "plain"])
def test_head_forward_every_width_and_class_count(prec, bn):
    """Main shape 2 x 37 x 45: at one lane per pixel one block makes two trips, the second ragged; at 16 lanes 14 blocks with a
    ragged tail.  1 x 1 and 3 x 5 leave most of the only block idle.  NHWC and NCHW copies carry the same bits."""
    worst = Worst()
    shapes = [(R.FWD_MAIN, C_) for C_ in R.widths(prec)] + [(s, SMALL_WIDTH[prec]) for s in R.FWD_SMALL]
    for (B, H, W), C_ in shapes:
        ops = R.make_operands(prec, C_, B * H * W)
        d = to_dev(ops)
        for ncls in R.CLASSES:
            o = R.take(ops, ncls)
            ref, bound = R.fwd_ref(prec, o["y"], o["a"] if bn else None, o["b"] if bn else None, o["w"], o["bias"])
            n = B * H * W * ncls
            for nchw in (True, False):
                case = (prec, C_, ncls, (B, H, W), bn, nchw)
                nh, nc = run_fwd(prec, d, C_, ncls, B, H, W, bn, nchw)
                nh2, nc2 = run_fwd(prec, d, C_, ncls, B, H, W, bn, nchw)
                assert intact(nh, n) and (nc is None or intact(nc, n)), case
                worst.take("logits", nh[:n].cpu().numpy().reshape(-1, ncls), ref, bound, case)
                assert torch.equal(bits(nh), bits(nh2)), case
                if nchw:
                    as_nhwc = nc[:n].view(B, ncls, H * W).permute(0, 2, 1).reshape(-1)
                    assert torch.equal(bits(as_nhwc), bits(nh[:n])), case
                    assert torch.equal(bits(nc), bits(nc2)), case
    worst.report(f"fwd {prec} bn={bn}")


# ---- backward -----------------------------------------------------------------------------------------------------------
FORMS = {"bn_sums": (True, True), "bn": (True, False), "plain": (False, False)}


def check_bwd(worst, prec, ops, d, ncls, bn, sums):
    C_, npix = ops["C"], ops["npix"]
    o = R.take(ops, ncls)
    dl = d["dl"][:, :ncls].contiguous()
    a, b = (o["a"], o["b"]) if bn else (None, None)
    mean, invstd = (o["mean"], o["invstd"]) if sums else (None, None)
    ref = R.bwd_ref(prec, o["dl"], o["y"], a, b, o["w"], mean, invstd)
    out, again = (run_bwd(prec, d, dl, C_, ncls, npix, bn, sums) for _ in range(2))
    case = (prec, C_, ncls, npix, bn, sums)
    assert set(out) == set(ref)
    for name, (r, bound) in ref.items():
        assert intact(*out[name]), (case, name)
        worst.take(name, payload(out, name, r.shape), r, bound, case)
        assert torch.equal(bits(out[name][0]), bits(again[name][0])), (case, name)


@pytest.mark.parametrize("form", list(FORMS))
def test_head_backward_every_width_and_class_count(prec, form):
    """npix 1 and 63 (one partly idle block), 1665 and 4099 (ragged last block; 4099 = 4096 + 3).  In fp32 the kernel emits no
    BatchNorm-backward sums: the hook answers FU_ERR_UNSUPPORTED."""
    bn, sums = FORMS[form]
    if sums and prec == "fp32":
        ops = R.make_operands(prec, 64, 63)
        d = to_dev(ops)
        run_bwd(prec, d, d["dl"][:, :3].contiguous(), 64, 3, 63, True, True, expect=_lib.FU_ERR_UNSUPPORTED)
        assert b"does not emit the sums in this precision" in _lib.load().fu_last_error()
        return
    worst = Worst()
    for C_ in R.widths(prec):
        for npix in R.BWD_NPIX:
            ops = R.make_operands(prec, C_, npix)
            d = to_dev(ops)
            for ncls in R.CLASSES:
                check_bwd(worst, prec, ops, d, ncls, bn, sums)
    worst.report(f"bwd {prec} {form}")


def test_head_backward_at_the_grid_cap(prec):
    """133333 pixels at 16 pixels per block and unroll slot: more than the 2048 blocks of the cap take in one trip, so the
    grid-stride loop runs a second, ragged trip.  3 classes (specialised) and 8 (generic; two LDS passes in the 16-bit types)."""
    C_ = R.widths(prec)[-1]
    g = R.bwd_geometry(prec, C_, R.CAP_NPIX)
    assert g["nblk"] == R.HB_BLOCKS and g["trips"] == 2
    ops = R.make_operands(prec, C_, R.CAP_NPIX)
    d = to_dev(ops)
    worst = Worst()
    for ncls in (3, 8):
        check_bwd(worst, prec, ops, d, ncls, True, prec != "fp32")
    worst.report(f"bwd {prec} grid cap")


@pytest.mark.parametrize("npix", [4099, R.CAP_NPIX])
def test_head_backward_visits_every_pixel_exactly_once(prec, npix):
    """Independent of rounding: with dl = 1 everywhere db[k] == npix (an exact integer below 2^24; the hook runs without a loss
    scale), and with dl zero except at one pixel db == dl[p*] and dW is that pixel's outer product -- at the first and last
    pixel, either side of the first block's first trip and of the whole grid's first trip, and the last of the ragged tail."""
    ncls = 3
    worst = Worst()
    for C_ in (R.widths(prec)[0], R.widths(prec)[-1]):
        ops = R.make_operands(prec, C_, npix)
        d = to_dev(ops)
        g = R.bwd_geometry(prec, C_, npix)
        ones = torch.ones(npix, ncls, device=DEV)
        out = run_bwd(prec, d, ones, C_, ncls, npix, True, False)
        assert (payload(out, "db", (ncls,)) == float(npix)).all(), (prec, C_, npix, payload(out, "db", (ncls,)))
        trip, grid_trip = 4 * g["ppb"], g["nblk"] * 4 * g["ppb"]
        spots = sorted({p for p in (0, trip - 1, trip, grid_trip - 1, grid_trip, npix - 1) if 0 <= p < npix})
        if npix == R.CAP_NPIX and C_ == R.widths(prec)[-1]:
            assert grid_trip in spots and grid_trip - 1 in spots           # the capped grid: a second trip exists
        row = np.array([1.5, -0.37109375, 3.0e-3], f32)
        for p in spots:
            dl = torch.zeros(npix, ncls, device=DEV)
            dl[p] = torch.from_numpy(row).to(DEV)
            out = run_bwd(prec, d, dl, C_, ncls, npix, True, False)
            case = (prec, C_, npix, p)
            assert (payload(out, "db", (ncls,)) == row).all(), case
            ref, bound = R.single_pixel_dw(prec, npix, row, ops["y"][p], ops["a"], ops["b"])
            worst.take("dw", payload(out, "dw", (ncls, C_)), ref, bound, case)
            gp = payload(out, "g", (npix, C_))
            assert np.count_nonzero(np.abs(gp).sum(1)) == 1 and np.abs(gp[p]).sum() > 0, case   # g is non-zero at p* alone
    worst.report(f"coverage {prec} npix={npix}")


# ---- the skip_g form: g is not stored, the BatchNorm-backward apply pass recomputes it --------------------------------------
@pytest.mark.parametrize("lowp", ["bf16", "fp16"])
@pytest.mark.parametrize("base,ncls", [(8, 1), (16, 5), (32, 8)])
def test_head_gradient_recomputed_in_the_apply_pass_equals_the_stored_one_on_tiny_nets(base, ncls, lowp):
    """test_head_gradient_recomputed_in_the_apply_pass_equals_the_stored_one (test_gpu_benched_dispatch.py) at widths and class
    counts it does not reach: 1, 2 and 4 lanes per pixel, one class, the generic instantiation with 5 and with 8 classes (two
    LDS passes).  The head's own gradients bit-equal, block up4's within that test's bound."""
    from oracle import unet_oracle as O
    from test_gpu_benched_dispatch import LOWP, _outgoing, rel
    from conftest import is_dead_bias
    lib = _lib.load()
    torch.manual_seed(0)
    net = HipUNet(4, ncls, base_channels=base, precision=lowp).to(DEV).train()
    B, H, W = 2, 32, 48
    x = O.make_batch(B, 4, H, W, seed=11)["image"].to(DEV)
    dlog = (torch.randn(B, ncls, H, W, generator=torch.Generator().manual_seed(5)) * 1e-3).to(DEV)
    dt = LOWP[lowp]["dt"]
    res = []
    for store in (0, 1):
        net._forward_raw(x, True, want_logits=False)
        s = net._stream(DEV)
        try:
            lib.fu_test_head_store_g(store)
            check(lib.fu_backward_block(net._ctx, 0, ptr(dlog), s))
            check(lib.fu_backward_block(net._ctx, 1, None, s))
        finally:
            lib.fu_test_head_store_g(0)
        torch.cuda.synchronize()
        grads = {}
        for b in (0, 1):
            o, n = C.c_int64(), C.c_int64()
            check(lib.fu_block_param_range(net._ctx, b, C.byref(o), C.byref(n)))
            grads.update({k: net.flat_grads()[off:off + m].clone() for (k, p, off, m) in net._table
                          if o.value <= off < o.value + n.value})
        res.append((grads, _outgoing(net, 8, dt)))
    (g_re, out_re), (g_st, out_st) = res
    tol = 2.0 ** -7 if lowp == "bf16" else 2.0 ** -10
    worst = 0.0
    assert any(k.startswith("outc.") for k in g_re)
    for k in g_re:
        assert torch.isfinite(g_re[k]).all() and torch.isfinite(g_st[k]).all(), k
        if k.startswith("outc."):
            assert torch.equal(g_re[k], g_st[k]) and g_re[k].abs().max() > 0, k
            continue
        if is_dead_bias(k) or g_st[k].norm().item() < 1e-9:
            continue
        e = rel(g_re[k], g_st[k])
        worst = max(worst, e)
        assert e <= tol, (k, e)
    for (label, a), (_, c) in zip(out_re, out_st):
        e = rel(a.float(), c.float())
        worst = max(worst, e)
        assert e <= tol, (label, e)
    print(f"MEASURED recompute base {base} ncls {ncls} {lowp}: worst deviation {worst:.3e}; bound {tol:.3e}")
    assert worst > 0.0               # the two routes really are different code


# ---- whole network with 8 classes: the 16-bit head backward asked for more than 64 KiB of LDS and failed ---------------------
@pytest.mark.parametrize("lowp", ["bf16", "fp16"])
def test_eight_class_net_trains_in_16_bit_and_tracks_fp32(lowp):
    """HipUNet(n_in, n_classes=8) at its default width (base 64: the width every other whole-net 16-bit tolerance of the suite was
    stated at) forward, loss and backward on a 2 x 32 x 48 batch: finite gradients, and logits, loss and gradients within
    test_bf16_step_within_stated_tolerance_of_fp32_reference's tolerances (LOWP_TOL, test_gpu_unet.py) of the fp32 run of the
    same net.  The batch leaves 2 x 2 x 3 = 12 samples per channel at the deepest BatchNorm, so the 16-bit noise is near those
    tolerances whatever the head does: the first draft of this test ran base 16 and measured a median bf16 gradient cosine of
    0.8998 against the 0.9 (every other figure inside: logits max 0.135 / rms 0.018, loss 4e-5, agreement 0.958)."""
    from oracle import unet_oracle as O
    from test_gpu_unet import LOWP_TOL
    from conftest import is_dead_bias
    tol = LOWP_TOL[lowp]
    base, n_in, ncls = 64, 4, 8
    st = O.make_state(n_in, ncls, base, True, seed=3)
    batch = O.make_batch(2, n_in, 32, 48, seed=4, n_label_values=ncls)
    x, t = batch["image"].to(DEV), batch["target"].to(DEV)
    assert len(torch.unique(batch["target"])) == ncls

    def step(precision):
        net = HipUNet(n_in, ncls, precision=precision)
        assert net.base_channels == base
        net.load_state_dict({k: v.clone() for k, v in st.items()})
        net.to(DEV).train()
        loss, logits = net.loss(x, t, 255, return_logits=True)
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), logits.detach().cpu().numpy(), {k: p.grad.detach().cpu().double() for k, p in net.named_parameters()}

    loss_r, logits_r, grads_r = step("fp32")
    loss_l, logits_l, grads_l = step(lowp)
    d = logits_l - logits_r
    agree = (logits_l.argmax(1) == logits_r.argmax(1)).mean()
    cos = []
    for k, g in grads_l.items():
        assert torch.isfinite(g).all(), k
        if is_dead_bias(k):
            continue
        ref_norm = grads_r[k].norm().item()
        if ref_norm >= 1e-5:
            assert 0.5 * ref_norm <= g.norm().item() <= 2.0 * ref_norm, (k, g.norm().item(), ref_norm)
        if g.numel() >= 64:
            a, b = g.reshape(-1), grads_r[k].reshape(-1)
            cos.append((a @ b / (a.norm() * b.norm() + 1e-30)).item())
    print(f"MEASURED 8-class net {lowp} vs fp32: logits max {np.abs(d).max():.4f} rms {np.sqrt((d ** 2).mean()):.4f}  "
          f"loss {abs(loss_l - loss_r):.5f}  argmax agreement {agree:.4f}  median gradient cosine {np.median(cos):.4f}")
    head = [k for k in grads_l if k.startswith("outc.")]
    assert len(head) == 2 and all(grads_l[k].abs().max() > 0 for k in head), head
    assert np.abs(d).max() <= tol["lmax"] and np.sqrt((d ** 2).mean()) <= tol["lrms"]
    assert abs(loss_l - loss_r) <= tol["loss"]
    assert agree >= tol["agree"], agree
    assert np.median(cos) >= tol["cos"], np.median(cos)
