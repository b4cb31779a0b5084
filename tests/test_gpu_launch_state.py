"""GPU: what a launch does depends on its own context and arguments only, never on what another context's call left
behind.  The exact-sync descriptor and the fp16 1/S pointer travel as arguments of the launchers (fu_common.h), so calls
of several contexts interleave freely.  Every net: base_channels 8, 4 input channels, 3 classes, batch 2 of 32 x 32, one
device, fixed seeds.  Bit-equality with a solo run rests on a step being bit-reproducible run to run (fixed-order
reductions, no atomics), as tools/step_digest.py does.

  sync isolation     net P (bf16, no sync) gives its solo bits -- loss, flat gradient, running statistics -- when its
                     forward, loss and backward are interleaved with the calls of net S (bf16, fu_set_exact_sync with
                     world = 2 and a hook that doubles the exchange buffer on the call's stream: two identical ranks);
                     the hook is never called during a call of P, S's two training forwards call it the same non-zero
                     number of times, an eval forward of S not at all.
  unscale isolation  net F (fp16) and net Q (bf16), backward calls interleaved: both flat gradients equal their solo bits.
                     F's solo gradient is pinned too, since a missing 1/S would scale it by a power of two (S is in
                     [32, 64)) in both runs alike: against the fp32 net of the same seed and weights, with the fp16 gradient
                     tolerance of test_gpu_unet.py (test_bf16_step_within_stated_tolerance_of_fp32_reference: every live
                     tensor's norm within a factor 2 of the fp32 one, median cosine >= LOWP_TOL["fp16"]["cos"]); that file
                     has no fp16-against-bf16 pair tolerance."""
import numpy as np
import pytest
import torch

from conftest import is_dead_bias
from floodplanet_code_amd import _lib
from floodplanet_code_amd.unet import HipUNet
from test_gpu_unet import LOWP_TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def make_net(prec):
    torch.manual_seed(21)
    return HipUNet(4, 3, base_channels=8, precision=prec).to(DEV).train()


def make_data():
    torch.manual_seed(22)
    return torch.rand(2, 4, 32, 32, device=DEV), torch.randint(0, 3, (2, 32, 32), device=DEV)


def forward(net, x, training=True):
    net._forward_raw(x, training, want_logits=False)


def loss(net, tgt):
    return net._loss_raw(tgt, -100, DEV)


def backward(net):
    net._flat_grad.zero_()
    net._backward_raw(None, DEV)


def result(net, loss_dev):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in (loss_dev.reshape(1), net._flat_grad, net._flat_rm, net._flat_rv)]


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


def solo_step(net, x, tgt):
    forward(net, x)
    l = loss(net, tgt)
    backward(net)
    return result(net, l)


def test_sync_isolation_between_contexts():
    lib = _lib.load()
    x, tgt = make_data()
    P, S = make_net("bf16"), make_net("bf16")
    ctx_p, ctx_s = P._get_ctx(DEV, 2, 32, 32), S._get_ctx(DEV, 2, 32, 32)
    start = [t.clone() for t in (P._flat_rm, P._flat_rv, P._flat_nbt)]
    solo = solo_step(P, x, tgt)
    for buf, t in zip((P._flat_rm, P._flat_rv, P._flat_nbt), start):     # the running statistics the solo step started from
        buf.copy_(t)
    assert P._get_ctx(DEV, 2, 32, 32) is ctx_p

    nbytes = int(lib.fu_exact_sync_bytes(ctx_s))
    xbuf = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device=DEV)
    calls = []

    def hook(_user, n_elems, is_double):
        (xbuf[:n_elems] if is_double else xbuf.view(torch.float32)[:n_elems]).mul_(2)     # two identical ranks, summed
        calls.append(n_elems)
        return 0

    def hook_calls_during(fn, *args):
        before = len(calls)
        out = fn(*args)
        return len(calls) - before, out

    cb = _lib.SYNC_HOOK(hook)
    _lib.check(lib.fu_set_exact_sync(ctx_s, cb, None, 2, _lib.ptr(xbuf), nbytes))
    try:
        n, _ = hook_calls_during(forward, P, x)
        assert n == 0
        s_fwd1, _ = hook_calls_during(forward, S, x)
        ls = loss(S, tgt)
        backward(S)
        n, lp = hook_calls_during(loss, P, tgt)
        assert n == 0
        s_fwd2, _ = hook_calls_during(forward, S, x)
        n, _ = hook_calls_during(backward, P)
        assert n == 0
        inter = result(P, lp)
        s_eval, _ = hook_calls_during(forward, S, x, False)
    finally:
        _lib.check(lib.fu_set_exact_sync(ctx_s, _lib.SYNC_HOOK(0), None, 1, None, 0))
    torch.cuda.synchronize()
    print("hook calls: S training forwards", s_fwd1, s_fwd2, "S eval forward", s_eval, "in all", len(calls))
    assert same_bits(inter, solo), [(u.double() - v.double()).abs().max().item() for u, v in zip(inter, solo)]
    assert s_fwd1 == s_fwd2 and s_fwd1 >= len(S._bn), (s_fwd1, s_fwd2)      # every BatchNorm's statistics went through the hook
    assert s_eval == 0
    assert len(calls) > 2 * s_fwd1                                            # S's loss and backward sums did too
    assert torch.isfinite(ls).item() and torch.isfinite(S._flat_grad).all()


def test_unscale_isolation_between_contexts():
    x, tgt = make_data()
    F, Q, R = make_net("fp16"), make_net("bf16"), make_net("fp32")
    assert torch.equal(F._table[0][1].detach().cpu(), Q._table[0][1].detach().cpu())     # same seed, same weights
    gf = solo_step(F, x, tgt)[1]
    gq = solo_step(Q, x, tgt)[1]
    gr = solo_step(R, x, tgt)[1]

    forward(F, x)
    loss(F, tgt)
    forward(Q, x)
    loss(Q, tgt)
    F._flat_grad.zero_()
    Q._flat_grad.zero_()
    F._backward_raw(None, DEV)
    Q._backward_raw(None, DEV)
    torch.cuda.synchronize()
    assert same_bits([F._flat_grad], [gf])
    assert same_bits([Q._flat_grad], [gq])
    assert torch.isfinite(gf).all() and gf.abs().max() > 0

    # fp16's solo gradient against the fp32 net's: the norms of the true gradients agree, whatever rounding does to directions
    cos, ratios = [], []
    for name, p, off, n in F._table:
        if is_dead_bias(name):
            continue
        a, b = gf[off:off + n].cpu().double(), gr[off:off + n].cpu().double()
        ref_norm = b.norm().item()
        if ref_norm >= 1e-5:
            ratios.append((a.norm().item() / ref_norm, name))
        if n >= 64:
            cos.append((a @ b / (a.norm() * b.norm() + 1e-30)).item())
    print("fp16 / fp32 gradient norm ratios: min %.4f max %.4f; median cosine %.4f over %d tensors"
          % (min(ratios)[0], max(ratios)[0], float(np.median(cos)), len(cos)))
    assert ratios and cos
    for ratio, name in ratios:
        assert 0.5 <= ratio <= 2.0, (name, ratio)
    assert np.median(cos) >= LOWP_TOL["fp16"]["cos"], np.median(cos)
