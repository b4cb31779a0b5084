"""SHA-256 digests of what the fused loss and optimiser entry points write, with fixed seeds: two builds of the library
compute the same bits exactly when their lines are equal.  Select the build with FU_LIB_PATH (floodplanet_code_amd/_lib.py),
as tools/ab_libs.sh does:

    FU_LIB_PATH=tools/dbglibs/parent.so python tools/step_digest.py
    python tools/step_digest.py

Losses: base-8 net, batch 3 of 48 x 40, training mode, 2 / 3 / 4 / 6 classes, ignore_index 0 / 2 / -100 and an all-ignored
batch; fu_loss_ce, fu_loss_ce_weighted (weights [2.5, 0, 1.3, ...], eps 0 and 0.1) and, on 3 classes, fu_loss_bce_dice; each
digest covers the loss, n_valid, the confusion matrix (the weight sum) and the flat gradient after fu_backward.
Optimiser: the four Adam entry points, three steps each on flat buffers 0, 1 and 3 floats past a 16-byte boundary, with a
parameter count that is a multiple of 4 and one that is not, gradients across five decades; one fp16 case with an inf in
the gradient (the skipped step).
Steps: one training step each (forward, fu_loss_ce, fu_backward; digest of the logits, the loss, the flat gradient and the
running statistics), batch 2 of 32 x 32 in fp32 / bf16 / fp16 with bilinear upsampling (base 8) and with ConvTranspose
(base 64, the only width fu_create takes it at); a 37 x 45 bf16 tile (the pad path); a two-encoder late-fusion net in bf16;
a bf16 step driven block by block (fu_set_side_stream(2), fu_backward_block, fu_backward_join); an eval fu_forward_srcs of
two sources; fu_forward_views + fu_merge_views over the four flip codes.
Convs: what fu_op_conv3x3_fwd, _dgrad, _dgrad_bnsums and _wgrad write, bf16 and fp16, at the smallest shapes that reach each
kernel route (tests/test_conv_route_cpu.py names them): 64 -> 64 at 64 x 64 under tile modes 3 (rs4) and 4 (pp: eight 16 x 32
tiles), 8 -> 64 at 16 x 16 and 64 x 16 (the two c8 variants), 16 -> 24 at 37 x 45 by default (fast) and on the general kernel,
the weight gradient with 8, 64 and 128 input channels and 256 -> 128 at 80 x 80, B = 2 (three stages per workgroup of the
ping-pong kernel: its loop's odd exit after a full round) under each fu_test_force_lockstep_wgrad mode; under the default
dispatch 32 -> 64 at 256 x 256, B = 2 (exactly 512 workgroups) and a dgrad with fused sums below 256 input channels.  The
one-tap kernels have no operator of their own: a late-fusion step of base 8 runs them with 16 ... 128 input channels.
BN: fu_op_bn_bwd (dL/dy, dgamma, dbeta) in fp32 / bf16 / fp16 at 12 x 5 x 7 (C / 4 = 3 does not divide the block: one thread
without a pixel row), 8 x 5 x 7 pooled (windows without a pool output) and 2 x 64 x 32 x 48 plain and pooled; fu_op_head_bwd with
the fused BatchNorm-backward sums in bf16 / fp16 at C = 64 with 2, 3 and 5 classes (the two compile-time class counts and the
run-time one); one base-8 training step in fp32 and in bf16 under fu_set_exact_sync with world = 2 in this one process -- the
hook doubles the exchange buffer in place on the call's stream, i.e. two identical ranks -- which is the only way to
k_bn_finalize / k_bn_bwd_finalize without a second GPU.  (The head-recompute apply, k_bn_bwd_apply_head, already runs in the
steps group: every 16-bit base-8 step there has 8 | base channels, so its head backward skips the store of g.)
Arguments: the groups to run (losses, optimiser, steps, convs, bn; all five by default).  Prints one JSON line."""
import ctypes as C
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from floodplanet_code_amd import _lib  # noqa: E402
from floodplanet_code_amd.latefusion import HipLateFusion  # noqa: E402
from floodplanet_code_amd.unet import HipUNet  # noqa: E402

DEV = torch.device("cuda:0")
ADAM = (1e-3, 0.9, 0.999, 1e-8)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t.dtype in (torch.bfloat16, torch.float16):
            t = t.view(torch.int16)
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def losses(lib, out):
    for ncls in (2, 3, 4, 6):
        torch.manual_seed(ncls)
        net = HipUNet(4, ncls, base_channels=8).to(DEV).train()
        x = torch.rand(3, 4, 48, 40, device=DEV)
        tgt = torch.randint(0, ncls, (3, 48, 40), device=DEV)
        cw = torch.tensor([2.5, 0.0, 1.3, 0.7, 1.9, 0.4][:ncls], device=DEV)
        s = net._stream(DEV)
        for name, t, ign in [(f"ign{i}", tgt, i) for i in (0, 2, -100)] + [("all_ignored", torch.zeros_like(tgt), 0)]:
            kinds = [("ce", None), ("wce_eps0", 0.0), ("wce_eps0.1", 0.1)] + ([("bce_dice", None)] if ncls == 3 else [])
            for kind, eps in kinds:
                net._forward_raw(x, True, want_logits=False)
                loss, nv, wsum = torch.zeros((), device=DEV), torch.zeros((), dtype=torch.int64, device=DEV), torch.zeros((), device=DEV)
                conf = torch.zeros(ncls * ncls, dtype=torch.int64, device=DEV)
                if kind == "ce":
                    _lib.check(lib.fu_loss_ce(net._ctx, t.data_ptr(), ign, loss.data_ptr(), conf.data_ptr(), nv.data_ptr(), s))
                elif kind == "bce_dice":
                    _lib.check(lib.fu_loss_bce_dice(net._ctx, t.data_ptr(), ign, 0.7, loss.data_ptr(), s))
                else:
                    _lib.check(lib.fu_loss_ce_weighted(net._ctx, t.data_ptr(), ign, cw.data_ptr(), eps, loss.data_ptr(),
                                                       conf.data_ptr(), nv.data_ptr(), wsum.data_ptr(), s))
                net._flat_grad.zero_()
                net._backward_raw(None, DEV)
                out[f"{kind}/c{ncls}/{name}"] = digest(loss, nv, conf, wsum, net._flat_grad)


def optimiser(lib, out):
    def dev_scalars(fn, *a):
        host = (C.c_float * 8)()
        _lib.check(fn(*a, host))
        return torch.tensor(list(host), device=DEV)

    for cin, ncls, prec in ((3, 3, "fp32"), (4, 4, "fp32"), (4, 3, "fp16")):      # n % 4 = 3, 0, 3
        net = HipUNet(cin, ncls, base_channels=8, precision=prec).to(DEV).train()
        ctx, s = net._get_ctx(DEV, 1, 64, 64), net._stream(DEV)
        n, nb = net._total, net._total_bn
        assert (n % 4 == 0) == (ncls == 4)
        nbt = torch.zeros(len(net._bn), dtype=torch.int64, device=DEV)
        for shift in (0, 1, 3):
            for entry in ("adam", "adam_dev", "adam_ema", "adam_ema_dev") if prec == "fp32" else ("adam_ema",):
                g = torch.Generator(device=DEV).manual_seed(7 + cin + shift)

                def buf(count, rand=False):
                    t = torch.zeros(count + 8 + shift, device=DEV)[shift:shift + count]
                    assert t.data_ptr() % 16 == (4 * shift) % 16
                    return t.copy_(torch.randn(count, device=DEV, generator=g) * 0.1) if rand else t

                p, grad, m, v, rm, rv = buf(n, True), buf(n), buf(n), buf(n), buf(nb, True), buf(nb, True)
                ep, erm, erv = buf(n, True), buf(nb), buf(nb)
                _lib.check(lib.fu_bind_buffers(ctx, p.data_ptr(), grad.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr()))
                _lib.check(lib.fu_bind_adam_state(ctx, m.data_ptr(), v.data_ptr()))
                _lib.check(lib.fu_bind_ema_state(ctx, ep.data_ptr(), erm.data_ptr(), erv.data_ptr()))
                for step in (1, 2, 3):
                    grad.copy_(torch.randn(n, device=DEV, generator=g) * 10.0 ** (torch.arange(n, device=DEV) % 5 - 3.0))
                    if prec == "fp16" and step == 2:
                        grad[n // 2] = float("inf")                      # this step is skipped
                    w = (0.3, 0.5, 0.999)[step - 1]                       # both lerp branches
                    if entry == "adam":
                        _lib.check(lib.fu_adam_step(ctx, *ADAM, step, 0.5, s))
                    elif entry == "adam_dev":
                        sc = dev_scalars(lib.fu_adam_scalars, *ADAM, step, 0.5)
                        _lib.check(lib.fu_adam_step_dev(ctx, sc.data_ptr(), s))
                    elif entry == "adam_ema":
                        _lib.check(lib.fu_adam_ema_step(ctx, *ADAM, step, 0.5, w, s))
                    else:
                        sc = dev_scalars(lib.fu_adam_ema_scalars, *ADAM, step, 0.5, w)
                        _lib.check(lib.fu_adam_ema_step_dev(ctx, sc.data_ptr(), s))
                    torch.cuda.synchronize()
                out[f"{entry}/{prec}/n{n}/shift{shift}"] = digest(p, m, v, ep, erm, erv)
        _lib.check(lib.fu_bind_ema_state(ctx, None, None, None))
        net._bind(ctx)


def train_step(lib, net, x, tgt, by_block=False):
    s = net._stream(DEV)
    logits = net._forward_raw(x, True)
    loss, nv = torch.zeros((), device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    conf = torch.zeros(net.n_classes ** 2, dtype=torch.int64, device=DEV)
    _lib.check(lib.fu_loss_ce(net._ctx, tgt.data_ptr(), -100, loss.data_ptr(), conf.data_ptr(), nv.data_ptr(), s))
    net._flat_grad.zero_()
    if by_block:
        _lib.check(lib.fu_set_side_stream(net._ctx, 2))
        for b in range(lib.fu_num_blocks(net._ctx)):
            _lib.check(lib.fu_backward_block(net._ctx, b, None, s))
        _lib.check(lib.fu_backward_join(net._ctx, s))
        _lib.check(lib.fu_set_side_stream(net._ctx, 1))
    else:
        net._backward_raw(None, DEV)
    torch.cuda.synchronize()
    return digest(logits, loss, nv, conf, net._flat_grad, net._flat_rm, net._flat_rv, net._flat_nbt)


def steps(lib, out):
    def data(seed, c, h, w):
        torch.manual_seed(seed)
        return torch.rand(2, c, h, w, device=DEV), torch.randint(0, 3, (2, h, w), device=DEV)

    for prec in ("fp32", "bf16", "fp16"):
        for bilinear in (True, False):
            x, tgt = data(11, 4, 32, 32)
            net = HipUNet(4, 3, bilinear=bilinear, base_channels=8 if bilinear else 64, precision=prec).to(DEV).train()
            out[f"step/{prec}/{'bilinear' if bilinear else 'convT'}/32x32"] = train_step(lib, net, x, tgt)
    x, tgt = data(12, 4, 37, 45)
    net = HipUNet(4, 3, base_channels=8, precision="bf16").to(DEV).train()
    out["step/bf16/bilinear/37x45"] = train_step(lib, net, x, tgt)
    x, tgt = data(13, 5, 32, 32)
    net = HipLateFusion({"ms_image": 3, "dem": 2}, 3, base_channels=8, precision="bf16").to(DEV).train()
    out["step/bf16/latefusion2/32x32"] = train_step(lib, net, x, tgt)
    x, tgt = data(14, 4, 32, 32)
    net = HipUNet(4, 3, base_channels=8, precision="bf16").to(DEV).train()
    out["step/bf16/by_block/32x32"] = train_step(lib, net, x, tgt, by_block=True)
    # the eval paths, on the running statistics that the step above left
    net.eval()
    out["eval/bf16/srcs2/32x32"] = digest(net._forward_raw([x[:, :3], x[:, 3:]], False))
    logits = net.forward_views(x, [0, 1, 2, 3], want_logits=True)
    probs, counts = net.merge_views(target=tgt, ignore_index=-100)
    out["eval/bf16/views4/32x32"] = digest(logits, probs, counts)


def convs(lib, out):
    ptr, check = _lib.ptr, _lib.check
    s = torch.cuda.current_stream().cuda_stream

    def operands(dt, B, C0, Cout, H, W):
        g = torch.Generator().manual_seed(B + C0 + Cout + H + W)
        r = lambda *shape: torch.randn(*shape, generator=g)
        t = {"x": r(B, H, W, C0).to(DEV).to(dt), "dy": r(B, H, W, Cout).to(DEV).to(dt), "y": r(B, H, W, C0).to(DEV).to(dt),
             "w": (r(Cout, C0, 3, 3) / (3.0 * C0 ** 0.5)).to(DEV), "bias": r(Cout).to(DEV),
             "a": (torch.rand(C0, generator=g) + 0.5).to(DEV), "b": (r(C0) * 0.1).to(DEV),
             "mean": (r(C0) * 0.1).to(DEV), "invstd": (torch.rand(C0, generator=g) + 0.5).to(DEV)}
        return t

    def fwd(code, dt, B, C0, Cout, H, W, bn):
        t = operands(dt, B, C0, Cout, H, W)
        y, ssum, ssq = torch.zeros(B, H, W, Cout, device=DEV, dtype=dt), torch.zeros(Cout, device=DEV), torch.zeros(Cout, device=DEV)
        check(lib.fu_op_conv3x3_fwd(code, ptr(t["x"]), C0, ptr(t["a"]) if bn else None, ptr(t["b"]) if bn else None, None, 0,
                                    ptr(t["w"]), ptr(t["bias"]), ptr(y), Cout, B, H, W, ptr(ssum), ptr(ssq), s))
        return digest(y, ssum, ssq)

    def dgrad(code, dt, B, C0, Cout, H, W, sums):
        t = operands(dt, B, C0, Cout, H, W)
        dx, s1, s2 = torch.zeros(B, H, W, C0, device=DEV, dtype=dt), torch.zeros(C0, device=DEV), torch.zeros(C0, device=DEV)
        if sums:
            check(lib.fu_op_conv3x3_dgrad_bnsums(code, ptr(t["dy"]), Cout, ptr(t["w"]), ptr(dx), C0, ptr(t["y"]), ptr(t["a"]),
                                                 ptr(t["b"]), ptr(t["mean"]), ptr(t["invstd"]), ptr(s1), ptr(s2), B, H, W, s))
        else:
            check(lib.fu_op_conv3x3_dgrad(code, ptr(t["dy"]), Cout, ptr(t["w"]), ptr(dx), C0, None, 0, B, H, W, s))
        return digest(dx, s1, s2)

    def wgrad(code, dt, B, C0, Cout, H, W, bn):
        t = operands(dt, B, C0, Cout, H, W)
        dw = torch.zeros(Cout, C0, 3, 3, device=DEV)
        check(lib.fu_op_conv3x3_wgrad(code, ptr(t["x"]), C0, ptr(t["a"]) if bn else None, ptr(t["b"]) if bn else None, None, 0,
                                      ptr(t["dy"]), Cout, ptr(dw), B, H, W, s))
        return digest(dw)

    try:
        for code, dt, nm in ((_lib.FU_BF16, torch.bfloat16, "bf16"), (_lib.FU_F16, torch.float16, "fp16")):
            for mode in (3, 4):
                lib.fu_test_conv_tile_mode(mode)
                out[f"conv/{nm}/mode{mode}/fwd/64x64"] = fwd(code, dt, 1, 64, 64, 64, 64, True)
                out[f"conv/{nm}/mode{mode}/dgrad/64x64"] = dgrad(code, dt, 1, 64, 64, 64, 64, False)
                out[f"conv/{nm}/mode{mode}/dgrad_bnsums/64x64"] = dgrad(code, dt, 1, 64, 64, 64, 64, True)
            lib.fu_test_conv_tile_mode(0)
            for H in (16, 64):
                out[f"conv/{nm}/c8/fwd/{H}x16"] = fwd(code, dt, 1, 8, 64, H, 16, False)
            for general in (0, 1):
                lib.fu_test_force_general_conv(general)
                out[f"conv/{nm}/general{general}/fwd/37x45"] = fwd(code, dt, 2, 16, 24, 37, 45, True)
                out[f"conv/{nm}/general{general}/dgrad/37x45"] = dgrad(code, dt, 2, 16, 24, 37, 45, False)
            lib.fu_test_force_general_conv(0)
            for lock in (0, 1, 2):
                lib.fu_test_force_lockstep_wgrad(lock)
                out[f"conv/{nm}/lock{lock}/wgrad/c8"] = wgrad(code, dt, 1, 8, 64, 16, 32, False)
                out[f"conv/{nm}/lock{lock}/wgrad/c64"] = wgrad(code, dt, 1, 64, 64, 32, 32, True)
                out[f"conv/{nm}/lock{lock}/wgrad/c128"] = wgrad(code, dt, 1, 128, 64, 32, 32, True)
                out[f"conv/{nm}/lock{lock}/wgrad/37x45"] = wgrad(code, dt, 2, 16, 24, 37, 45, True)
                out[f"conv/{nm}/lock{lock}/wgrad/c256_3stages"] = wgrad(code, dt, 2, 256, 128, 80, 80, True)
            lib.fu_test_force_lockstep_wgrad(0)
            out[f"conv/{nm}/default/fwd/512wg"] = fwd(code, dt, 2, 32, 64, 256, 256, True)
            out[f"conv/{nm}/default/dgrad/512wg"] = dgrad(code, dt, 2, 64, 32, 256, 256, False)
            out[f"conv/{nm}/default/dgrad_bnsums/c64"] = dgrad(code, dt, 2, 64, 64, 256, 256, True)
            torch.manual_seed(15)
            x, tgt = torch.rand(2, 5, 32, 32, device=DEV), torch.randint(0, 3, (2, 32, 32), device=DEV)
            net = HipLateFusion({"ms_image": 3, "dem": 2}, 3, base_channels=8, precision=nm).to(DEV).train()
            out[f"conv/{nm}/one_tap/latefusion2"] = train_step(lib, net, x, tgt)
    finally:
        lib.fu_test_conv_tile_mode(0)
        lib.fu_test_force_general_conv(0)
        lib.fu_test_force_lockstep_wgrad(0)


def bn(lib, out):
    ptr, check = _lib.ptr, _lib.check
    s = torch.cuda.current_stream().cuda_stream
    precs = ((_lib.FU_F32, torch.float32, "fp32"), (_lib.FU_BF16, torch.bfloat16, "bf16"), (_lib.FU_F16, torch.float16, "fp16"))

    def coefficients(g, Cc):
        r = lambda *shape: torch.randn(*shape, generator=g)
        return [t.to(DEV) for t in (torch.rand(Cc, generator=g) + 0.5, r(Cc) * 0.1, r(Cc) * 0.1, torch.rand(Cc, generator=g) + 0.5)]

    for code, dt, nm in precs:
        for (B, Cc, H, W), pooled in (((1, 12, 5, 7), False), ((1, 8, 5, 7), True), ((2, 64, 32, 48), False), ((2, 64, 32, 48), True)):
            g = torch.Generator().manual_seed(B + Cc + H + W + pooled)
            y, gy = (torch.randn(B, H, W, Cc, generator=g).to(DEV).to(dt) for _ in range(2))
            gp = torch.randn(B, H // 2, W // 2, Cc, generator=g).to(DEV).to(dt) if pooled else None
            a, b, mean, invstd = coefficients(g, Cc)
            dgamma, dbeta = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
            check(lib.fu_op_bn_bwd(code, ptr(gy), ptr(y), Cc, B, H, W, ptr(a), ptr(b), ptr(mean), ptr(invstd), ptr(gp),
                                   ptr(dgamma), ptr(dbeta), s))
            out[f"bn/{nm}/bn_bwd/{B}x{Cc}x{H}x{W}/{'pooled' if pooled else 'plain'}"] = digest(gy, dgamma, dbeta)
    for code, dt, nm in precs[1:]:
        for ncls in (2, 3, 5):
            Cc, npix = 64, 2 * 40 * 48
            g = torch.Generator().manual_seed(ncls)
            y = torch.randn(npix, Cc, generator=g).to(DEV).to(dt)
            dl, w = (torch.randn(npix, ncls, generator=g) * 1e-3).to(DEV), (torch.randn(ncls, Cc, generator=g) * 0.2).to(DEV)
            a, b, mean, invstd = coefficients(g, Cc)
            gout = torch.zeros(npix, Cc, device=DEV, dtype=dt)
            dw, db, s1, s2 = (torch.zeros(n, device=DEV) for n in (ncls * Cc, ncls, Cc, Cc))
            check(lib.fu_op_head_bwd(code, ptr(dl), ptr(y), ptr(a), ptr(b), ptr(w), Cc, ncls, npix, ptr(gout), ptr(dw), ptr(db),
                                     ptr(mean), ptr(invstd), ptr(s1), ptr(s2), s))
            out[f"bn/{nm}/head_bwd_sums/c{ncls}"] = digest(gout, dw, db, s1, s2)
    for prec in ("fp32", "bf16"):
        torch.manual_seed(16)
        x, tgt = torch.rand(2, 4, 32, 32, device=DEV), torch.randint(0, 3, (2, 32, 32), device=DEV)
        net = HipUNet(4, 3, base_channels=8, precision=prec).to(DEV).train()
        ctx = net._get_ctx(DEV, 2, 32, 32)
        nbytes = int(lib.fu_exact_sync_bytes(ctx))
        xbuf = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device=DEV)
        calls = []

        def hook(_user, n_elems, is_double):
            (xbuf[:n_elems] if is_double else xbuf.view(torch.float32)[:n_elems]).mul_(2)     # two identical ranks, summed
            calls.append(n_elems)
            return 0

        cb = _lib.SYNC_HOOK(hook)
        check(lib.fu_set_exact_sync(ctx, cb, None, 2, ptr(xbuf), nbytes))
        try:
            out[f"bn/{prec}/exact_sync_world2/32x32"] = train_step(lib, net, x, tgt)
        finally:
            check(lib.fu_set_exact_sync(ctx, _lib.SYNC_HOOK(0), None, 1, None, 0))
        assert len(calls) >= 2 * len(net._bn), calls      # every BatchNorm's forward and backward sums went through the hook


def main():
    lib, out = _lib.load(), {}
    groups = sys.argv[1:] or ["losses", "optimiser", "steps", "convs", "bn"]
    if "losses" in groups:
        losses(lib, out)
    if "steps" in groups:
        steps(lib, out)
    if "optimiser" in groups:
        optimiser(lib, out)
    if "convs" in groups:
        convs(lib, out)
    if "bn" in groups:
        bn(lib, out)
    torch.cuda.synchronize()
    out["all"] = hashlib.sha256(json.dumps(out, sort_keys=True).encode()).hexdigest()
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
