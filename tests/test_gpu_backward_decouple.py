"""GPU: the backward's weight-gradient chains run decoupled from the caller's stream -- every conv has its own
bias-gradient partials, so the caller's stream never waits for the chain of an earlier conv inside a backward; the
joins order the reuse from one backward to the next.  No kernel and no dispatch decision differs from the serial chain
(fu_set_side_stream(ctx, 0)), so every comparison here is BITWISE: the failure mode of the change is a missing
dependency -- a buffer written before its last reader is done -- which shows as wrong numbers, most easily with short
kernels, where the caller's stream runs many convs ahead of the chains.  Hence the small shapes.

Cases (the issue's table): base-64 net, 8 bands, 64 x 64, B = 2 in bf16 and fp16 (ping-pong and lock-step-64 wgrad, the
8-band wgrad, k_wgrad_reduce_oihw at small and large split counts); base-8 net, 32 x 32, B = 2 in fp32 (k_wgrad_reduce +
k_wgrad_transpose); a ConvTranspose net in fp32 (shares the workspace on the caller's stream) -- at base 64, not base 8
as the issue's table has it: fu_create takes bilinear = 0 at base_channels 64 only; a two-encoder late-fusion net, base 8,
in bf16 (the fusion block joins mid-backward and then uses the context-level buffers)."""
import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd.latefusion import HipLateFusion
from floodplanet_code_amd.unet import HipUNet
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INT_OF_SIZE = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def bit_mismatches(a, b):
    """Number of elements of a whose bit pattern differs from b's (NaN payloads and the sign of zero count)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    ia = a.detach().reshape(-1).contiguous().view(INT_OF_SIZE[a.element_size()])
    ib = b.detach().reshape(-1).contiguous().view(INT_OF_SIZE[b.element_size()])
    return int((ia != ib).sum().item())


def first_mismatch(got, want):
    """got / want: dicts name -> tensor.  None when every tensor is equal as bit patterns, else (name, count)."""
    assert got.keys() == want.keys()
    for k in got:
        n = bit_mismatches(got[k], want[k])
        if n:
            return k, n
    return None


def snapshot(net, loss=None):
    """Copies, on the current stream and without a host synchronisation, of what a step leaves behind."""
    out = {"grads": net.flat_grads().clone(), "params": net.flat_parameters().clone(),
           "bn_running_mean": net._flat_rm.clone(), "bn_running_var": net._flat_rv.clone()}
    if loss is not None:
        out["loss"] = loss.reshape(1).clone()
    return out


def make_net(kind, prec):
    torch.manual_seed(0)
    if kind == "unet64":
        net, shape = HipUNet(8, 3, base_channels=64, precision=prec), (2, 8, 64, 64)
    elif kind == "unet8":
        net, shape = HipUNet(8, 3, base_channels=8, precision=prec), (2, 8, 32, 32)
    elif kind == "convT64":
        net, shape = HipUNet(8, 3, bilinear=False, base_channels=64, precision=prec), (2, 8, 32, 32)
    else:
        net, shape = HipLateFusion({"ms_image": 5, "dem": 3}, 3, base_channels=8, precision=prec), (2, 8, 32, 32)
    b = O.make_batch(*shape, seed=21)
    return net.to(DEV).train(), b["image"].to(DEV), b["target"].to(DEV)


def set_mode(net, x, mode):
    ctx = net._get_ctx(DEV, x.shape[0], x.shape[2], x.shape[3])
    _lib.check(_lib.load().fu_set_side_stream(ctx, mode))
    return ctx


def run_steps(kind, prec, mode, steps=5):
    net, x, t = make_net(kind, prec)
    set_mode(net, x, mode)
    snaps = []
    for k in range(1, steps + 1):                      # no host synchronisation between the steps
        net._forward_raw(x, True, want_logits=False)
        loss = net._loss_raw(t, 0, DEV)
        net._backward_raw(None, DEV)
        net.adam_step(1e-3, k)
        snaps.append(snapshot(net, loss))
    torch.cuda.synchronize()
    set_mode(net, x, 1)
    return snaps


@pytest.mark.parametrize("kind,prec", [("unet64", "bf16"), ("unet64", "fp16"), ("unet8", "fp32"), ("convT64", "fp32"),
                                       ("latefusion8", "bf16")])
def test_serial_equals_decoupled_over_steps(kind, prec):
    """Five consecutive train steps (forward, CE with ignore_index 0, backward, Adam) from the same state and batch, once on
    the serial chain and once decoupled: loss, flat gradients, parameters and BatchNorm running statistics are equal as bit
    patterns after every step."""
    serial = run_steps(kind, prec, 0)
    decoupled = run_steps(kind, prec, 1)
    assert float(serial[0]["grads"].abs().max()) > 0 and bool(torch.isfinite(serial[-1]["params"]).all())
    assert first_mismatch(serial[0], serial[1]) is not None          # the steps do move the state
    for k, (a, b) in enumerate(zip(serial, decoupled)):
        assert first_mismatch(b, a) is None, (k, first_mismatch(b, a))


def _forward_loss(net, x, t):
    net._forward_raw(x, True, want_logits=False)
    net._loss_raw(t, 0, DEV)
    net._flat_grad.zero_()                              # a launch that never ran must not pass on an earlier run's values


def test_blockwise_entry_with_fence_equals_whole_backward():
    """fu_backward_block over all blocks in mode 2, fu_backward_fence after a middle block onto a second stream,
    fu_backward_join after the last: the gradients equal fu_backward's bit for bit, and a copy of the fenced blocks'
    gradient ranges made ON the fenced stream equals the final gradients of those ranges -- the fence covers the side
    stream, where the weight and bias gradients are written."""
    lib = _lib.load()
    net, x, t = make_net("unet64", "bf16")
    _forward_loss(net, x, t)
    net._backward_raw(None, DEV)
    whole = net.flat_grads().clone()
    _forward_loss(net, x, t)
    ctx = set_mode(net, x, 2)
    s = net._stream(DEV)
    other = torch.cuda.Stream(device=DEV)
    nb = lib.fu_num_blocks(ctx)
    ranges = net.block_ranges()
    mid = nb // 2
    fenced = {}
    try:
        for b in range(nb):
            _lib.check(lib.fu_backward_block(ctx, b, None, s))
            if b == mid:
                _lib.check(lib.fu_backward_fence(ctx, s, other.cuda_stream))
                with torch.cuda.stream(other):
                    for k in range(mid + 1):
                        off, n = ranges[k]
                        fenced[k] = net.flat_grads()[off:off + n].clone()
        _lib.check(lib.fu_backward_join(ctx, s))
    finally:
        _lib.check(lib.fu_set_side_stream(ctx, 1))
    torch.cuda.synchronize()
    final = net.flat_grads()
    assert float(whole.abs().max()) > 0
    assert bit_mismatches(final, whole) == 0
    assert len(fenced) == mid + 1
    for k, g in fenced.items():
        off, n = ranges[k]
        assert n > 0 and float(g.abs().max()) > 0, k
        assert bit_mismatches(g, final[off:off + n]) == 0, k


def test_two_backwards_of_one_loss():
    """fu_backward twice without a forward in between: the same gradients both times, equal to the serial chain's."""
    net, x, t = make_net("unet64", "bf16")
    set_mode(net, x, 0)
    _forward_loss(net, x, t)
    net._backward_raw(None, DEV)
    serial = net.flat_grads().clone()
    set_mode(net, x, 1)
    _forward_loss(net, x, t)
    net._backward_raw(None, DEV)
    first = net.flat_grads().clone()
    net._flat_grad.zero_()
    net._backward_raw(None, DEV)
    second = net.flat_grads().clone()
    torch.cuda.synchronize()
    assert float(serial.abs().max()) > 0
    assert bit_mismatches(first, serial) == 0
    assert bit_mismatches(second, serial) == 0


def test_captured_step_keeps_its_topology():
    """DataParallelTrainer(graph=True) on the base-64 64 x 64 net: the captured step forks to the side stream and joins it
    as the eager one does (two branches, no wait between them but the fork and the join); three replayed steps equal three
    eager steps bitwise."""
    from floodplanet_code_amd.distributed import DataParallelTrainer
    outs = []
    for graph in (False, True):
        net, x, t = make_net("unet64", "bf16")
        tr = DataParallelTrainer(net, lr=1e-3, graph=graph)
        snaps = []
        for _ in range(4):                               # graph=True: one eager step (it creates the context), three replays
            loss = tr.step(x, t, 0)
            snaps.append(snapshot(net, loss))
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph
        outs.append(snaps)
    eager, replayed = outs
    assert first_mismatch(eager[0], eager[1]) is not None
    for k in range(4):
        assert first_mismatch(replayed[k], eager[k]) is None, (k, first_mismatch(replayed[k], eager[k]))


def test_comparison_helper_sees_one_flipped_mantissa_bit():
    """Negative control: one flipped low mantissa bit in one array is a mismatch; so are -0.0 against +0.0."""
    a = {"grads": torch.linspace(-1.0, 1.0, 1001, device=DEV), "params": torch.ones(7, device=DEV)}
    b = {k: v.clone() for k, v in a.items()}
    assert first_mismatch(a, b) is None
    b["grads"].view(torch.int32)[500] ^= 1
    assert first_mismatch(a, b) == ("grads", 1)
    assert torch.allclose(a["grads"], b["grads"], rtol=0, atol=1e-7)       # (a difference a tolerance would not have seen)
    assert bit_mismatches(torch.zeros(3, device=DEV), -torch.zeros(3, device=DEV)) == 3
    h = torch.ones(4, device=DEV, dtype=torch.bfloat16)
    g = h.clone()
    g.view(torch.int16)[2] ^= 1
    assert bit_mismatches(h, g) == 1
