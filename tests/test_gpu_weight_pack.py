"""GPU: the packed weight copies that a real step's conv kernels read, and the eval-mode BatchNorm fold inside them, against
tests/tools/pack_ref.py (checked on its own by test_pack_ref_cpu.py) -- bit for bit, through fu_test_get_pack.  A pack is
produced the way it is in use: by one forward through HipUNet / HipLateFusion on the smallest context the plan accepts (16x16
tiles, batch 1).  Every comparison is torch.equal-strict on the raw bits (numpy on the integer view); the one thing forgiven is
a NaN's payload.  +0.0 and -0.0 differ.

PARITY.  What each case reaches in fu_plan.hip's repack():
  k_pack_tiles_16<false / true>   every double conv of a bf16 / fp16 context.  First conv, n_channels in {1, 2, 7, 33}: the
                                  scalar read loop (cin_real % 4 != 0); {4, 12, 36, 64}: the float4 pieces; all but 64 have
                                  cin_pad > cin_real (padding that must be +0.0 bits, in eval mode too, where the fold scale
                                  may be negative); 33 / 36: a second c_in tile holding 1 / 4 real channels; 64: two full
                                  ones.  Base 8 and 16: partial c_out tiles (8, 16 channels); base 32: 256 x 256 and
                                  512 x 256 layers, several full tiles both ways.
  k_pack_all<float, false>        the same cases in fp32 (cin_pad = cin_real rounded up to 4).
  two PackTables                  a 3-encoder HipLateFusion at base 8 has 38 double convs, MAX_PACK = 32 per launch.
  k_center_to_w3 + k_pack_*       its five fusion convs, against pack_ref(center_w3_ref(w)).
  k_convT_to_w3 + k_pack_*        the four transposed convs of the bilinear=False net (base 64, bf16), against convT_w3_ref,
                                  with bias4; the centre tap element for element, every other tap all-zero bits.
  k_bn_fold_eval + use_scale      eval mode of every case: fold_scale / fold_bias == fold_ref, a == 1, b == 0, the packs ==
                                  pack_ref(scale = fold_scale).  Statistics come in through load_state_dict: running_var in
                                  [0.05, 4] and one channel exactly 0, gamma with a 0 and negative entries, conv bias != 0.
The 16-bit instantiations of k_pack_all are NOT covered and cannot be: fu_create admits 16-bit contexts only at base >= 8, where
every c_out and cin_pad is a multiple of 8, so repack's tiled_ok is always true and the tiled kernel always runs.
Weights are seeded, then a few per layer are overwritten with +-0.0, exact bf16 and fp16 round-to-even ties in both directions,
fp16 subnormals, values below half the smallest fp16 subnormal, 65520 and 70000 (inf in fp16, finite in bf16), -1e-30, and one
NaN in one layer.  Each reference holds exactly the 9 * cin_pad * cout elements the hook's fields give and that many are read
back: a check of the layout's shape, not of where the device buffer ends (a write past the end is not seen here).

FRESHNESS (bf16 and fp32, base 8).  After each step the live flat parameters and running statistics are read at that moment
and all packs must equal their reference; where the step changed the parameters the packs must also differ from the previous
step's, so nothing passes vacuously: first training forward; eval right after (the fold uses the statistics the training
forward just moved); training after eval (plain again); train_step + adam_step then training / eval; eval, a bare fu_adam_step
(the module's own flag untouched: the C-side flag alone), eval; load_state_dict between two evals (the module's flag alone);
forward_views as the first eval entry after a change; the EMA block (packs and fold from the EMA buffers, load_ema_state_dict
inside it, live again after it); a new context for a larger batch and another tile size; three replays of the captured
DataParallelTrainer step, whose pack runs at the head of the step and therefore shows the parameters from before it.

WHAT CATCHES WHAT.  A wd slot or tap error: every 16-bit parity case (and the freshness cases in bf16).  Wrong statistics or
arithmetic in the fold: every case with an eval pack, through fold_scale / fold_bias and then the packs.  A missing
packed_dirty in the optimiser step: step 5 of test_packs_follow_mode_switches_and_optimiser_steps alone, since every other
path also raises the module's own flag.  (fu_plan.hip's comments name the two eval-pack defects these tests found.)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib
from floodplanet_code_amd._lib import check
from floodplanet_code_amd.latefusion import HipLateFusion
from floodplanet_code_amd.unet import HipUNet

sys.path.insert(0, os.path.dirname(__file__))
from tools import pack_ref as R                               # noqa: E402
from tools.hip_mem import memcpy_dtod as _memcpy_dtod         # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32

# exact ties: bf16 keeps 8 significant bits, fp16 11; the even neighbour is below for 1 + u/2 and above for 1 + 3u/2
EDGES = [0.0, -0.0,
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),            # bf16 ties, both directions
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11),        # fp16 ties
         2.0 ** -14 * (1 + 2.0 ** -11),                                                    # fp16: tie at the smallest normal
         3.3e-6, -2.0 ** -24 * 2.5, 2.0 ** -24 * 1.5,                                      # fp16 subnormals (inexact, and ties)
         2.0 ** -25, -(2.0 ** -26), 2.0 ** -25 * 1.0000001,                                # at, below and just above half the smallest
         65520.0, -65520.0, 70000.0, 65519.996, -1e-30]
NAN_LAYER = "up4.conv.double_conv.3.weight"       # (suffix) the one layer that also gets a NaN


# ----------------------------------------------------------------------------------------------------------------------
# nets and states
# ----------------------------------------------------------------------------------------------------------------------
def _with_edges(net, seed):
    """state_dict of `net` (constructed under a fixed seed) with the EDGES written into every 4-d weight at seeded places."""
    g = torch.Generator().manual_seed(seed)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    for k, v in sd.items():
        if v.dim() != 4:
            continue
        flat = v.view(-1)
        vals = EDGES + ([float("nan")] if k.endswith(NAN_LAYER) else [])
        idx = (torch.arange(len(vals)) * 37 + int(torch.randint(0, 1 << 20, (1,), generator=g))) % flat.numel()
        flat[idx] = torch.tensor(vals, dtype=torch.float32)[: len(idx)]
    return sd


def _with_eval_stats(net, sd, seed):
    """sd with the running statistics, affine parameters and conv biases of the eval-fold cases."""
    g = torch.Generator().manual_seed(seed)
    sd = dict(sd)
    for name, m, _ in net._bn:
        c = m.weight.numel()
        gamma = torch.randn(c, generator=g)
        gamma[0], gamma[2] = 0.0, -gamma[2].abs() - 0.25
        rv = torch.rand(c, generator=g) * 3.95 + 0.05
        rv[1] = 0.0
        sd[name + ".weight"], sd[name + ".bias"] = gamma, torch.randn(c, generator=g)
        sd[name + ".running_mean"], sd[name + ".running_var"] = torch.randn(c, generator=g), rv
    for k, v in sd.items():
        if v.dim() == 1 and k.endswith(".bias") and k[: -len(".bias")] not in {n for n, _, _ in net._bn}:
            sd[k] = torch.randn(v.shape, generator=g) * 0.5 + 0.05
    return sd


def _x(net, B=1, H=16, W=16, seed=1):
    return torch.randn(B, net.n_channels, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)


# ----------------------------------------------------------------------------------------------------------------------
# what the hook exposes, read back, and its reference
# ----------------------------------------------------------------------------------------------------------------------
def _get_pack(net, kind, index, which=0):
    out = _lib.FuTestPack()
    check(_lib.load().fu_test_get_pack(net._ctx, kind, index, which, C.byref(out)))
    return out if out.present else None


def _layout(net):
    """Every pack of the net's current context: [(tag, kind, block or level, which, FuTestPack)], and the C side's parameter /
    BatchNorm tables."""
    lib = _lib.load()
    n_enc = max(1, net._enc_config()[0])
    nb = 5 * n_enc + 4
    packs = [(f"block{i}.conv{j}", 0, i, j, _get_pack(net, 0, i, j)) for i in range(nb) for j in range(2)]
    assert all(p is not None for *_, p in packs)
    packs += [(f"fuse{l}", 1, l, 0, p) for l in range(5) for p in [_get_pack(net, 1, l)] if p is not None]
    packs += [(f"block{i}.convT", 2, i, 0, p) for i in range(5 * n_enc, nb) for p in [_get_pack(net, 2, i)] if p is not None]
    params, by_name = [], {}
    name, ndim, shape, off = C.c_char_p(), C.c_int32(), (C.c_int64 * 4)(), C.c_int64()
    for i in range(lib.fu_num_params(net._ctx)):
        check(lib.fu_param_info(net._ctx, i, C.byref(name), C.byref(ndim), shape, C.byref(off)))
        params.append((name.value.decode(), tuple(shape[: ndim.value]), off.value))
        by_name[params[-1][0]] = i
    bns, ch = [], C.c_int32()
    for i in range(lib.fu_num_bn(net._ctx)):
        check(lib.fu_bn_info(net._ctx, i, C.byref(name), C.byref(ch), C.byref(off)))
        bns.append((name.value.decode(), ch.value, off.value))
    return packs, params, by_name, bns


def _read(ptr, n, prec):
    """n elements at a device pointer -> numpy: float32, or the uint16 codes of a 16-bit type."""
    dt = torch.float32 if prec == "fp32" else torch.int16
    t = torch.empty(n, dtype=dt, device=DEV)
    _memcpy_dtod(t.data_ptr(), ptr, n * t.element_size())
    a = t.cpu().numpy()
    return a if prec == "fp32" else a.view(np.uint16)


def _bound(net):
    """The flat buffers the context reads right now (inside ema_weights(): the EMA ones), copied to the host."""
    torch.cuda.synchronize()
    src = net.ema_buffers() if net.ema_serving else (net._flat, net._flat_rm, net._flat_rv)
    return tuple(t.detach().cpu().numpy().copy() for t in src)


def _param(P, params, i):
    _, shape, off = params[i]
    return P[off: off + int(np.prod(shape))].reshape(shape)


def _check_packs(net, state, eval_mode, only=None):
    """All packs of the context (or the tags in `only`) against the reference of `state` = (P, RM, RV) host copies.
    Returns the concatenated wf bits, for the 'did it change' assertions."""
    prec = net.precision
    assert prec in R.PRECS
    P, RM, RV = state
    packs, params, by_name, bns = _layout(net)
    torch.cuda.synchronize()
    seen = []
    n_enc = max(1, net._enc_config()[0])
    for tag, kind, block, which, p in packs:
        if only is not None and tag not in only:
            continue
        n = 9 * p.cin_pad * p.cout
        pname, pshape, _ = params[p.p_weight]
        bias = _param(P, params, p.p_bias)
        first = kind == 0 and p.wd is None
        align = 4 if prec == "fp32" else 8
        assert p.cin_pad == (-(-p.cin_real // align) * align if first else p.cin_real), (tag, p.cin_real, p.cin_pad)
        # no dgrad copy exactly for conv 0 of an encoder's first block (blocks run inc, down1..4 per encoder, then up1..4)
        assert first == (kind == 0 and which == 0 and block < 5 * n_enc and block % 5 == 0), tag
        scale = None
        if kind == 0:
            assert pshape == (p.cout, p.cin_real, 3, 3) and params[p.p_bias][1] == (p.cout,) and p.bn >= 0, (tag, pshape)
            w = _param(P, params, p.p_weight)
            bname, bc, boff = bns[p.bn]
            stem, bn_idx = bname.rsplit(".", 1)                 # double_conv.0 / .3 are the convs, .1 / .4 their BatchNorms
            assert bc == p.cout and pname == f"{stem}.{ {'1': '0', '4': '3'}[bn_idx]}.weight", (pname, bname)
            if eval_mode:
                gamma, beta = (_param(P, params, by_name[bname + s]) for s in (".weight", ".bias"))
                scale, fbias = R.fold_ref(gamma, beta, RM[boff: boff + bc], RV[boff: boff + bc], bias)
                for what, ptr, want in (("fold_scale", p.fold_scale, scale), ("fold_bias", p.fold_bias, fbias),
                                        ("a", p.a, np.ones(bc, f32)), ("b", p.b, np.zeros(bc, f32))):
                    got = _read(ptr, bc, "fp32")
                    bad = R.mismatches(got, want, "fp32")
                    assert bad.size == 0, (f"{tag} {what}: {bad.size} of {bc} channels differ, first c={bad[0]}: got "
                                           f"{got[bad[0]]!r} ({got.view(np.uint32)[bad[0]]:#x}) want {want[bad[0]]!r} "
                                           f"({want.view(np.uint32)[bad[0]]:#x}); gamma {gamma[bad[0]]!r} beta {beta[bad[0]]!r} "
                                           f"rm {RM[boff + bad[0]]!r} rv {RV[boff + bad[0]]!r} bias {bias[bad[0]]!r}")
        elif kind == 1:
            assert pshape == (p.cout, p.cin_real, 1, 1) and p.bn == -1 and p.cin_real == net._enc_config()[0] * p.cout
            w = R.center_w3_ref(_param(P, params, p.p_weight))
        else:
            assert pshape == (p.cin_real, p.cout // 4, 2, 2) and p.bn == -1 and p.bias4, (tag, pshape)
            w, b4 = R.convT_w3_ref(_param(P, params, p.p_weight), bias)
            assert R.mismatches(_read(p.bias4, p.cout, "fp32"), b4.numpy(), "fp32").size == 0, tag
        wf_ref, wd_ref = R.pack_ref(w, p.cin_pad, prec, scale=scale)
        assert wf_ref.size == n and wd_ref.size == n, (tag, n)
        for what, ptr, want in (("wf", p.wf, wf_ref), ("wd", p.wd, wd_ref)):
            if what == "wd" and first:
                continue                                   # the first conv of an encoder has no dgrad copy
            assert ptr, (tag, what)
            got = _read(ptr, n, prec).reshape(want.shape)
            bad = R.mismatches(got, want, prec)
            if bad.size:
                i = np.unravel_index(bad[0], want.shape)
                raise AssertionError(f"{tag} {what} ({pname}, cout {p.cout} cin {p.cin_real}/{p.cin_pad}, "
                                     f"{'eval' if eval_mode else 'train'}): {bad.size} of {n} elements differ, first at "
                                     f"{tuple(int(v) for v in i)}: got {got[i]!r} want {want[i]!r}")
            if kind != 0:       # an embedded 1x1: the centre tap holds everything, all other taps are all-zero bits
                raw = got.view(np.uint32) if prec == "fp32" else got
                assert not raw[[0, 1, 2, 3, 5, 6, 7, 8]].any() and raw[4].any(), (tag, what)
            if what == "wf":
                seen.append(got.view(np.uint32 if prec == "fp32" else np.uint16).ravel().copy())
    assert seen, only
    return np.concatenate([s.astype(np.uint32) for s in seen])


def _parity(net, sd_edges, x):
    """One training forward and one eval forward of a fresh module, all packs against the reference each time."""
    net.load_state_dict(sd_edges)
    net.to(DEV).train()
    with torch.no_grad():
        net(x)
        plain = _check_packs(net, _bound(net), eval_mode=False)
        net.load_state_dict(_with_eval_stats(net, sd_edges, seed=5))
        net.eval()
        net(x)
        folded = _check_packs(net, _bound(net), eval_mode=True)
    assert not np.array_equal(plain, folded)              # the fold did change the packs


# ----------------------------------------------------------------------------------------------------------------------
# parity
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("n_channels", [1, 2, 4, 7, 12, 33, 36, 64])
def test_first_conv_geometry_at_base_8(n_channels, prec):
    torch.manual_seed(100 + n_channels)
    net = HipUNet(n_channels, 3, base_channels=8, precision=prec)
    _parity(net, _with_edges(net, seed=n_channels), _x(net))


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("base", [16, 32])
def test_wider_nets_partial_and_full_tiles(base, prec):
    torch.manual_seed(base)
    net = HipUNet(5, 3, base_channels=base, precision=prec)
    _parity(net, _with_edges(net, seed=base), _x(net))


@pytest.mark.parametrize("prec", R.PRECS)
def test_late_fusion_two_pack_tables_and_fusion_convs(prec):
    torch.manual_seed(38)
    net = HipLateFusion({"ms_image": 7, "dem": 1, "slope": 4}, 3, base_channels=8, precision=prec)
    sd = _with_edges(net, seed=3)
    net.load_state_dict(sd)
    net.to(DEV).train()
    with torch.no_grad():
        net(_x(net))
    packs = _layout(net)[0]
    kinds = [k for _, k, *_ in packs]
    assert kinds.count(0) == 38 and kinds.count(1) == 5 and kinds.count(2) == 0      # 38 > MAX_PACK = 32
    _parity(net, sd, _x(net))


def test_transposed_conv_net_bf16():
    torch.manual_seed(64)
    net = HipUNet(4, 3, bilinear=False, base_channels=64, precision="bf16")
    sd = _with_edges(net, seed=9)
    net.load_state_dict(sd)
    net.to(DEV).train()
    x = _x(net)
    only = {"block0.conv0", "block6.conv1"} | {f"block{i}.convT" for i in range(5, 9)}    # (two double convs: host time)
    with torch.no_grad():
        net(x)
        packs = _layout(net)[0]
        assert [t for t, k, *_ in packs if k == 2] == sorted(t for t in only if t.endswith("convT"))
        assert _get_pack(net, 1, 0) is None                                               # no fusion convs here
        plain = _check_packs(net, _bound(net), eval_mode=False, only=only)
        net.load_state_dict(_with_eval_stats(net, sd, seed=5))
        net.eval()
        net(x)
        folded = _check_packs(net, _bound(net), eval_mode=True, only=only)
    assert not np.array_equal(plain, folded)


def test_hook_reports_bad_arguments_and_absent_kinds():
    torch.manual_seed(0)
    net = HipUNet(3, 3, base_channels=8, precision="bf16").to(DEV).eval()
    with torch.no_grad():
        net(_x(net))
    lib, out = _lib.load(), _lib.FuTestPack()
    for kind, index, which in ((0, -1, 0), (0, 9, 0), (0, 0, 2), (0, 0, -1), (1, 5, 0), (1, -1, 0), (1, 0, 1), (2, 4, 0),
                               (2, 9, 0), (2, 5, 1), (3, 0, 0), (-1, 0, 0)):
        assert lib.fu_test_get_pack(net._ctx, kind, index, which, C.byref(out)) == _lib.FU_ERR_INVALID, (kind, index, which)
        assert b"fu_test_get_pack" in lib.fu_last_error()
    assert lib.fu_test_get_pack(net._ctx, 0, 0, 0, None) == _lib.FU_ERR_INVALID
    assert lib.fu_test_get_pack(None, 0, 0, 0, C.byref(out)) == _lib.FU_ERR_INVALID
    for kind, index in ((1, 0), (1, 4), (2, 5), (2, 8)):           # a plain bilinear UNet has neither kind
        out.cout = 77
        check(lib.fu_test_get_pack(net._ctx, kind, index, 0, C.byref(out)))
        assert out.present == 0 and not out.wf and not out.wd and out.cout == 0 and (out.p_weight, out.p_bias, out.bn) == (-1,) * 3
    p = _get_pack(net, 0, 0, 0)
    assert p.wf and not p.wd and (p.cout, p.cin_real, p.cin_pad, p.bn) == (8, 3, 8, 0) and not p.bias4
    p = _get_pack(net, 0, 8, 1)
    assert p.wf and p.wd and p.fold_scale and p.fold_bias and p.a and p.b and (p.cout, p.cin_real, p.bn) == (8, 8, 17)


# ----------------------------------------------------------------------------------------------------------------------
# freshness
# ----------------------------------------------------------------------------------------------------------------------
class _Fresh:
    """A net under test and the packs of the previous step."""

    def __init__(self, prec, n_channels=5, seed=0):
        torch.manual_seed(seed)
        self.net = HipUNet(n_channels, 3, base_channels=8, precision=prec).to(DEV)
        self.prev = None
        g = torch.Generator().manual_seed(seed + 1)
        self.x = torch.randn(2, n_channels, 16, 16, generator=g).to(DEV)
        self.t = torch.randint(0, 3, (2, 16, 16), generator=g).to(DEV)
        self.step = 0

    def forward(self, training, B=1, x=None):
        self.net.train(training)
        with torch.no_grad():
            self.net(self.x[:B] if x is None else x)

    def optimise(self, lr=1e-2, B=2):
        self.net.train()
        self.net.train_step(self.x[:B], self.t[:B], 0)
        self.step += 1
        self.net.adam_step(lr, self.step)

    def check(self, eval_mode, changed, state=None):
        """The packs equal the reference of the buffers bound now (or of `state`); changed: they differ from / equal the
        previous check's."""
        state = _bound(self.net) if state is None else state
        assert all(np.isfinite(s).all() for s in state)          # (a NaN would match anything)
        cur = _check_packs(self.net, state, eval_mode)
        if changed is not None:
            assert self.prev is not None and (not np.array_equal(cur, self.prev)) == changed
        self.prev = cur


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_packs_follow_mode_switches_and_optimiser_steps(prec):
    f = _Fresh(prec)
    net = f.net
    f.forward(True)
    f.check(False, None)                        # 1. first training forward
    rm0 = net._flat_rm.clone()
    f.forward(False)
    assert not torch.equal(rm0, torch.zeros_like(rm0))          # the training forward did move the running statistics
    f.check(True, True)                         # 2. eval right after: the fold uses the statistics just moved
    f.forward(True)
    f.check(False, True)                        # 3. training after eval: plain again, no scale left
    f.optimise()
    f.forward(True)
    f.check(False, True)                        # 4a. train_step + adam_step, then a training forward
    f.optimise()
    f.forward(False)
    f.check(True, True)                         # 4b. ... then an eval forward
    # 5. eval, a bare fu_adam_step with the module's own flag untouched, eval: the C-side flag alone
    before = net._flat.clone()
    assert net._eval_dirty is False
    check(_lib.load().fu_adam_step(net._ctx, 1e-2, 0.9, 0.999, 1e-8, f.step + 1, 1.0, net._stream(net._flat.device)))
    assert net._eval_dirty is False
    f.step += 1
    f.forward(False)
    assert not torch.equal(before, net._flat)
    f.check(True, True)
    # 6. load_state_dict of other weights between two eval forwards: the module's flag alone
    sd = {k: (v * 1.25 + 0.01 if v.is_floating_point() else v) for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    f.forward(False)
    f.check(True, True)
    f.forward(False)
    f.check(True, False)                        # nothing changed: the same packs


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_forward_views_packs_after_a_parameter_change(prec):
    f = _Fresh(prec)
    f.forward(True, B=2)
    f.check(False, None)
    f.optimise()
    f.net.eval()
    f.net.forward_views(f.x[:1], "hflip")       # 7. two views of one crop: the first eval entry after the step
    f.check(True, True)
    f.optimise()
    f.net.eval()
    f.net.forward_views(f.x[:1], "hflip")
    f.check(True, True)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_ema_block_packs_come_from_the_ema_buffers(prec):
    f = _Fresh(prec)
    net = f.net
    f.forward(False)
    net.enable_ema(0.5, warmup=False)
    for _ in range(3):
        f.optimise(lr=3e-2)
    f.forward(False)
    f.check(True, None)
    live = _bound(net)
    with net.ema_weights():                     # 8. inside the block: the EMA parameters and EMA running statistics
        ema = _bound(net)
        assert not any(np.array_equal(a, b) for a, b in zip(live, ema))
        f.forward(False)
        f.check(True, True, state=ema)
        sd = {k: (v * 0.75 - 0.02 if v.is_floating_point() else v) for k, v in net.ema_state_dict().items()}
        net.load_ema_state_dict(sd)             # picked up by the next eval forward
        f.forward(False)
        ema2 = _bound(net)
        assert not np.array_equal(ema[0], ema2[0]) and not np.array_equal(ema[2], ema2[2])
        f.check(True, True, state=ema2)
    f.forward(False)
    assert all(np.array_equal(a, b) for a, b in zip(live, _bound(net)))       # the live buffers came back untouched
    f.check(True, True, state=live)             # after the block: the live buffers again


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_new_contexts_pack_on_their_first_forward(prec):
    f = _Fresh(prec)
    f.forward(False)
    f.check(True, None)
    assert f.net._ctx_key[1:] == (16, 16, 1)
    f.optimise(B=1)                             # (one tile: the step stays on the batch-1 context)
    assert f.net._ctx_key[1:] == (16, 16, 1)
    f.forward(True, B=2)                        # 9. a larger batch: a new context, its first forward a training one ...
    assert f.net._ctx_key[1:] == (16, 16, 2)
    f.check(False, True)
    g = torch.Generator().manual_seed(4)
    f.optimise()
    f.forward(False, x=torch.randn(3, 5, 16, 16, generator=g).to(DEV))      # ... or an eval one
    assert f.net._ctx_key[1:] == (16, 16, 3)
    f.check(True, True)
    f.optimise()
    f.forward(False, x=torch.randn(1, 5, 32, 16, generator=g).to(DEV))      # ... then another tile size
    assert f.net._ctx_key[1:] == (32, 16, 1)
    f.check(True, True)
    f.forward(True, x=torch.randn(1, 5, 16, 48, generator=g).to(DEV))
    assert f.net._ctx_key[1:] == (16, 48, 1)
    f.check(False, True)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_captured_step_packs_the_parameters_from_before_the_step(prec):
    """10. DataParallelTrainer(graph=True), one device: the pack is the first node of the captured step, so after a replay the
    packs are those of the parameters as they were before it (default queue settings, no environment variables)."""
    from floodplanet_code_amd.distributed import DataParallelTrainer
    f = _Fresh(prec)
    net = f.net.train()
    tr = DataParallelTrainer(net, lr=1e-2, graph=True)
    tr.step(f.x, f.t, 0)                        # eager: makes the context
    assert tr._graph is None
    for it in range(3):
        before = _bound(net)
        tr.step(f.x, f.t, 0)
        assert tr._graph is not None
        after = _bound(net)
        assert not np.array_equal(before[0], after[0])
        f.check(False, True if it else None, state=before)
