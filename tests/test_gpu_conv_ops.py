"""GPU: the 3x3 convolutions on their own, through fu_op_conv3x3_fwd / _dgrad / _wgrad / _dgrad_bnsums, element by element against
the fp64 reference and the analytic bounds of tests/tools/conv_ref.py (derived there; test_conv_ref_cpu.py holds a float32
restatement to them and proves the route of every table entry) -- never against the code under test.

Every entry of conv_ref.TABLE (every ConvRoute in forward and dgrad, every WgradRoute and the ping-pong kernel's three stagings,
both TH instantiations of the fp32 kernel and k_wgrad_f32) runs in bf16 and fp16 (fp32 for its own entries) on two operand kinds:
  dense   err / bound <= 1 for EVERY element of the output and of the forward's statistics, no margin on top; a dense weight
          gradient keeps the norm check of test_gpu_ops.py beside it
  exact   sparse integers whose every partial sum is exact: bit equality with the reference, statistics included
Destinations are prefilled with NaN and followed by a sentinel row that must survive; the switches are set and reset around
every call.  The embedded-1x1 entries (fu_test_op_center_only) are checked against the centre tap's reference, and again under
fu_test_force_full_taps(1) against the same reference with the nine-tap chain length; the one-tap weight gradient's other taps
are exactly 0 through the hook (it clears the slabs the launch does not write).

MEASURED worst err / bound (MI355X) by precision, output and route: conv_ref.MEASURED_GPU (16-bit outputs 0.47 - 0.99, the store
rounding; statistics <= 0.001, weight gradients <= 0.002, fp32 <= 0.06).  Every exact case is bit-equal on every route: no defect
found.  The whole file takes about 20 s.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from tools import conv_ref as R   # noqa: E402

from floodplanet_code_amd import _lib   # noqa: E402
from floodplanet_code_amd._lib import check, ptr   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32, f64 = np.float32, np.float64
CODE = {"fp32": _lib.FU_F32, "bf16": _lib.FU_BF16, "fp16": _lib.FU_F16}
SENTINEL = 1024.0
# precision outermost: the routes that share a shape follow each other, so reference() computes their convolutions once
PARAMS = [(p, c["name"]) for p in ("bf16", "fp16", "fp32") for c in R.TABLE if p in R.precisions(c)]


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(x, dt=torch.float32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).to(dt).to(DEV)


def out_buf(shape, dt=torch.float32):
    """NaN in the shape asked for, followed by one row (the last dimension) of a sentinel"""
    n = int(np.prod(shape))
    t = torch.full((n + shape[-1],), float("nan"), device=DEV, dtype=dt)
    t[n:] = SENTINEL
    return t


def payload(t, shape, what):
    n = int(np.prod(shape))
    assert bool((t[n:].float() == SENTINEL).all()), f"{what}: written past its end"
    return t[:n].float().cpu().numpy().astype(f64).reshape(shape)


def run(prec, c, o, full_taps=0):
    """one call under the case's switches (always reset); {name: float64 array} of what the kernel wrote"""
    lib, dt, code = _lib.load(), R.PREC[prec]["dt"], CODE[prec]
    B, C0, C1, Cout, H, W = c["shape"]
    w = dev(o["w"]) if "w" in o else None
    out = {}
    with R.hooks(lib, c):
        lib.fu_test_force_full_taps(full_taps)
        if c["kind"] == "fwd":
            x0, x1, a, b, bias = dev(o["x0"], dt), dev(o["x1"], dt), dev(o["a"]), dev(o["b"]), dev(o["bias"])
            y, s, q = out_buf((B, H, W, Cout), dt), out_buf((Cout,)), out_buf((Cout,))
            check(lib.fu_op_conv3x3_fwd(code, ptr(x0), C0, ptr(a), ptr(b), ptr(x1), C1, ptr(w), ptr(bias), ptr(y), Cout, B, H, W,
                                        ptr(s), ptr(q), stream()))
            torch.cuda.synchronize()
            out = dict(y=payload(y, (B, H, W, Cout), "y"), sum=payload(s, (Cout,), "sum"), sqsum=payload(q, (Cout,), "sqsum"))
        elif c["kind"] == "dgrad":
            dy = dev(o["dy"], dt)
            dx0, dx1 = out_buf((B, H, W, C0), dt), (out_buf((B, H, W, C1), dt) if C1 else None)
            if c["bnsums"]:
                y, a, b, m, iv = dev(o["y"], dt), dev(o["bn_a"]), dev(o["bn_b"]), dev(o["mean"]), dev(o["invstd"])
                s1, s2 = out_buf((C0,)), out_buf((C0,))
                check(lib.fu_op_conv3x3_dgrad_bnsums(code, ptr(dy), Cout, ptr(w), ptr(dx0), C0, ptr(y), ptr(a), ptr(b), ptr(m),
                                                     ptr(iv), ptr(s1), ptr(s2), B, H, W, stream()))
            else:
                check(lib.fu_op_conv3x3_dgrad(code, ptr(dy), Cout, ptr(w), ptr(dx0), C0, ptr(dx1), C1, B, H, W, stream()))
            torch.cuda.synchronize()
            dx = [payload(dx0, (B, H, W, C0), "dx0")] + ([payload(dx1, (B, H, W, C1), "dx1")] if C1 else [])
            out = dict(dx=np.concatenate(dx, -1))
        else:
            x0, x1, a, b, dy = dev(o["x0"], dt), dev(o["x1"], dt), dev(o["a"]), dev(o["b"]), dev(o["dy"], dt)
            dw = out_buf((Cout, C0 + C1, 3, 3))
            check(lib.fu_op_conv3x3_wgrad(code, ptr(x0), C0, ptr(a), ptr(b), ptr(x1), C1, ptr(dy), Cout, ptr(dw), B, H, W, stream()))
            torch.cuda.synchronize()
            out = dict(dw=payload(dw, (Cout, C0 + C1, 3, 3), "dw"))
    return out


@functools.lru_cache(maxsize=2)
def _convs(prec, opkind, shape, kind, bn, th, center):
    """operands and the float64 convolutions of one shape: (operands, staged input, (ref, sum |a| |b|))"""
    c = dict(shape=shape, kind=kind, bn=bn, th=th, center=center)
    o = R.dense_operands(prec, c) if opkind == "dense" else R.exact_operands(c)
    taps = R.taps_of(c)
    if kind == "dgrad":
        return o, None, R.dgrad_parts(o["dy"], o["w"], taps)
    z = R.staged_input(prec, o)
    return o, z, (R.fwd_parts(z, o["w"], taps) if kind == "fwd" else R.wgrad_parts(z, o["dy"], taps))


def reference(prec, opkind, c, chain_taps=None):
    """(operands, {name: (ref, bound)}) of the case"""
    o, z, parts = _convs(prec, opkind, c["shape"], c["kind"], c["bn"], c["th"], c["center"])
    taps = R.taps_of(c)
    if c["kind"] == "fwd":
        return o, R.fwd_ref(prec, z, o["w"], o["bias"], R.STAT_TILE_PX[c["route"]], taps, parts, chain_taps)
    if c["kind"] == "dgrad":
        return o, {"dx": R.dgrad_ref(prec, o["dy"], o["w"], taps, parts, chain_taps)}
    n, _, _ = R.wgrad_chain(prec, c, _lib.load())
    return o, {"dw": R.wgrad_ref(prec, z, o["dy"], n, taps, parts)}


def fail(c, what, got, ref, bound, r):
    idx = R.worst_element(got, ref, bound)
    where = R.locate(c, idx, got[idx], ref[idx]) if got.ndim == 4 else f"channel {idx[0]} got {got[idx]} ref {ref[idx]}"
    bad = int((np.abs(got - ref) > bound).sum()) + int((~np.isfinite(got)).sum())
    pytest.fail(f"{c['name']} {what}: err / bound {r:.3g}, {bad} of {got.size} elements outside; worst at {where}")


def compare(worst, c, opkind, got, ref, tag=""):
    assert set(got) == set(ref)
    for name, (r_, bound) in ref.items():
        g = got[name]
        if opkind == "exact":            # every partial sum is exact; only a statistic's total may need its one last rounding
            r_ = r_.astype(f32).astype(f64)
            if not np.array_equal(g, r_):
                fail(c, f"exact {name}{tag}", g, r_, np.zeros_like(r_), float("inf"))
            continue
        r = R.worst_ratio(g, r_, bound)
        worst[name + tag] = max(worst.get(name + tag, 0.0), r)
        if not r <= 1.0:
            fail(c, f"dense {name}{tag}", g, r_, bound, r)
        if name == "dw":                     # the norm check of test_gpu_ops.py stays beside the element-wise bound
            assert np.linalg.norm(g - r_) / (np.linalg.norm(r_) + 1e-30) < (1e-5 if c["prec"] == "fp32" else 1e-4)


@pytest.mark.parametrize("prec,name", PARAMS, ids=[f"{p}-{n}" for p, n in PARAMS])
def test_conv_route_parity(prec, name):
    c = R.BY_NAME[name]
    lib = _lib.load()
    with R.hooks(lib, c):
        assert R.route_of(lib, c) == c["route"]
    worst = {}
    for opkind in ("dense", "exact"):
        o, ref = reference(prec, opkind, c)
        if c["kind"] == "wgrad":
            assert R.wgrad_chain(prec, c, lib)[0] <= R.DENSE_WGRAD_MAX_N
        got = run(prec, c, o)
        if c["kind"] == "wgrad" and c["center"]:
            off = R._embed(got["dw"].copy(), 1) != got["dw"]
            assert not off.any(), f"{name}: {int(off.sum())} off-centre entries of a one-tap dw are not 0"
        compare(worst, c, opkind, got, ref)
        if not c["center"]:
            continue
        # the same embedded 1x1 through all nine taps: the same sums over eight taps of exact zeros more
        full = run(prec, c, o, full_taps=1)
        if c["kind"] == "wgrad":             # ... where the weight gradient fills the other eight taps
            c9 = dict(c, center=0)
            z = R.staged_input(prec, o)
            n9 = R.wgrad_chain(prec, c9, lib)[0]
            compare(worst, c, opkind, full, {"dw": R.wgrad_ref(prec, z, o["dy"], n9)}, " full taps")
            if opkind == "exact":
                assert np.array_equal(full["dw"][:, :, 1, 1], got["dw"][:, :, 1, 1])
            continue
        _, ref9 = reference(prec, opkind, c, chain_taps=9)
        compare(worst, c, opkind, full, ref9, " full taps")
        for k in got:                        # against each other: both lie within their bound of one reference
            if opkind == "exact":
                assert np.array_equal(full[k], got[k]), (name, k)
            else:
                assert R.worst_ratio(full[k], got[k], ref[k][1] + ref9[k][1]) <= 1.0, (name, k)
    print(f"MEASURED {prec} {c['kind']} {c['route']} {name}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
