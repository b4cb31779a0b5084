"""GPU: BatchNorm + ReLU backward on its own in fp32, through fu_op_bn_bwd, against fp64 autograd of relu(batch_norm(y))
consumed by a skip gradient and, in the pooled cases, by max_pool2d -- never against the code under test.

  k_bn_bwd_reduce<float> / k_bn_bwd_apply<float>      plain:  (1, 12, 5, 7) and (2, 64, 32, 48)
  k_bn_bwd_pool<float, false / true>                  pooled: (1, 8, 5, 7) and (2, 64, 32, 48)
  k_bn_stats_fused<1>                                 between the two passes of each

(1, 12, 5, 7): C / 4 = 3 does not divide the 256 threads of a block, so thread 255 belongs to no pixel row -- the smallest
shape that reaches the `row < rows` guard of the kernels and of their block epilogue.  (1, 8, 5, 7): an odd edge row and column,
i.e. 2x2 windows without a pool output.  (2, 64, 32, 48): more than one block, several pixels per thread.

INPUTS.  Fixed seed.  fp32 and fp64 must take the same ReLU masks (and the same max-pool winners' masks), or one element's
whole gradient differs and the comparison measures nothing, so the inputs are built with every pre-activation away from zero:
y is drawn, and while some |a*y + b| is below 2e-3 those elements are moved to 4e-3 on their own side of zero (the batch
statistics move by ~1e-6 with them, hence the loop; it ends after one or two rounds).  Seed selection alone cannot do this
at 196,608 elements (about 14 of them fall within 1e-4 of zero for any seed).  The test asserts min |a*y + b| > 1e-4 over the
whole tensor on the host before the GPU call: a condition on the inputs, no element is left out of any comparison.

BOUNDS.  dgamma / dbeta: the project's 1e-4 (tests/test_gpu_benched_dispatch.py).  dL/dy: there was no project number for fp32 at
these shapes, so the relative error (norm of the difference over the norm of the reference) of the library was measured on
these exact inputs on an MI355X, with the build of the commit before this test (whose bits this tree's BatchNorm kernels
reproduce): MEASURED_DY below, 5.0e-8 .. 6.6e-8, about one unit roundoff of float32 (ATen's own float32 backward of the same
graph on the CPU errs by 6.1e-8 .. 6.9e-8 against the same reference).  The bound is 4x the measured figure of each case: a
later change to these kernels is meant to reproduce their bits, so the margin only has to absorb another GPU or driver, and one
wrong mask or one misrouted pool gradient is >= 1e-3 at these sizes.  The test prints each figure before it asserts.

OP-LEVEL PARITY ON EVERY ROUTE (the tests below test_fp32_bn_relu_backward_against_autograd).  Through fu_op_bn_bwd_ex, fu_op_bn_stats
and fu_op_maxpool2, element by element against the fp64 reference and the analytic bounds of tests/tools/bn_ref.py (derived there;
test_bn_ref_cpu.py holds a float32 restatement of the kernels' arithmetic to them) -- never against the code under test.

  k_bn_bwd_reduce / k_bn_bwd_apply<T>            plain shapes x {fused, two-level finalisation}
  k_bn_bwd_pool<T, false / true>                 pooled shapes x {fused, two-level}; fp16 once with unscale = 2^-7
  k_bn_bwd_apply_head<T, 2 / 3 / 0>              C in {8, 16, 64, 128} x ncls in {1, 2, 3, 5, 8} x npix in {1, 35, 4099}, bf16 / fp16
  launch_bn_bwd with external sums               plain shapes x rows in {1, 3, 385, 2048}
  k_bn_stats_fused<0>, k_partials_reduce + k_bn_finalize, bn_fwd_finish      n_part x C grids of bn_ref.STATS_FUSED / STATS_TWO_LEVEL
  k_partials_reduce + k_bn_bwd_finalize          every plain and pooled case again with two_level = 1
  k_maxpool2<T>                                  with and without the prologue, ties, zeros and -0.0

The ReLU mask and every window's argmax are taken from the float32 pre-activation fl(fl(a*y) + b) (bn_act_pre's definition), so
the operands hold exact zeros, windows with two and four equal maxima and all-negative windows.  `dense` operands: a pass is
err / bound <= 1 for EVERY element of dy, dgamma, dbeta, db, coef (mean, invstd, a, b, rmean, rvar), no margin on top.  `exact`
operands (powers of two and small integers, sums made multiples of N): every output equals the reference bit for bit.  Outputs are
prefilled with NaN and followed by a sentinel row that must survive; y, g_pool, dl, w and the partials are bit-identical after
the call.  The forward has no `exact` variant: (var + eps)^-1/2 with eps = 1e-5 is not representable whatever the partials.

MEASURED worst err / bound per output, precision and route (MI355X, this file's cases; a pass is <= 1): bn_ref.MEASURED_GPU, as
the tests print them:
  fp32 plain        coef 0.235  db 0.104  dbeta 0.246  dgamma 0.272  dy 0.420
  fp32 pool         coef 0.161  db 0.069  dbeta 0.157  dgamma 0.161  dy 0.402
  bf16 plain        coef 0.232  db 0.087  dbeta 0.003  dgamma 0.259  dy 0.995
  bf16 pool         coef 0.150  db 0.049  dbeta 0.002  dgamma 0.150  dy 0.995
  fp16 plain        coef 0.308  db 0.092  dbeta 0.003  dgamma 0.253  dy 0.993
  fp16 pool         coef 0.146  db 0.057  dbeta 0.002  dgamma 0.146  dy 0.995
  fp32 ext          coef 0.990  db 0.167  dbeta 0.999  dgamma 1.000  dy 0.860
  bf16 ext          coef 0.997  db 0.148  dbeta 1.000  dgamma 1.000  dy 0.995
  fp16 ext          coef 0.993  db 0.152  dbeta 0.995  dgamma 0.998  dy 0.995
  bf16 head         coef 0.990  db 0.376  dbeta 0.999  dgamma 0.996  dy 0.996
  fp16 head         coef 0.990  db 0.376  dbeta 0.999  dgamma 0.999  dy 1.000
  forward fused     a 0.891  b 0.913  invstd 0.996  mean 0.999  rmean 0.895  rvar 0.877
  forward two_level a 0.784  b 0.722  invstd 0.899  mean 0.956  rmean 0.768  rvar 0.762
(every `exact` case: 0.000, bit-equal.  The float32 restatement measures the same figures to the second digit -- bn_ref.
MEASURED_RESTATEMENT -- i.e. the kernels' error IS their arithmetic's; with external sums dgamma / dbeta / coef are one rounding of an
fp64 value against a bound of one rounding, 1 by construction, and the 16-bit dy sits at the store rounding.)
DEFECTS.  One, on the host: fu_op_bn_bwd with C < 4 ended the process with SIGFPE (bn_bwd_partial_elems divided by C >> 2
before launch_bn_bwd's channel check) and C = 6 reached hipMalloc before being rejected; the hooks now check first
(test_launch_errors_cpu.py).  No defect in the kernels' device code: no ratio above 1 on any route, so fu_bn.hip's
kernels are unchanged and the `bn` and `steps` digests of tools/step_digest.py do not move.  The whole file takes about 6 s.
"""
import pytest
import torch
import torch.nn.functional as F

from floodplanet_code_amd import _lib
from floodplanet_code_amd._lib import check, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BN_EPS = 1e-5

CASES = [((1, 12, 5, 7), False), ((1, 8, 5, 7), True), ((2, 64, 32, 48), False), ((2, 64, 32, 48), True)]
# relative error of dL/dy measured on an MI355X (see BOUNDS above); dgamma / dbeta were 5.7e-8 .. 1.1e-7 in the same run
MEASURED_DY = {((1, 12, 5, 7), False): 6.2340e-08, ((1, 8, 5, 7), True): 6.6166e-08,
               ((2, 64, 32, 48), False): 4.9719e-08, ((2, 64, 32, 48), True): 5.4473e-08}

def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def bn_coefficients(y, gamma, beta):
    yd = y.double()
    mean = yd.mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(yd.var((0, 2, 3), unbiased=False) + BN_EPS)
    a = gamma.double() * invstd
    b = beta.double() - mean * a
    return mean.float(), invstd.float(), a.float(), b.float()


def pre_activation(y, a, b):
    return a.view(1, -1, 1, 1) * y + b.view(1, -1, 1, 1)     # float32, a multiply and an add as bn_act_pre


def make_case(shape, pooled):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(20261018 + C + H)
    y = torch.randn(B, C, H, W, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    for _ in range(8):
        mean, invstd, a, b = bn_coefficients(y, gamma, beta)
        z = pre_activation(y, a, b)
        near = z.abs() < 2e-3
        if not near.any():
            break
        side = torch.where(z >= 0, 1.0, -1.0)
        y = torch.where(near, (side * 4e-3 - b.view(1, -1, 1, 1)) / a.view(1, -1, 1, 1), y)
    mean, invstd, a, b = bn_coefficients(y, gamma, beta)
    g_skip = torch.randn(B, C, H, W, generator=g)
    g_pool = torch.randn(B, C, H // 2, W // 2, generator=g) if pooled else None
    return y, gamma, beta, mean, invstd, a, b, g_skip, g_pool


def to_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


@pytest.mark.parametrize("shape,pooled", CASES)
def test_fp32_bn_relu_backward_against_autograd(shape, pooled):
    lib = _lib.load()
    B, C, H, W = shape
    y, gamma, beta, mean, invstd, a, b, g_skip, g_pool = make_case(shape, pooled)
    zmin = pre_activation(y, a, b).abs().min().item()
    assert zmin > 1e-4, zmin                                  # the input condition: no ReLU mask can differ from fp64's
    if pooled:                                                # ... and no window's first maximum either
        z32 = torch.relu(pre_activation(y, a, b))
        z64 = torch.relu(F.batch_norm(y.double(), None, None, gamma.double(), beta.double(), True, 0.0, BN_EPS))
        assert torch.equal(F.max_pool2d(z32, 2, return_indices=True)[1], F.max_pool2d(z64, 2, return_indices=True)[1])

    y64 = y.double().requires_grad_(True)
    ga64, be64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    out = torch.relu(F.batch_norm(y64, None, None, ga64, be64, True, 0.0, BN_EPS))
    obj = (out * g_skip.double()).sum()
    if pooled:
        obj = obj + (F.max_pool2d(out, 2) * g_pool.double()).sum()
    obj.backward()

    gbuf, dyv = to_nhwc(g_skip), to_nhwc(y)
    dgp = to_nhwc(g_pool) if pooled else None
    dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    da, dbb, dm, di = a.to(DEV), b.to(DEV), mean.to(DEV), invstd.to(DEV)
    check(lib.fu_op_bn_bwd(_lib.FU_F32, ptr(gbuf), ptr(dyv), C, B, H, W, ptr(da), ptr(dbb), ptr(dm), ptr(di), ptr(dgp),
                           ptr(dgamma), ptr(dbeta), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    e_dy = rel(gbuf.permute(0, 3, 1, 2).cpu(), y64.grad)
    e_dg, e_db = rel(dgamma.cpu(), ga64.grad), rel(dbeta.cpu(), be64.grad)
    print(f"bn_bwd fp32 {shape} pooled={pooled}: min|z| {zmin:.3e}  dy {e_dy:.4e}  dgamma {e_dg:.3e}  dbeta {e_db:.3e}")
    assert e_dg <= 1e-4 and e_db <= 1e-4, (e_dg, e_db)
    assert e_dy <= 4 * MEASURED_DY[(shape, pooled)], e_dy     # measured 6.2e-8 / 6.6e-8 / 5.0e-8 / 5.4e-8


# ---- op-level parity on every route (see the second half of the module docstring) -----------------------------------------------
import os            # noqa: E402
import sys           # noqa: E402

import numpy as np   # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))
from tools import bn_ref as R   # noqa: E402

f32 = np.float32
CODE = {"fp32": _lib.FU_F32, "bf16": _lib.FU_BF16, "fp16": _lib.FU_F16}
SENTINEL = 1024.0                     # exact in every element type
PRECS, PRECS16 = list(R.PREC), ["bf16", "fp16"]


def stream():
    return torch.cuda.current_stream().cuda_stream


def out_buf(n, row, dt=torch.float32):
    """n elements of NaN followed by one row of the sentinel"""
    t = torch.full((n + row,), float("nan"), device=DEV, dtype=dt)
    t[n:] = SENTINEL
    return t


def in_buf(x, row, dt=torch.float32):
    """the values of x (flattened) in the element type, followed by one row of the sentinel (never a null pointer)"""
    t = torch.full((x.size + row,), SENTINEL, device=DEV, dtype=dt)
    t[:x.size] = torch.from_numpy(np.ascontiguousarray(x, f32).reshape(-1)).to(dt)
    return t


def intact(t, n):
    return bool((t[n:].float() == SENTINEL).all())


def payload(t, n, shape):
    return t[:n].float().cpu().numpy().reshape(shape)


class Worst(dict):
    def take(self, got, ref, case):
        for name in ref:
            r = R.worst_ratio(got[name], *ref[name])
            self[name] = max(self.get(name, 0.0), r)
            assert r <= 1.0, (case, name, r)

    def report(self, what):
        print(f"MEASURED_GPU {what}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(self.items())))


def run_bwd(prec, route, kw, unscale=None, two_level=0):
    """one fu_op_bn_bwd_ex call on the operands kw of bn_ref.call_args (+ ext) -> {name: float32 array} as bn_ref.bwd_ref"""
    dt = R.PREC[prec]["dt"]
    B, H, W, C_ = kw["y"].shape
    N = B * H * W
    y = in_buf(kw["y"], C_, dt)
    g = out_buf(N * C_, C_, dt) if route == "head" else in_buf(kw["g"], C_, dt)
    coefs = [torch.from_numpy(np.ascontiguousarray(kw[k], f32)).to(DEV) for k in ("a", "b", "mean", "invstd")]
    gp = in_buf(kw["gpool"], C_, dt) if route == "pool" else None
    ext = in_buf(kw["ext"], 2 * C_) if kw.get("ext") is not None else None
    dl = in_buf(kw["dl"], 8) if route == "head" else None
    w = in_buf(kw["w"], C_) if route == "head" else None
    ncls = kw["w"].shape[0] if route == "head" else 0
    us = torch.tensor([unscale], device=DEV, dtype=torch.float32) if unscale is not None else None
    outs = dict(dgamma=out_buf(C_, C_), dbeta=out_buf(C_, C_), db=out_buf(C_, C_), coef=out_buf(2 * C_, C_))
    keep = {k: t.clone() for k, t in dict(y=y, gp=gp, ext=ext, dl=dl, w=w).items() if t is not None}
    check(_lib.load().fu_op_bn_bwd_ex(CODE[prec], ptr(g), ptr(y), C_, B, H, W, *[ptr(t) for t in coefs], ptr(gp),
                                      ptr(outs["dgamma"]), ptr(outs["dbeta"]), ptr(ext), 0 if ext is None else kw["ext"].shape[0],
                                      ptr(dl), ptr(w), ncls, ptr(us), ptr(outs["db"]), ptr(outs["coef"]), two_level, stream()))
    torch.cuda.synchronize()
    case = (prec, route, kw["y"].shape, ncls, two_level)
    for k, t in dict(y=y, gp=gp, ext=ext, dl=dl, w=w).items():
        if t is not None:                       # the operands are bit-identical after the call, their sentinel rows included
            assert torch.equal(t.view(torch.uint8), keep[k].view(torch.uint8)), (case, k)
    assert intact(g, N * C_) and all(intact(t, t.numel() - C_) for t in outs.values()), case
    got = {k: payload(t, t.numel() - C_, (C_, 2) if k == "coef" else (C_,)) for k, t in outs.items()}
    got["dy"] = payload(g, N * C_, (N, C_))
    assert all(np.isfinite(v).all() for v in got.values()), case     # head: g was NaN and comes back without one
    return got


def reference(operands, prec, route, kw, unscale=1.0):
    """bn_ref.bwd_ref; on exact operands the float32 restatement must equal it bit for bit on the host before any GPU call"""
    ref = R.bwd_ref(prec, route, unscale=unscale, **kw)
    if operands == "exact":
        host = R.restate_bwd(prec, route, unscale=unscale, **kw)
        for name in ref:
            assert np.array_equal(host[name].astype(np.float64), ref[name][0]), ("host", prec, route, kw["y"].shape, name)
    return ref


def judge(operands, worst, got, ref, case):
    if operands == "exact":
        for name in ref:
            assert np.array_equal(got[name].astype(np.float64), ref[name][0]), (case, name)
    worst.take(got, ref, case)


def operands_of(operands, prec, route, shape):
    return (R.exact if operands == "exact" else R.dense)(prec, route, shape)


def ext_rows(operands, prec, route, kw, shape, rows):
    if operands == "exact":
        return R.exact_ext(shape[1], shape[0] * shape[2] * shape[3], rows)
    S = R.bwd_ref(prec, route, **kw)
    return R.split_sums(np.stack([S["dbeta"][0], S["dgamma"][0]], 1), rows)


@pytest.mark.parametrize("operands", ["dense", "exact"])
@pytest.mark.parametrize("route", ["plain", "pool"])
@pytest.mark.parametrize("prec", PRECS)
def test_bn_backward_plain_and_pooled_every_element(prec, route, operands):
    worst = Worst()
    for shape in (R.PLAIN_SHAPES if route == "plain" else R.POOL_SHAPES):
        kw = R.call_args(operands_of(operands, prec, route, shape))
        ref = reference(operands, prec, route, kw)
        for two_level in (0, 1):
            judge(operands, worst, run_bwd(prec, route, kw, two_level=two_level), ref, (prec, route, shape, two_level))
    if prec == "fp16" and route == "pool":       # the loss scale leaves the parameters' gradients, never coef or dy
        kw = R.call_args(operands_of(operands, prec, route, (1, 8, 5, 7)))
        ref = reference(operands, prec, route, kw, 2.0 ** -7)
        for two_level in (0, 1):
            judge(operands, worst, run_bwd(prec, route, kw, unscale=2.0 ** -7, two_level=two_level), ref, (prec, route, "unscale"))
    worst.report(f"{prec} {route} {operands}")


@pytest.mark.parametrize("operands", ["dense", "exact"])
@pytest.mark.parametrize("prec", PRECS)
def test_bn_backward_with_external_sums_every_element(prec, operands):
    worst = Worst()
    for shape in R.PLAIN_SHAPES:
        ops = operands_of(operands, prec, "plain", shape)
        for rows in R.EXT_ROWS:
            kw = R.call_args(ops)
            kw["ext"] = ext_rows(operands, prec, "plain", R.call_args(ops), shape, rows)
            ref = reference(operands, prec, "plain", kw)
            for two_level in ((0, 1) if rows in (3, 385) else (0,)):
                judge(operands, worst, run_bwd(prec, "plain", kw, two_level=two_level), ref, (prec, "ext", shape, rows, two_level))
    worst.report(f"{prec} ext {operands}")


@pytest.mark.parametrize("operands", ["dense", "exact"])
@pytest.mark.parametrize("prec", PRECS16)
def test_bn_backward_with_the_head_gradient_recomputed_every_element(prec, operands):
    worst = Worst()
    for C_ in R.HEAD_WIDTHS:
        for npix in R.HEAD_NPIX:
            shape = (1, C_, 1, npix)
            ops = operands_of(operands, prec, "head", shape)
            for ncls in R.HEAD_CLASSES:
                kw = R.call_args(ops, ncls)
                kw["ext"] = ext_rows(operands, prec, "head", R.call_args(ops, ncls), shape, 3)
                us = 2.0 ** -7 if (prec, C_, ncls, npix) == ("fp16", 64, 3, 4099) else None
                ref = reference(operands, prec, "head", kw, us or 1.0)
                judge(operands, worst, run_bwd(prec, "head", kw, unscale=us), ref, (prec, "head", C_, npix, ncls))
    worst.report(f"{prec} head {operands}")


# ---- forward finalisation --------------------------------------------------------------------------------------------------------
def run_stats(ops, bias=True, running=True, calls=1):
    """fu_op_bn_stats `calls` times on the partials of bn_ref.make_partials; -> the outputs of every call, nbt before / after"""
    part = ops["partials"]
    n_part, C_ = part.shape[:2]
    dpart = in_buf(part, 2 * C_)
    keep = dpart.clone()
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, f32)).to(DEV)     # noqa: E731
    cb, gam, bet = (dev(ops["conv_bias"]) if bias else None), dev(ops["gamma"]), dev(ops["beta"])
    rm, rv = (in_buf(ops["rmean"], C_), in_buf(ops["rvar"], C_)) if running else (None, None)
    nbt = torch.tensor([5, 777], device=DEV, dtype=torch.int64) if running else None
    results = []
    for _ in range(calls):
        outs = {k: out_buf(C_, C_) for k in ("mean", "invstd", "a", "b")}
        check(_lib.load().fu_op_bn_stats(ptr(dpart), n_part, C_, ops["count"], ptr(cb), ptr(gam), ptr(bet), ops["eps"],
                                         ops["momentum"], ptr(outs["mean"]), ptr(outs["invstd"]), ptr(outs["a"]), ptr(outs["b"]),
                                         ptr(rm), ptr(rv), ptr(nbt), stream()))
        torch.cuda.synchronize()
        assert all(intact(t, C_) for t in outs.values()) and torch.equal(dpart.view(torch.int32), keep.view(torch.int32))
        got = {k: payload(t, C_, (C_,)) for k, t in outs.items()}
        if running:
            assert intact(rm, C_) and intact(rv, C_)
            got["rmean"], got["rvar"] = payload(rm, C_, (C_,)), payload(rv, C_, (C_,))
        results.append(got)
    return results, (None if nbt is None else nbt.cpu().tolist())


def check_stats(worst, ops, case):
    args = {k: ops[k] for k in ("partials", "count", "gamma", "beta", "eps", "momentum")}
    (first, second), nbt = run_stats(ops, calls=2)
    assert nbt == [7, 777], (case, nbt)                      # + 1 per call, whatever C is; the neighbour survives
    worst.take(first, R.stats_ref(conv_bias=ops["conv_bias"], rmean=ops["rmean"], rvar=ops["rvar"], **args), case)
    worst.take(second, R.stats_ref(conv_bias=ops["conv_bias"], rmean=first["rmean"], rvar=first["rvar"], **args), case + (2,))
    (bare,), _ = run_stats(ops, bias=False, running=False)
    worst.take(bare, R.stats_ref(conv_bias=None, **args), case + ("bare",))


@pytest.mark.parametrize("form", ["fused", "two_level"])
def test_bn_forward_finalisation_every_channel(form):
    """fused: C % 4 == 0, k_bn_stats_fused<0> (385 partials: the first count that enters its four-loads-in-flight loop);
    two_level: any other C, k_partials_reduce + k_bn_finalize (32 groups: 31 / 32 / 33 partials straddle the boundary).
    Channel 0 is constant (the variance clamp), the last channel has |mean| / std = 1e3; count = 1 is a case of its own."""
    worst = Worst()
    grid = R.STATS_FUSED if form == "fused" else R.STATS_TWO_LEVEL
    for C_ in grid["C"]:
        for n_part in grid["n_part"]:
            check_stats(worst, R.make_partials(n_part, C_), (form, n_part, C_))
        check_stats(worst, R.make_partials_count1(C_), (form, "count1", C_))
    worst.report(f"forward {form}")


# ---- 2x2 max-pool ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bn", [True, False], ids=["bnrelu", "plain"])
@pytest.mark.parametrize("prec", PRECS)
def test_maxpool_selects_value_for_value(prec, bn):
    dt, V = R.PREC[prec]["dt"], R.PREC[prec]["vec"]
    for shape in R.POOL2_SHAPES:
        B, C_, H, W = (1, V, 2, 2) if shape == "V" else shape
        rng = np.random.default_rng(11 + C_ + H * W)
        x = rng.standard_normal((B, H, W, C_)).astype(f32)
        xw = R.to_windows(x)
        wi = np.arange(xw.shape[0] * xw.shape[1] * xw.shape[2]).reshape(xw.shape[:3])
        xw[wi % 4 == 1] = xw[wi % 4 == 1][:, :1]              # four equal values
        xw[wi % 4 == 2, 1:3] = 0.0                            # zeros in the window ...
        xw[wi % 4 == 2, 3] = -0.0                             # ... and a negative zero
        xw[wi % 4 == 3, :, 0] = -np.abs(xw[wi % 4 == 3, :, 0])    # channel 0 all negative
        x = R.round_to(R.from_windows(xw, H, W), dt)
        a = (rng.random(C_) + 0.5).astype(f32) * np.where(np.arange(C_) % 3 == 2, -1, 1).astype(f32)
        b = (rng.standard_normal(C_) * 0.3).astype(f32)
        ref = R.maxpool_ref(prec, x, a if bn else None, b if bn else None)
        n = ref.size
        src, dst = in_buf(x, C_, dt), out_buf(n, C_, dt)
        keep = src.clone()
        da, db = (torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)) if bn else (None, None)
        check(_lib.load().fu_op_maxpool2(CODE[prec], ptr(src), ptr(da), ptr(db), ptr(dst), B, H, W, C_, stream()))
        torch.cuda.synchronize()
        assert intact(dst, n) and torch.equal(src.view(torch.uint8), keep.view(torch.uint8)), (prec, shape)
        got = payload(dst, n, ref.shape)
        assert np.array_equal(got, ref), (prec, shape, bn, int((got != ref).sum()))     # -0.0 == 0.0 counts as equal
