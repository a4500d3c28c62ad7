"""Fused BatchNorm + add + ReLU (csrc/bn_act.hip) against torch's own ops on the same inputs.

Reference: F.batch_norm(training=True) -> + residual -> relu, evaluated in fp64 (CPU) from the
same (bf16-rounded, for the bf16 path) inputs; autograd of that expression for the grads.
Tolerances: fp32 path 2e-5 relative to the tensor's scale (one-pass shifted statistics vs
torch's Welford); bf16 path: outputs are bf16, so |got - ref| <= 1/128 of the scale plus
one bf16 ulp of the value (the reference is rounded once more by the cast).
Running statistics: 1e-5 relative (fp32 path) / 1e-3 (bf16 inputs, same statistics).
"""
from __future__ import annotations

import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from bn_cases import FAR_MEAN_CASES, MAIN_CASES, OPTION_CASE, SHAPES, launch_plan

pytestmark = pytest.mark.gpu


def _ref(x, bn, relu, res):
    """torch reference in fp64 on the CPU from the same inputs (copies of bn's buffers are updated).
    (fp64: torch's GPU fp32 batch_norm itself loses digits to E[x^2] - E[x]^2 on tiny M.)"""
    xr = x.detach().cpu().double().requires_grad_(True)
    w = bn.weight.detach().cpu().double().requires_grad_(True)
    b = bn.bias.detach().cpu().double().requires_grad_(True)
    rr = res.detach().cpu().double().requires_grad_(True) if res is not None else None
    rm, rv = bn.running_mean.cpu().double(), bn.running_var.cpu().double()
    y = F.batch_norm(xr, rm, rv, w, b, training=True, momentum=bn.momentum, eps=bn.eps)
    if rr is not None:
        y = y + rr
    if relu:
        y = F.relu(y)
    return y, xr, w, b, rr, rm, rv


def _close(got, ref, tol, scale=None):
    bf16 = got.dtype == torch.bfloat16
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    scale = ref.abs().max().clamp_min(1e-12) if scale is None else max(float(scale), float(ref.abs().max()))
    err = (got - ref).abs()
    ok = err <= tol * scale + ref.abs() * (2 ** -8 if bf16 else 0)
    return bool(ok.all()), float(err.max() / scale)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ["relu", "res_relu", "plain"])
def test_bn_act_matches_torch(dev, dtype, shape, mode):
    torch.manual_seed(hash((shape, mode)) & 0xFFFF)
    x = (torch.randn(shape, device=dev) * 1.7 + 0.3).to(dtype).contiguous(memory_format=torch.channels_last)
    res = (torch.randn(shape, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
           if mode == "res_relu" else None)
    _check_fwd_bwd(dev, x, res, mode != "plain")


def _check_fwd_bwd(dev, x, res, relu, stored_mask=False):
    """One forward and one backward of bn_act on x (channels-last) against _ref: y, the running
    statistics, num_batches_tracked, dx, dgamma, dbeta within the file's tolerances, dres bit-exact.
    Returns the measured errors (relative to each tensor's scale).

    stored_mask (the multi-million element cases): the reference's ReLU gradient uses y > 0 of the
    stored y, the backward's definition. Among 10^7 elements a few pre-activations lie within the
    kernel's fp32 rounding of zero, where the fp64 reference's own sign is no better founded; one
    such element would put a whole |dy| into dx and dres. The two masks may differ only where the
    reference is within the forward tolerance of zero, which is asserted; y itself is still compared
    with the reference's relu."""
    from distributedauc_amd.fused_bn import bn_act, supported

    dtype, shape, C = x.dtype, tuple(x.shape), x.shape[1]
    errs = {}
    bn = nn.BatchNorm2d(C).to(dev).train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.1, 0.1)
        bn.running_var.uniform_(0.9, 1.1)
    assert supported(x)
    stored_mask = stored_mask and relu
    yref, xr, w, b, rr, rm, rv = _ref(x, bn, relu and not stored_mask, res)
    if stored_mask:
        pre, yref = yref, F.relu(yref.detach())
    xg = x.detach().clone().requires_grad_(True)
    rg = res.detach().clone().requires_grad_(True) if res is not None else None
    y = bn_act(xg, bn, relu, rg)
    assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
    tol = 2e-5 if dtype == torch.float32 else 2 ** -7
    ok, errs["y"] = _close(y, yref, tol)
    assert ok, ("forward", errs)
    rs_tol = 1e-5 if dtype == torch.float32 else 1e-3
    for got, ref, name in ((bn.running_mean, rm, "running_mean"), (bn.running_var, rv, "running_var")):
        got = got.cpu().double()
        errs[name] = float(((got - ref).abs() / (1 + ref.abs())).max())  # in units of atol + rtol |ref|
        assert torch.allclose(got, ref, rtol=rs_tol, atol=rs_tol), (name, errs)
    assert int(bn.num_batches_tracked) == 1

    dy = torch.randn(shape, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
    if stored_mask:
        keep = (y.detach() > 0).cpu()
        flips = keep != (pre.detach() > 0)
        errs["mask_flips"] = int(flips.sum())
        assert bool((pre.detach().abs()[flips] <= tol * yref.abs().max()).all()), ("mask", errs)
        yref = pre * keep
    yref.backward(dy.cpu().double())
    y.backward(dy)
    # dx = gamma*invstd*(g - mean g - xhat mean(g xhat)) cancels when M is tiny: its error is
    # relative to the scale of the terms, gamma*invstd*|g|
    xd = x.detach().cpu().double()
    invstd = 1.0 / torch.sqrt(xd.var(dim=(0, 2, 3), unbiased=False) + bn.eps)
    term = float((w.detach().abs() * invstd).max() * dy.detach().cpu().double().abs().max())
    for got, ref, name in ((xg.grad, xr.grad, "dx"), (bn.weight.grad, w.grad, "dgamma"),
                           (bn.bias.grad, b.grad, "dbeta")):
        ok, errs[name] = _close(got, ref, tol if name == "dx" else 1e-4, term if name == "dx" else None)
        assert ok, (name, errs)
    if rg is not None:
        ok, errs["dres"] = _close(rg.grad, rr.grad, 0)
        assert ok, ("dres", errs)
    return errs


def test_bn_act_deterministic(dev):
    from distributedauc_amd.fused_bn import bn_act

    x = torch.randn(16, 256, 28, 28, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    outs = []
    for _ in range(2):
        bn = nn.BatchNorm2d(256).to(dev).train()
        xg = x.clone().requires_grad_(True)
        y = bn_act(xg, bn, True, None)
        y.backward(torch.ones_like(y))
        outs.append((y, xg.grad, bn.weight.grad, bn.running_var.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_bn_act_rejects_unsupported(dev):
    from distributedauc_amd.fused_bn import bn_act, supported

    bn = nn.BatchNorm2d(96).to(dev).train()
    x = torch.randn(2, 96, 4, 4, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert not supported(x)
    with pytest.raises(ValueError):
        bn_act(x, bn)
    bn64 = nn.BatchNorm2d(64).to(dev).train()
    x_nchw = torch.randn(2, 64, 4, 4, device=dev)
    assert not supported(x_nchw)
    with pytest.raises(ValueError):
        bn_act(x_nchw, bn64)


def test_resnet_fused_matches_unfused(dev):
    """A ResNet-50 training step (channels-last) three ways: fp32 torch (the reference), bf16
    autocast with torch's BN/add/relu, bf16 autocast with the fused kernels. Summed over 3 seeds
    (tests/bf16_step_compare.py), the fused run must be as close to the fp32 reference as torch's
    own bf16 run is: logits max error <= 2x torch's + 1e-3; every parameter gradient's L2 error
    <= 2x torch bf16's + 1e-3 of its norm; every BN running statistic's max error likewise."""
    from bf16_step_compare import compare

    compare(dev, fused_bn=True, gemm_1x1=False, check_buffers=True)


def test_resnet_fused_counts_batches_once(dev):
    """Fused training forwards bump every BN's num_batches_tracked once (one multi-tensor launch)."""
    from distributedauc_amd.backbone import resnet18

    net = resnet18().to(dev).to(memory_format=torch.channels_last).set_fused_bn(True).train()
    x = torch.randn(4, 3, 32, 32, device=dev).contiguous(memory_format=torch.channels_last)
    net(x)
    net(x)
    counts = {n: int(b) for n, b in net.named_buffers() if n.endswith("num_batches_tracked")}
    assert counts and set(counts.values()) == {2}, counts
    net.eval()
    net(x)
    assert {int(b) for n, b in net.named_buffers() if n.endswith("num_batches_tracked")} == {2}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("residual", [False, True])
def test_bn_relu_mask_matches_y_path(dev, dtype, residual):
    """Round 5: the forward's 1-bit ReLU mask (one byte per 16-byte vector) is exactly `y > 0` on the
    stored y -- zeros, negative zeros, values whose bf16 rounding lands on a denormal or on zero,
    +inf and NaN included -- and the backward that reads it gives dx, dres, dgamma and dbeta bit for
    bit as the backward that reads y (the layout: element i of vector v is bit i of mask byte v)."""
    from distributedauc_amd import _lib
    from distributedauc_amd.fused_bn import _DTYPES
    from distributedauc_amd.ops import _ptr, _stream, check, workspaces

    g = torch.Generator(device=dev).manual_seed(21)
    N, C, H, W = 4, 64, 6, 5
    x = torch.randn(N, C, H, W, device=dev, generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
    flat = x.permute(0, 2, 3, 1).reshape(-1)  # channels-last order
    flat[::97] = 0.0
    flat[5::211] = float("nan")
    flat[7::223] = float("inf")
    res = torch.randn(N, C, H, W, device=dev, generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
    # shift/scale so that many outputs sit just above / below zero, some in the denormal range
    gamma = torch.full((C,), 1e-38, device=dev)
    gamma[: C // 2] = 1.0
    beta = torch.zeros(C, device=dev)
    M = N * H * W
    L = _lib.load()
    ws = workspaces.get(dev, "bn_mask_test", L.dauc_bn_workspace_size(M, C))
    y = torch.empty_like(x)
    mask = torch.full((M * C * x.element_size() // 16,), 0xAA, dtype=torch.uint8, device=dev)
    mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    rp = res if residual else None
    check(L.dauc_bn_act_forward(_ptr(x), _DTYPES[dtype], M, C, _ptr(rp), 1, _ptr(gamma), _ptr(beta), None, None,
                                0.1, 1e-5, _ptr(y), _ptr(mask), _ptr(mean), _ptr(invstd), _ptr(ws), ws.numel(),
                                _stream(dev)), "forward")
    yv = y.permute(0, 2, 3, 1).reshape(-1).float()
    vec = 16 // x.element_size()
    bits = (yv > 0).view(-1, vec).to(torch.int32)
    want = (bits << torch.arange(vec, device=dev, dtype=torch.int32)).sum(1).to(torch.uint8)
    assert torch.equal(mask, want)
    assert bool((yv > 0).any()) and bool((yv == 0).any())
    dy = torch.randn(N, C, H, W, device=dev, generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
    outs = []
    for use_mask in (False, True):
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if residual else None
        dgamma, dbeta = torch.empty(C, device=dev), torch.empty(C, device=dev)
        check(L.dauc_bn_act_backward(_ptr(dy), None if use_mask else _ptr(y), _ptr(mask) if use_mask else None,
                                     _ptr(x), _DTYPES[dtype], M, C, 1, _ptr(gamma), _ptr(mean), _ptr(invstd),
                                     _ptr(dres), _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel(),
                                     _stream(dev)), "backward")
        outs.append([t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).clone()
                     for t in (dx, dgamma, dbeta) + ((dres,) if residual else ())])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- the kernels' main loops (bn_cases.py; tests/test_bn_plan_host.py holds the shapes to them) ----

_TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16}
_EPS = 1e-5


def _case_id(case):
    return f"{case[0]}x{case[1]}-{case[2]}-{case[3]}"


def _nchw(t):
    """[M, C] row-major -> the (1, C, M, 1) channels-last view of the same memory."""
    M, C = t.shape
    return t.view(1, M, 1, C).permute(0, 3, 1, 2)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _dirty(*shape, dev, dtype=torch.float32):
    """An output the kernel has to overwrite: NaN (floats) or 0xAA (bytes) everywhere."""
    if dtype == torch.uint8:
        return torch.full(shape, 0xAA, dtype=dtype, device=dev)
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _dirty_ws(dev, M, C):
    """A workspace of the size the library asks for, every float of it NaN: a partial row or a
    coefficient that a launch reads without having written it poisons the result."""
    from distributedauc_amd import _lib

    ws = torch.empty(_lib.load().dauc_bn_workspace_size(M, C), dtype=torch.uint8, device=dev)
    ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    return ws


def _direct_forward(dev, x, gamma, beta, relu, res=None, want_mask=False):
    """dauc_bn_act_forward on x [M, C] with a dirty workspace and dirty outputs."""
    from distributedauc_amd import _lib
    from distributedauc_amd.fused_bn import _DTYPES
    from distributedauc_amd.ops import _ptr, _stream, check

    M, C = x.shape
    ws = _dirty_ws(dev, M, C)
    y = _dirty(M, C, dev=dev, dtype=x.dtype)
    mask = _dirty(M * C * x.element_size() // 16, dev=dev, dtype=torch.uint8) if want_mask else None
    mean, invstd = _dirty(C, dev=dev), _dirty(C, dev=dev)
    check(_lib.load().dauc_bn_act_forward(_ptr(x), _DTYPES[x.dtype], M, C, _ptr(res), int(relu), _ptr(gamma),
                                          _ptr(beta), None, None, 0.1, _EPS, _ptr(y), _ptr(mask), _ptr(mean),
                                          _ptr(invstd), _ptr(ws), ws.numel(), _stream(dev)), "forward")
    return y, mask, mean, invstd


def _direct_backward(dev, dy, y, mask, x, relu, gamma, mean, invstd):
    """dauc_bn_act_backward (reading y or the mask) with a dirty workspace and dirty outputs."""
    from distributedauc_amd import _lib
    from distributedauc_amd.fused_bn import _DTYPES
    from distributedauc_amd.ops import _ptr, _stream, check

    M, C = x.shape
    ws = _dirty_ws(dev, M, C)
    dx = _dirty(M, C, dev=dev, dtype=x.dtype)
    dgamma, dbeta = _dirty(C, dev=dev), _dirty(C, dev=dev)
    check(_lib.load().dauc_bn_act_backward(_ptr(dy), _ptr(y), _ptr(mask), _ptr(x), _DTYPES[x.dtype], M, C, int(relu),
                                           _ptr(gamma), _ptr(mean), _ptr(invstd), None, _ptr(dx), _ptr(dgamma),
                                           _ptr(dbeta), _ptr(ws), ws.numel(), _stream(dev)), "backward")
    return dx, dgamma, dbeta


def _stat_ratios(x, mean, invstd):
    """save_mean / save_invstd against fp64 statistics of the same x [M, C] (CPU), as multiples of the
    fp32 bar: |mean - ref| / (2e-5 std_ref + 2^-23 |mean_ref|) and |invstd / ref - 1| / 2e-5."""
    xd = x.detach().cpu().double()
    mref, vref = xd.mean(0), xd.var(0, unbiased=False)
    iref = 1.0 / torch.sqrt(vref + _EPS)
    rm = (mean.cpu().double() - mref).abs() / (2e-5 * vref.sqrt() + 2.0 ** -23 * mref.abs())
    ri = (invstd.cpu().double() / iref - 1.0).abs() / 2e-5
    return float(rm.max()), float(ri.max())


def _randn(M, C, dev, g, dtype, scale=1.0, shift=0.0):
    return (torch.randn(M, C, device=dev, generator=g) * scale + shift).to(dtype)


@pytest.mark.parametrize("case", list(MAIN_CASES), ids=_case_id)
def test_bn_main_loops_match_fp64(dev, case):
    """One forward and one backward at the smallest shapes whose row blocks run the partial-sum
    kernel's grouped main loops and its tail, a short last block, the finalize's grouped loop and a
    partly filled last elementwise workgroup (bn_cases.MAIN_CASES), against the fp64 reference: the
    assertions and tolerances of test_bn_act_matches_torch, unchanged (per-thread fp32 sums cover
    rows / RPB <= 19 terms, fp64 from there: the tiny shapes' bounds hold).
    Measured (relative to each tensor's scale; bounds 2e-5 | 2^-7 for y and dx, 1e-4 for dgamma
    and dbeta, 1e-5 | 1e-3 for the running statistics):
      147533 x 64 bf16 relu      y 2.3e-3  dx 3.1e-3  dgamma 2.2e-7  dbeta 2.1e-8  running 3.4e-9, 3.0e-8
      4603 x 2048 bf16 res_relu  y 3.5e-3  dx 2.5e-3  dgamma 7.9e-8  dbeta 4.0e-8  running 3.9e-9, 3.2e-8
      2301 x 2048 fp32 plain     y 1.0e-7  dx 1.1e-7  dgamma 1.1e-7  dbeta 5.9e-8  running 5.5e-9, 3.4e-8
      36869 x 256 fp32 res_relu  y 1.1e-7  dx 1.1e-7  dgamma 7.8e-8  dbeta 1.1e-7  running 3.9e-9, 3.0e-8
      86393 x 128 bf16 plain     y 2.3e-3  dx 1.7e-3  dgamma 1.2e-7  dbeta 2.8e-8  running 4.0e-9, 3.2e-8
    dres exact; no element's ReLU mask differed from the reference's (stored_mask, _check_fwd_bwd)."""
    M, C, dname, mode = case
    dtype = _TORCH[dname]
    torch.manual_seed(M % 65521 + C)
    g = torch.Generator(device=dev).manual_seed(M + C)
    x = _nchw(_randn(M, C, dev, g, dtype, 1.7, 0.3))
    res = _nchw(_randn(M, C, dev, g, dtype)) if mode == "res_relu" else None
    errs = _check_fwd_bwd(dev, x, res, mode != "plain", stored_mask=True)
    print("measured", _case_id(case), {k: (v if isinstance(v, int) else f"{v:.3g}") for k, v in errs.items()})


def test_bn_relu_mask_main_loops(dev):
    """The ReLU mask at 147533 x 64 bf16, where the backward's main loop reads mask bytes of several
    passes per group: the mask bytes are y > 0 of the stored y, and the backward that reads the mask
    gives dx, dgamma and dbeta bit for bit as the one that reads y. Workspace and outputs start dirty."""
    (M, C, dname, _), = [c for c in MAIN_CASES if c[3] == "relu"]
    dtype = _TORCH[dname]
    g = torch.Generator(device=dev).manual_seed(5)
    x = _randn(M, C, dev, g, dtype, 1.7, 0.3)
    gamma = torch.rand(C, device=dev, generator=g) + 0.5
    beta = torch.rand(C, device=dev, generator=g) - 0.5
    y, mask, mean, invstd = _direct_forward(dev, x, gamma, beta, True, want_mask=True)
    vec = 16 // x.element_size()
    bits = (y.float() > 0).view(-1, vec).to(torch.int32)
    want = (bits << torch.arange(vec, device=dev, dtype=torch.int32)).sum(1).to(torch.uint8)
    assert torch.equal(mask, want)
    assert 0.3 < float((y.float() > 0).float().mean()) < 0.7
    dy = _randn(M, C, dev, g, dtype)
    by_y = _direct_backward(dev, dy, y, None, x, True, gamma, mean, invstd)
    by_mask = _direct_backward(dev, dy, None, mask, x, True, gamma, mean, invstd)
    for a, b in zip(by_y, by_mask):
        assert not bool(torch.isnan(a).any())
        assert torch.equal(_bits(a), _bits(b))


_STAT_CASES = [(c[0], c[1], c[2]) for c in MAIN_CASES] + [
    (N * H * W, C, d) for (N, C, H, W) in (SHAPES[0], SHAPES[2]) for d in ("fp32", "bf16")]


@pytest.mark.parametrize("case", _STAT_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_bn_saved_statistics_match_fp64(dev, case):
    """save_mean and save_invstd of the C entry point (dirty workspace and outputs) against fp64
    statistics of the same inputs, at the main-loop shapes and two tiny ones. The bar is the fp32
    one for bf16 inputs too -- the statistics are fp32 outputs of fp64 folds and never pass through
    bf16: |mean - ref| <= 2e-5 std_ref + 2^-23 |mean_ref|, |invstd / ref - 1| <= 2e-5.
    Measured, as multiples of the bar (mean, invstd):
      147533 x 64 bf16  7.0e-4, 3.3e-3    4603 x 2048 bf16  4.6e-4, 3.5e-3    2301 x 2048 fp32  1.0e-3, 3.5e-3
      36869 x 256 fp32  8.0e-4, 3.1e-3    86393 x 128 bf16  5.7e-4, 3.3e-3
      252 x 64 fp32     3.1e-3, 9.6e-3    252 x 64 bf16     2.3e-3, 1.3e-2
      27 x 2048 fp32    1.8e-3, 3.6e-3    27 x 2048 bf16    2.0e-3, 3.0e-3"""
    M, C, dname = case
    g = torch.Generator(device=dev).manual_seed(M * 3 + C)
    x = _randn(M, C, dev, g, _TORCH[dname], 1.7, 0.3)
    _, _, mean, invstd = _direct_forward(dev, x, None, None, False)
    rm, ri = _stat_ratios(x, mean, invstd)
    print("measured", case, f"mean {rm:.3g} invstd {ri:.3g}")
    assert rm <= 1.0 and ri <= 1.0, (rm, ri)


@pytest.mark.parametrize("case", list(FAR_MEAN_CASES), ids=_case_id)
def test_bn_mean_far_from_zero(dev, case):
    """|mean| >> std, the case the shifted one-pass sums (k = each block's first row) exist for:
    x ~ 300 + 0.05 randn in fp32 (mean / std = 6000), 8 + 0.25 randn rounded to bf16, 147296 x 64 (the
    main loops run; 256 blocks, each with its own k). Statistics: the bar of
    test_bn_saved_statistics_match_fp64. y: the file's tolerance plus what fp32 cannot avoid,
    2^-24 |mean| |gamma| invstd per channel (save_mean and x - mean are fp32, as in torch). dx: the
    file's tolerance.
    Measured, as multiples of the bars (dx relative to its scale, bound 2e-5 | 2^-7):
      fp32  mean 0.41 (the fp32 rounding of save_mean itself)  invstd 6.0e-3  y 0.61  dx 7.7e-7
      bf16  mean 0.073  invstd 2.9e-3  y 0.21  dx 1.9e-3"""
    from distributedauc_amd.fused_bn import bn_act

    M, C, dname, _ = case
    dtype = _TORCH[dname]
    torch.manual_seed(C)
    g = torch.Generator(device=dev).manual_seed(M)
    x2 = _randn(M, C, dev, g, dtype, 0.05, 300.0) if dtype == torch.float32 else _randn(M, C, dev, g, dtype, 0.25, 8.0)
    _, _, mean, invstd = _direct_forward(dev, x2, None, None, False)
    rm, ri = _stat_ratios(x2, mean, invstd)
    assert rm <= 1.0 and ri <= 1.0, (rm, ri)

    x = _nchw(x2)
    bn = nn.BatchNorm2d(C).to(dev).train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    yref, xr, w, b, _, _, _ = _ref(x, bn, False, None)
    xg = x.detach().clone().requires_grad_(True)
    y = bn_act(xg, bn, False, None)
    tol = 2e-5 if dtype == torch.float32 else 2 ** -7
    xd = x2.cpu().double()
    mref, iref = xd.mean(0), 1.0 / torch.sqrt(xd.var(0, unbiased=False) + bn.eps)
    extra = (2.0 ** -24 * mref.abs() * w.detach().abs() * iref).view(1, C, 1, 1)
    yd, yr = y.detach().cpu().double(), yref.detach()
    bound = tol * yr.abs().max() + yr.abs() * (2 ** -8 if dtype == torch.bfloat16 else 0) + extra
    ey = float(((yd - yr).abs() / bound).max())
    dy = _nchw(_randn(M, C, dev, g, dtype))
    yref.backward(dy.cpu().double())
    y.backward(dy)
    term = float((w.detach().abs() * iref).max() * dy.cpu().double().abs().max())
    ok, edx = _close(xg.grad, xr.grad, tol, term)
    print("measured", _case_id(case), f"mean {rm:.3g} invstd {ri:.3g} y/bound {ey:.3g} dx {edx:.3g}")
    assert ey <= 1.0, ("y", ey)
    assert ok, ("dx", edx)


@pytest.mark.parametrize("case", [c for c in MAIN_CASES if c[:3] in ((147533, 64, "bf16"), (2301, 2048, "fp32"))],
                         ids=_case_id)
def test_bn_channels_are_isolated(dev, case):
    """NaN, +inf and -inf written into two channels, at rows inside the main-loop range (forward and
    backward) of a middle row block, change nothing in any other channel: y, save_mean, save_invstd,
    dx, dgamma and dbeta of every other channel are bit-identical to the clean run's (a thread's
    other channels of the same 16-byte vector, the LDS reduction and the finalize included)."""
    M, C, dname, mode = case
    dtype = _TORCH[dname]
    relu = mode != "plain"
    p = launch_plan(M, C, dname)
    rs, RPB = (p["nrb"] // 2) * p["rows"], p["RPB"]
    assert 4 * RPB <= min(p["fwd_group_rows"], p["bwd_group_rows"]) <= p["rows"]
    g = torch.Generator(device=dev).manual_seed(11)
    x = _randn(M, C, dev, g, dtype, 1.7, 0.3)
    bad = x.clone()
    poisoned = [5, C - 2]
    for c in poisoned:  # passes 1, 2 and 3 of the block: inside the first group of both main loops
        bad[rs + RPB + 1, c] = float("nan")
        bad[rs + 2 * RPB, c] = float("inf")
        bad[rs + 3 * RPB + RPB - 1, c] = float("-inf")
    gamma = torch.rand(C, device=dev, generator=g) + 0.5
    beta = torch.rand(C, device=dev, generator=g) - 0.5
    dy = _randn(M, C, dev, g, dtype)
    keep = torch.ones(C, dtype=torch.bool, device=dev)
    keep[poisoned] = False
    outs = []
    for xin in (x, bad):
        y, mask, mean, invstd = _direct_forward(dev, xin, gamma, beta, relu, want_mask=relu)
        dx, dgamma, dbeta = _direct_backward(dev, dy, None, mask, xin, relu, gamma, mean, invstd)
        outs.append([_bits(t)[..., keep] for t in (y, mean, invstd, dx, dgamma, dbeta)])
        assert not any(bool(torch.isnan(t[..., keep]).any()) for t in (y, mean, invstd, dx, dgamma, dbeta))
    assert bool(torch.isnan(mean[poisoned]).all())  # the poison did reach the statistics of its channels
    for name, a, b in zip(("y", "save_mean", "save_invstd", "dx", "dgamma", "dbeta"), *outs):
        assert torch.equal(a, b), name


_OPTIONS = {"no_affine": dict(affine=False), "no_running_stats": dict(track_running_stats=False),
            "cumulative_average": dict(momentum=None)}


@pytest.mark.parametrize("shape", [SHAPES[0]] + [(1, c[1], c[0], 1) for c in OPTION_CASE], ids=["tiny", "main_loops"])
@pytest.mark.parametrize("option", list(_OPTIONS))
def test_bn_act_module_options(dev, option, shape):
    """affine=False (gamma, beta, dgamma, dbeta absent), track_running_stats=False (no running
    statistics) and momentum=None (the cumulative average: two consecutive forwards, factors 1/1
    then 1/2), each against the same nn.BatchNorm2d in fp64 on the CPU, at a tiny and a main-loop
    shape in fp32 with the file's fp32 tolerances."""
    from distributedauc_amd.fused_bn import bn_act

    N, C, H, W = shape
    # ReLU at the tiny shape only: among millions of elements a pre-activation within fp32 rounding of
    # zero makes the fp64 reference's own ReLU mask arbitrary (see _check_fwd_bwd)
    relu = N * H * W < 1000
    torch.manual_seed(len(option) + C)
    bn = nn.BatchNorm2d(C, **_OPTIONS[option]).to(dev).train()
    with torch.no_grad():
        if bn.affine:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
        if bn.track_running_stats:
            bn.running_mean.uniform_(-0.1, 0.1)
            bn.running_var.uniform_(0.9, 1.1)
    ref = copy.deepcopy(bn).cpu().double().train()
    for step in range(2 if option == "cumulative_average" else 1):
        x = (torch.randn(shape, device=dev) * 1.7 + 0.3 * (step + 1)).contiguous(memory_format=torch.channels_last)
        xg = x.clone().requires_grad_(True)
        xr = x.cpu().double().requires_grad_(True)
        y, yr = bn_act(xg, bn, relu, None), ref(xr)
        yr = F.relu(yr) if relu else yr
        ok, e = _close(y, yr, 2e-5)
        assert ok, ("forward", step, e)
        if bn.track_running_stats:
            assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == step + 1
            assert torch.allclose(bn.running_mean.cpu().double(), ref.running_mean, rtol=1e-5, atol=1e-5)
            assert torch.allclose(bn.running_var.cpu().double(), ref.running_var, rtol=1e-5, atol=1e-5)
        else:
            assert bn.running_mean is None and bn.num_batches_tracked is None
        dy = torch.randn_like(x)
        y.backward(dy)
        yr.backward(dy.cpu().double())
        gam = ref.weight.detach().abs() if bn.affine else torch.ones(C, dtype=torch.float64)
        invstd = 1.0 / torch.sqrt(xr.detach().var(dim=(0, 2, 3), unbiased=False) + bn.eps)
        ok, e = _close(xg.grad, xr.grad, 2e-5, float((gam * invstd).max()) * float(dy.abs().max()))
        assert ok, ("dx", step, e)
        if bn.affine:
            for got, want, name in ((bn.weight.grad, ref.weight.grad, "dgamma"), (bn.bias.grad, ref.bias.grad, "dbeta")):
                ok, e = _close(got, want, 1e-4)
                assert ok, (name, step, e)
                got.zero_(), want.zero_()
        else:
            assert bn.weight is None and bn.bias is None
