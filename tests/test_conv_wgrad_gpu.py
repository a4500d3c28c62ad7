"""The 3x3 convolution weight gradient kernel (csrc/conv_wgrad.hip, dauc_conv3x3_wgrad) against an
fp64 reference of the same bf16 operands.

Reference: the weight gradient autograd computes for the ResNet 3x3 convolutions (resnet.py:72-108,
main.py:326), here as torch's fp64 convolution backward on the CPU from the same bf16-rounded x and
dy. The kernel accumulates exact bf16 products in fp32 (MFMA), split over pixel chunks whose fp32
partials are summed in a fixed order: error within fp32 summation noise of the fp64 result
(<= 2e-5 of the tensor's scale here), and bitwise reproducible. Also the transposing LDS read's
lane map (tuning build probe) and the backbone path that uses the kernel.

Which loop each group of cases reaches (a workgroup owns one split: cps consecutive chunks;
tests/test_wgrad_plan_host.py asserts all of this from the launcher's own plan, without a GPU):

* test_conv3x3_wgrad_matches_fp64, 12 small shapes x 6 forms: every layout's geometry and edges
  (Wo of 1, 64 < Wo, one-pixel images, rows that leave a chunk partly empty), with one chunk per
  split in 71 of the 72 and two in one. The gather kernel's in-loop prefetch and the window kernel's
  in-loop staging of its second LDS buffer load a clamped copy nobody reads there: these cases run
  the kernels' prologue and exit.
* test_conv3x3_wgrad_main_loop_* over wgrad_cases.MAIN_CASES, 14 shapes of 10 to 63 chunks: 3 to 5
  chunks per split, so the window kernel stages both buffer parities inside its loop and prefetches
  chunk c + 2 unclamped, the gather kernel prefetches c + 1 unclamped, and the last split holds
  fewer chunks (1 to 3: the loop exits on either parity). Gather at both strides; per-row windows
  with 64- and 128-pixel chunks, with R > Ho and R not dividing Ho (chunks straddle images);
  shared rows with 64 and 128, one image and 2 or 3 images per chunk, both strides; the XCD
  placement of the grid at 8 and 16 splits; a partial and a full last chunk.
* test_conv3x3_wgrad_resnet50_b256: the bench's five shapes, 28 to 64 chunks per split, all of them
  dividing evenly, against MIOpen's fp32 result.
"""
from __future__ import annotations

import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from wgrad_cases import FORMS, MAIN_CASES, NONFINITE_CASES, case_id, out_hw

pytestmark = pytest.mark.gpu


def test_transposing_read_lane_map(dev):
    """ds_read_b64_tr_b16 as the kernel uses it: lane l gets channel 16 + (l & 15) of pixel rows
    8 (l >> 4) .. 8 (l >> 4) + 7 -- the 16x16x32 MFMA operand fragment."""
    from distributedauc_amd import ops

    got = ops.probe_tr16().cpu()
    for lane in range(64):
        g, i = lane >> 4, lane & 15
        want = [(8 * g + j) * 64 + 16 + i for j in range(8)]
        assert got[lane].tolist() == want, (lane, got[lane].tolist(), want)


def _ref_wgrad(x, dy, stride):
    xr = x.detach().cpu().double()
    gr = dy.detach().cpu().double()
    Co, Ci = dy.shape[1], x.shape[1]
    w = torch.zeros((Co, Ci, 3, 3), dtype=torch.float64)
    return torch.ops.aten.convolution_backward(gr, xr, w, None, [stride] * 2, [1, 1], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


@pytest.mark.parametrize("form", ["auto", "gather", "window64", "window128", "shared64", "shared128"])
@pytest.mark.parametrize("N,Ci,Co,H,W,stride", [
    (2, 64, 64, 9, 11, 1), (3, 128, 64, 14, 14, 2), (1, 64, 192, 7, 5, 1), (4, 64, 128, 15, 13, 2),
    (2, 256, 256, 14, 14, 1), (5, 512, 512, 7, 7, 1), (1, 64, 64, 1, 1, 1), (2, 64, 64, 2, 3, 2),
    (3, 64, 64, 70, 9, 1), (2, 64, 128, 131, 5, 2), (1, 64, 64, 3, 70, 1), (2, 64, 64, 5, 131, 2)])
def test_conv3x3_wgrad_matches_fp64(dev, form, N, Ci, Co, H, W, stride):
    """Every form of the kernel: the window form (whole output rows per chunk, the taps read one
    staged input window) with 64- or 128-pixel chunks (Wo <= 64 / 128; the automatic choice takes
    128 where its rows fill 7/8 of the chunk), and the gather form (64-pixel chunks, one gathered
    tile per tap; wider images), and the window form with shared rows (stride 1: a chunk's output
    rows read its R + 2 input rows, per image Ho + 2, when R divides Ho or Ho divides R). The tuning
    build's dauc_set_wgrad_form(1 .. 5) forces one form (a window form that does not fit falls back
    to the gather form)."""
    from distributedauc_amd import _lib, ops

    if form == "auto":
        _check_wgrad(dev, N, Ci, Co, H, W, stride)
        return
    ops.set_wgrad_form({"gather": 1, "window64": 2, "window128": 3, "shared64": 4, "shared128": 5}[form])
    try:
        with _lib.using(_lib.tuning()):
            _check_wgrad(dev, N, Ci, Co, H, W, stride)
    finally:
        ops.set_wgrad_form(0)


def _check_wgrad(dev, N, Ci, Co, H, W, stride):
    from distributedauc_amd import ops

    g = torch.Generator(device=dev).manual_seed(N * 1000 + Ci + Co + H)
    x = torch.randn((N, Ci, H, W), device=dev, generator=g).to(torch.bfloat16)
    x = x.contiguous(memory_format=torch.channels_last)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = torch.randn((N, Co, Ho, Wo), device=dev, generator=g).to(torch.bfloat16)
    dy = dy.contiguous(memory_format=torch.channels_last)
    got = ops.conv3x3_wgrad(x, dy, stride)
    assert got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last)
    ref = _ref_wgrad(x, dy, stride)
    scale = float(ref.abs().max())
    err = float((got.cpu().double() - ref).abs().max())
    assert err <= 2e-5 * scale, (err, scale)
    again = ops.conv3x3_wgrad(x, dy, stride)
    assert torch.equal(got, again)  # fixed summation order


# ---- the main-loop cases (wgrad_cases.MAIN_CASES): three or more chunks per split ----------------

@contextlib.contextmanager
def _form(form):
    """The ops under the case's form: the product library's own choice, or the tuning build with
    that form forced."""
    from distributedauc_amd import _lib, ops

    if form == "auto":
        yield
        return
    ops.set_wgrad_form(FORMS[form])
    try:
        with _lib.using(_lib.tuning()):
            yield
    finally:
        ops.set_wgrad_form(0)


def _channels_last(t, dev):
    return t.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _randn_case(case):
    """(x, dy, fp64 reference, clean result) of a case with randn operands: computed once and shared
    by the tests below, which leave them unchanged."""
    from distributedauc_amd import ops

    N, Ci, Co, H, W, stride, form = case
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(N * 1000 + Ci + Co + H + W)
    Ho, Wo = out_hw(H, W, stride)
    x = _channels_last(torch.randn((N, Ci, H, W), generator=g), dev)
    dy = _channels_last(torch.randn((N, Co, Ho, Wo), generator=g), dev)
    ref = _ref_wgrad(x, dy, stride)
    with _form(form):
        got = ops.conv3x3_wgrad(x, dy, stride)
    return x, dy, ref, got


@pytest.mark.parametrize("case", list(MAIN_CASES), ids=case_id)
def test_conv3x3_wgrad_main_loop_matches_fp64(dev, case):
    """Randn bf16 operands against the fp64 reference at the file's bar, 2e-5 of the tensor's scale,
    and bitwise equal to a second call. Measured on an MI355X: err / scale between 1.46e-7 and
    2.25e-7 over the 14 cases (the worst is auto-7x512x512-7x33-s1), a hundredth of the bar."""
    from distributedauc_amd import ops

    x, dy, ref, got = _randn_case(case)
    assert got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last)
    scale = float(ref.abs().max())
    err = float((got.cpu().double() - ref).abs().max())
    print(f"wgrad main loop {case_id(case)}: err / scale = {err / scale:.3e}")
    assert err <= 2e-5 * scale, (err, scale)
    with _form(case[6]):
        again = ops.conv3x3_wgrad(x, dy, case[5])
    assert torch.equal(got, again)  # fixed summation order


@pytest.mark.parametrize("case", list(MAIN_CASES), ids=case_id)
def test_conv3x3_wgrad_main_loop_exact_on_integers(dev, case):
    """x and dy integer-valued in [-4, 4] (exact in bf16): every product and every partial sum is an
    integer below 2^24, so the fp32 result does not depend on the summation order and must equal
    the fp64 reference exactly -- no tolerance for a dropped, doubled or misplaced chunk, row or tap
    to hide under."""
    from distributedauc_amd import ops

    N, Ci, Co, H, W, stride, form = case
    Ho, Wo = out_hw(H, W, stride)
    assert 16 * N * Ho * Wo < 2 ** 24  # the largest sum of |products| any partial sum can hold
    g = torch.Generator().manual_seed(7 * N + Ci + H + 31 * W)
    x = _channels_last(torch.randint(-4, 5, (N, Ci, H, W), generator=g).float(), dev)
    dy = _channels_last(torch.randint(-4, 5, (N, Co, Ho, Wo), generator=g).float(), dev)
    ref = _ref_wgrad(x, dy, stride)
    assert float(ref.abs().max()) < 2 ** 24 and float(ref.abs().max()) > 0
    with _form(form):
        got = ops.conv3x3_wgrad(x, dy, stride)
    assert torch.equal(got.cpu().double(), ref), int((got.cpu().double() != ref).sum())


@pytest.mark.parametrize("case", list(MAIN_CASES), ids=case_id)
def test_conv3x3_wgrad_main_loop_dirty_memory(dev, case):
    """The pooled split workspace filled with 0xFF bytes and a caller's out= filled with NaN before the
    call: bitwise the clean-memory result (every slab element and every output element is written
    before it is read)."""
    from distributedauc_amd import _lib, ops

    N, Ci, Co, H, W, stride, form = case
    Ho, Wo = out_hw(H, W, stride)
    x, dy, _, clean = _randn_case(case)
    nbytes = _lib.load().dauc_conv3x3_wgrad_workspace_size(N, Ho, Wo, Ci, Co)
    assert nbytes > 0  # several splits: the slabs are in use
    ops.workspaces.get(dev, "wgrad3x3", nbytes).fill_(0xFF)
    out = torch.full((Co, Ci, 3, 3), float("nan"), device=dev).contiguous(memory_format=torch.channels_last)
    with _form(form):
        got = ops.conv3x3_wgrad(x, dy, stride, out=out)
    assert got is out
    assert torch.equal(got, clean)


@pytest.mark.parametrize("case", NONFINITE_CASES, ids=case_id)
def test_conv3x3_wgrad_main_loop_nonfinite_x_stays_in_its_column(dev, case):
    """One inf, one -inf and one nan in x, each in its own input channel: at a chunk's first pixel
    (image 0, h = 0, w = 0), at an image's last column, and at an interior pixel of the last,
    partial chunk. dy has no zeros, so exactly the entries dW[:, that channel, the taps that reach
    the pixel] are non-finite in the fp64 reference; the kernel's set must be the same one (inf or
    NaN is not compared) and its finite entries meet the bar. The window kernel multiplies a chunk's
    padding pixels (zero dy rows) by window position 0 and a partial chunk's missing rows by what
    their loads returned: both must be zeros, never a 0 * inf."""
    from distributedauc_amd import ops

    N, Ci, Co, H, W, stride, form = case
    Ho, Wo = out_hw(H, W, stride)
    x, dy, _, _ = _randn_case(case)
    assert bool((dy != 0).all())
    x = x.clone()
    marks = [(0, 3, 0, 0, float("inf")), (1, 64 + 17, H // 2, W - 1, float("-inf")),
             (N - 1, Ci - 1, stride * (Ho - 1), stride * (Wo - 2) + stride - 1, float("nan"))]
    for n, ci, h, w, v in marks:
        x[n, ci, h, w] = v
    ref = _ref_wgrad(x, dy, stride)
    bad = ~torch.isfinite(ref)
    cols = torch.zeros(Ci, dtype=torch.bool)
    cols[[m[1] for m in marks]] = True
    assert bool((bad.sum(dim=(0, 2, 3)) > 0)[cols].all()) and not bool(bad[:, ~cols].any())  # the reference's own
    with _form(form):
        got = ops.conv3x3_wgrad(x, dy, stride).cpu().double()
    assert torch.equal(~torch.isfinite(got), bad), int((~torch.isfinite(got) != bad).sum())
    scale = float(ref[~bad].abs().max())
    err = float((got[~bad] - ref[~bad]).abs().max())
    print(f"wgrad non-finite {case_id(case)}: err / scale = {err / scale:.3e}, non-finite {int(bad.sum())}")
    assert err <= 2e-5 * scale, (err, scale)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("C,H,stride", [(64, 56, 1), (128, 56, 2), (256, 28, 2), (512, 14, 2), (512, 7, 1)])
def test_conv3x3_wgrad_resnet50_b256(dev, C, H, stride):
    """The bench's shapes (ResNet-50 b256 224^2: layer1 conv2, layer2.0 conv2, layer4 conv2) against
    torch's fp32 convolution backward on the GPU (fp32 operands from the same bf16 values)."""
    from distributedauc_amd import ops

    g = torch.Generator(device=dev).manual_seed(C + H)
    N = 256
    x = torch.relu(torch.randn((N, C, H, H), device=dev, generator=g)).to(torch.bfloat16)
    x = x.contiguous(memory_format=torch.channels_last)
    Ho = (H - 1) // stride + 1
    dy = (torch.randn((N, C, Ho, Ho), device=dev, generator=g) * 1e-3).to(torch.bfloat16)
    dy = dy.contiguous(memory_format=torch.channels_last)
    got = ops.conv3x3_wgrad(x, dy, stride)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        ref = torch.ops.aten.convolution_backward(dy.float(), x.float(), torch.zeros((C, C, 3, 3), device=dev), None,
                                                  [stride] * 2, [1, 1], [1, 1], False, [0, 0], 1,
                                                  [False, True, False])[1]
    finally:
        torch.backends.cudnn.deterministic = det
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= 2e-4 * scale, (err, scale)


def test_conv3x3_wgrad_rejects_unsupported(dev):
    from distributedauc_amd import _lib, ops

    x = torch.randn((2, 48, 8, 8), device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = torch.randn((2, 64, 8, 8), device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert not ops.conv3x3_wgrad_supported(x, dy, 1, 1, 1, 1)
    with pytest.raises(_lib.DaucError):
        ops.conv3x3_wgrad(x, dy, 1)  # Ci = 48: not a multiple of 64
    x = torch.randn((2, 64, 8, 8), device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(_lib.DaucError):
        ops.conv3x3_wgrad(x, dy, 2)  # dy's 8 x 8 is not the stride-2 output size
    with pytest.raises(ValueError):
        ops.conv3x3_wgrad(x.contiguous(), dy, 1)
