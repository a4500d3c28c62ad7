"""The fused BatchNorm tests' shapes reach the loops they are meant to test (no GPU: the launch plan
is host arithmetic, dauc_bn_launch_plan of the tuning build).

csrc/bn_act.hip chooses its row blocks from the shape (make_geometry: kRowBlockTarget blocks of
whole passes, a pass being RPB = threads / TPR rows), so whether a test shape runs the kernels'
grouped main loops or only their tails depends on the tuning constants. A retune of
kRowBlockTarget, kUnroll or the workgroup size that takes the main loops out of the GPU tests'
reach fails here.
"""
from __future__ import annotations

import ctypes

import pytest

from bn_cases import ALL_CASES, MAIN_CASES, SHAPES, launch_plan, loop_counts, regime
from distributedauc_amd import _lib


@pytest.mark.parametrize("case", list(ALL_CASES), ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_bn_case_reaches_its_regime(case):
    """Every main-loop shape: the recorded loop counts per full row block, forward and backward, with
    at least one main-loop iteration and one tail pass each; the row-block and channel-tile counts;
    a short last block; the finalize's grouped loop where recorded; an elementwise grid with
    unguarded interior workgroups and a partly filled last one."""
    M, C, dtype, _ = case
    want = ALL_CASES[case]
    got = regime(M, C, dtype)
    assert got == want, (got, want)
    for groups, tail in (got.fwd, got.bwd):
        assert groups >= 1 and tail >= 1
    assert got.short_last
    p = launch_plan(M, C, dtype)
    # the short last block runs other loop counts than the full ones (its own row count is in play)
    last = M - (p["nrb"] - 1) * p["rows"]
    assert loop_counts(last, p["RPB"], p["fwd_group_rows"]) != got.fwd
    vec = {"fp32": 4, "bf16": 8}[dtype]
    nvec = M * (C // vec)
    assert p["apply_blocks"] >= 2 and nvec % p["apply_block_vecs"] != 0
    assert p["apply_blocks"] == -(-nvec // p["apply_block_vecs"])
    assert bool(p["hoist"]) == ((C // vec) <= 256)


def test_bn_main_cases_cover_the_regimes():
    """Between them the GPU cases hold: both dtypes; TPR = 256 with RPB = 2; two channel tiles with
    the elementwise kernels' per-vector parameter loads (no hoisting); two main-loop iterations
    forward; a finalize with and without its grouped loop."""
    plans = {c: launch_plan(c[0], c[1], c[2]) for c in MAIN_CASES}
    assert {c[2] for c in MAIN_CASES} == {"fp32", "bf16"}
    assert plans[(4603, 2048, "bf16", "res_relu")]["TPR"] == 256
    assert plans[(4603, 2048, "bf16", "res_relu")]["RPB"] == 2
    assert any(r.ctiles == 2 and not r.hoist for r in MAIN_CASES.values())
    assert any(r.fwd[0] >= 2 for r in MAIN_CASES.values())
    assert {r.fin_grouped for r in MAIN_CASES.values()} == {True, False}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bn_tiny_shapes_are_one_pass_per_block(dtype):
    """The record of the gap the main-loop cases close: every shape of SHAPES (the tiny-M edge, kept)
    has row blocks of exactly one pass, so neither main loop of the partial-sum kernel runs there,
    and too few row blocks for the finalize's grouped loop."""
    for N, C, H, W in SHAPES:
        p = launch_plan(N * H * W, C, dtype)
        assert p["rows"] == p["RPB"], ((N, C, H, W), p)
        r = regime(N * H * W, C, dtype)
        assert r.fwd == (0, 1) and r.bwd == (0, 1) and not r.fin_grouped, ((N, C, H, W), r)


def test_bn_launch_plan_refuses_what_the_kernels_refuse():
    lib = _lib.tuning()
    out = (ctypes.c_int64 * _lib.BN_PLAN_WORDS)()
    assert lib.dauc_bn_launch_plan(64, 96, _lib.DTYPE_BF16, out) == _lib.DAUC_EINVAL  # 12 vectors per row
    assert lib.dauc_bn_launch_plan(0, 64, _lib.DTYPE_F32, out) == _lib.DAUC_EINVAL
    assert lib.dauc_bn_launch_plan(64, 64, 7, out) == _lib.DAUC_EINVAL
    assert lib.dauc_bn_launch_plan(64, 64, _lib.DTYPE_F32, None) == _lib.DAUC_EINVAL
    assert not hasattr(_lib.load(), "dauc_bn_launch_plan") or _lib.load() is lib  # tuning builds only
