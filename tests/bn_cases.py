"""Shapes of the fused BatchNorm tests and the loops of csrc/bn_act.hip each one runs.

The partial-sum kernel walks a row block in passes of RPB rows: its main loop takes whole groups of
passes (all loads of a group issued before any math), its tail the remaining passes one by one. The
finalize folds the partial rows the same way (a grouped loop, then a tail), and the elementwise
kernels run unguarded interior workgroups and one guarded last workgroup. Which of these a shape
runs follows from the launch plan (dauc_bn_launch_plan of the tuning build, include/dauc_tuning.h:
the launchers' own geometry and constants). tests/test_bn_plan_host.py asserts, from that plan, that
the shapes below reach what the GPU tests of tests/test_fused_bn_gpu.py rely on.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

# the tiny-M edge: every row block of these is exactly one pass (rows == RPB), in both dtypes
SHAPES = [(4, 64, 7, 9), (2, 256, 5, 5), (3, 2048, 3, 3), (8, 128, 14, 14), (2, 64, 1, 1), (2, 32, 33, 17)]


class Regime(NamedTuple):
    """What a shape runs, per full row block (fwd / bwd: main-loop iterations, tail passes)."""
    fwd: tuple
    bwd: tuple
    nrb: int
    ctiles: int
    short_last: bool   # the last row block holds fewer rows than the others
    fin_grouped: bool  # the finalize's grouped loop runs
    hoist: bool        # elementwise kernels: a thread's channels never change


# (M, C, dtype, mode) -> regime. The smallest shapes that run every main loop: [M, C] activations,
# given to the kernels as (1, C, M, 1) channels-last tensors.
MAIN_CASES = {
    (147533, 64, "bf16", "relu"): Regime((1, 2), (2, 2), 231, 1, True, True, True),
    (4603, 2048, "bf16", "res_relu"): Regime((1, 1), (2, 1), 256, 1, True, True, True),
    (2301, 2048, "fp32", "plain"): Regime((1, 1), (2, 1), 128, 2, True, False, False),
    (36869, 256, "fp32", "res_relu"): Regime((2, 3), (4, 3), 243, 1, True, True, True),
    (86393, 128, "bf16", "plain"): Regime((1, 3), (2, 3), 246, 1, True, True, True),
}
# mean far from zero: M = 4603 * (2048 / C) rows of C = 64 channels, so that the main loops run and
# every block has its own shift k
FAR_MEAN_CASES = {
    (147296, 64, "fp32", "plain"): Regime((2, 2), (4, 2), 256, 1, True, True, True),
    (147296, 64, "bf16", "plain"): Regime((1, 1), (2, 1), 256, 1, True, True, True),
}
# the module options' main-loop shape (the tiny one is SHAPES[0])
OPTION_CASE = {(4603, 1024, "fp32", "plain"): Regime((1, 1), (2, 1), 256, 1, True, True, True)}

ALL_CASES = {**MAIN_CASES, **FAR_MEAN_CASES, **OPTION_CASE}


def launch_plan(M: int, C: int, dtype: str) -> dict:
    """dauc_bn_launch_plan as a dict (host arithmetic in the tuning build; no GPU)."""
    from distributedauc_amd import _lib

    out = (ctypes.c_int64 * _lib.BN_PLAN_WORDS)()
    code = {"fp32": _lib.DTYPE_F32, "bf16": _lib.DTYPE_BF16}[dtype]
    _lib.check(_lib.tuning().dauc_bn_launch_plan(M, C, code, out), "dauc_bn_launch_plan")
    names = ("TPR", "RPB", "ctiles", "nrb", "rows", "fwd_group_rows", "bwd_group_rows", "fin_group", "fin_subsets",
             "apply_block_vecs", "apply_blocks", "hoist")
    return dict(zip(names, (int(v) for v in out)))


def loop_counts(nb: int, RPB: int, group_rows: int, r0: int = 0) -> tuple:
    """(main-loop iterations, tail passes) of the thread on row r0 of a pass over a block of nb rows:
    bn_partial_kernel's `for (; r + step - RPB < re; r += step)` then `for (; r < re; r += RPB)`."""
    r, groups, tail = r0, 0, 0
    while r + group_rows - RPB < nb:
        r += group_rows
        groups += 1
    while r < nb:
        r += RPB
        tail += 1
    return groups, tail


def regime(M: int, C: int, dtype: str) -> Regime:
    p = launch_plan(M, C, dtype)
    rows, RPB = p["rows"], p["RPB"]
    last = M - (p["nrb"] - 1) * rows
    assert 0 < last <= rows and rows % RPB == 0
    return Regime(loop_counts(rows, RPB, p["fwd_group_rows"]), loop_counts(rows, RPB, p["bwd_group_rows"]),
                  p["nrb"], p["ctiles"], last < rows, p["nrb"] > p["fin_group"] - p["fin_subsets"], bool(p["hoist"]))
