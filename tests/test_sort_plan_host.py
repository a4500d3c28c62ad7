"""The sorted exact-AUC path's test sizes reach the kernels they are meant to test (no GPU: the plan is
host arithmetic, dauc_sort_table_plan of the tuning build).

csrc/auc_sort.hip picks the bucket size k, and with it the instantiation of the tree kernels, from the
table size and kMaxSplit; csrc/radix_sort.hip picks its scan form from the tile count and
kFusedScanTiles. Once already a retune (32767 -> 40000 splitters) moved the tests' tables to other
kernels than their docstrings named. A retune that takes a kernel out of reach of the sizes in
tests/sort_cases.py fails here.
"""
from __future__ import annotations

import ctypes

import pytest

from distributedauc_amd import _lib
from sort_cases import (CONSTANTS, HEIGHT_PLANS, LABELED_MS, PLAN_NAMES, ROUTE_M, SORT_PATTERN_NS, SORT_PLANS,
                        TREE_PLANS, UNLABELED_MS, plan)

TREE_WORDS = PLAN_NAMES[:13]


@pytest.mark.parametrize("M", list(TREE_PLANS))
def test_tree_case_plan_is_the_recorded_one(M):
    """Every tree case: the recorded plan words, the build's constants, and the plan's own consistency."""
    p = plan(M)
    assert tuple(p[n] for n in TREE_WORDS) == TREE_PLANS[M], p
    assert {n: p[n] for n in CONSTANTS} == CONSTANTS
    k, S = p["k"], p["S"]
    assert k & (k - 1) == 0 and S == -(-M // k) <= p["max_split"]
    assert k == 1 or -(-M // (k // 2)) > p["max_split"]  # the smallest such k
    assert p["K"] == (k if k <= 32 else 0)
    assert p["pad"] == (S * k - M if k <= 32 else 0) and 0 <= p["pad"] < k
    assert 5 ** (p["H"] - 1) <= S + 1 <= 5 ** p["H"]
    assert p["lds"] == 16 * p["nodes"] and p["lds"] + 3 * 16 * 8 <= 160 * 1024  # + the block reduction's words
    assert p["nodes"] >= -(-S // 4) + p["H"]  # 4 keys per node, one padding node per level
    assert p["tiles"] == -(-M // 2048) and p["nsum"] == -(-p["tiles"] * 256 // 1024)
    assert p["dk_tiles"] == -(-M // 1024) and p["dk_per"] == -(-p["dk_tiles"] // 1024)


def test_tree_cases_cover_the_kernels():
    """Between them the tree cases hold every K template, S at its cap, both last-bucket fills of a
    binary-searched bucket, and a distinct-key scan thread with two or more tiles."""
    plans = {M: plan(M) for M in TREE_PLANS}
    assert set(UNLABELED_MS) | set(LABELED_MS) == set(TREE_PLANS)
    assert {plans[M]["K"] for M in UNLABELED_MS} == {1, 2, 4, 8, 16, 32, 0}
    assert [plans[M]["K"] for M in LABELED_MS] == [32, 32, 0, 0]
    assert [plans[M]["k"] for M in LABELED_MS] == [32, 32, 64, 256]
    # past the count index's largest table, so the labeled call's mode 0 builds none and reaches the tree
    assert all(M > plans[M]["ci_max_table"] for M in LABELED_MS)
    for group in (UNLABELED_MS, LABELED_MS):
        assert sum(plans[M]["S"] == plans[M]["max_split"] for M in group) == 1
        assert any(plans[M]["S"] == plans[M]["max_split"] and plans[M]["lds"] == 160_128 for M in group)
    deep = [M for M in UNLABELED_MS if plans[M]["k"] > 32]  # buckets with bounds: no padding
    last = {M: M - (plans[M]["S"] - 1) * plans[M]["k"] for M in deep}
    assert sorted(last.values()) == [1, 64] and all(plans[M]["k"] == 64 for M in deep), last
    assert all(p["H"] == 7 for p in plans.values())
    assert any(p["dk_per"] >= 2 for p in plans.values()) and any(p["dk_per"] == 1 for p in plans.values())
    r = plan(ROUTE_M)  # the product's routes: K = 0 on either side
    assert r["K"] == 0 and r["k"] == 64 and ROUTE_M > r["ci_max_table"]


@pytest.mark.parametrize("S", list(HEIGHT_PLANS))
def test_height_case_plan(S):
    """k = 1 tables whose S = M sits on either side of every tree-height boundary 5^h - 1."""
    p = plan(S)
    assert (p["k"], p["K"], p["S"], p["pad"]) == (1, 1, S, 0)
    assert (p["H"], p["nodes"]) == HEIGHT_PLANS[S], p
    assert 5 ** (p["H"] - 1) <= S + 1 <= 5 ** p["H"]


def test_height_cases_sit_on_the_boundaries():
    hs = {S: plan(S)["H"] for S in HEIGHT_PLANS}
    for h in range(1, 7):
        assert hs[5 ** h - 1] == h and hs[5 ** h] == h + 1
    assert hs[1] == 1


@pytest.mark.parametrize("n", list(SORT_PLANS))
def test_sort_case_plan_is_the_recorded_one(n):
    p = plan(n)
    assert (p["tiles"], p["scan"], p["nsum"], p["per"]) == SORT_PLANS[n], p
    assert p["per"] == -(-p["nsum"] // 1024)


def test_sort_cases_cover_the_scan_forms():
    """Both scan forms on either side of their boundary, a partial and a whole last scan block, the
    block-sum scan with one sum per thread and with two; the structured inputs run in both forms."""
    plans = {n: plan(n) for n in SORT_PLANS}
    fused = [n for n, p in plans.items() if p["scan"] == 0]
    three = [n for n, p in plans.items() if p["scan"] == 1]
    assert max(plans[n]["tiles"] for n in fused) + 1 == min(plans[n]["tiles"] for n in three)
    assert {plans[n]["per"] for n in three} == {1, 2}
    assert any(plans[n]["tiles"] * 256 % 1024 for n in three) and any(plans[n]["tiles"] * 256 % 1024 == 0 for n in three)
    assert any(plans[n]["per"] >= 2 and plans[n]["nsum"] % plans[n]["per"] for n in three)  # a short last run
    assert [plans[n]["scan"] for n in SORT_PATTERN_NS] == [0, 1]
    assert {plan(M)["scan"] for M in TREE_PLANS} == {0, 1}


def test_sort_table_plan_refuses_what_the_entry_points_refuse():
    lib = _lib.tuning()
    out = (ctypes.c_int64 * _lib.SORT_PLAN_WORDS)()
    f = lib.dauc_sort_table_plan
    assert f(1, out) == _lib.DAUC_OK and f(0xffffffff, out) == _lib.DAUC_OK
    assert f(0, out) == _lib.DAUC_EINVAL and f(-5, out) == _lib.DAUC_EINVAL
    assert f(0x100000000, out) == _lib.DAUC_EINVAL
    assert f(1000, None) == _lib.DAUC_EINVAL
    assert not hasattr(_lib.load(), "dauc_sort_table_plan") or _lib.load() is lib  # tuning builds only
