"""The 3x3 weight-gradient tests' shapes reach the loops they are meant to test (no GPU: the launch
plan is host arithmetic, dauc_conv3x3_wgrad_launch_plan of the tuning build).

csrc/conv_wgrad.hip chooses the form, the chunk layout and the split count from the shape (win_geom,
win_layout, win_cost, split_count), so whether a test shape runs the kernels' chunk loops in their
steady state or only their prologue and exit depends on tuning constants. A retune of the split
target, the cost model or the layout limits that takes those loops out of the GPU tests' reach
fails here.
"""
from __future__ import annotations

import ctypes

import pytest

from distributedauc_amd import _lib
from wgrad_cases import FORMS, MAIN_CASES, NONFINITE_CASES, SHAPES, case_id, launch_plan, out_hw, regime


@pytest.mark.parametrize("case", list(MAIN_CASES), ids=case_id)
def test_wgrad_case_reaches_its_regime(case):
    """Every main-loop case: the recorded plan words; three or more chunks per split (both LDS buffers
    staged inside the window kernel's loop, an unclamped prefetch in either kernel), a last split
    with fewer chunks, the last chunk partial where recorded; and the plan's own consistency."""
    want = MAIN_CASES[case]
    got = regime(case)
    assert got == want, (got, want)
    assert got.cps >= 3 and got.last_split < got.cps
    N, Ci, Co, H, W, stride, form = case
    Ho, Wo = out_hw(H, W, stride)
    p = launch_plan(N, Ci, Co, H, W, stride, form)
    assert p["tiles"] == (Ci // 64) * (Co // 64)
    assert p["chunks"] == (p["splits"] - 1) * p["cps"] + p["last_split_chunks"]
    assert p["xcd"] == int(bool(p["window"]) and p["tiles"] > 1 and p["splits"] % 8 == 0)
    if p["window"]:
        assert p["KP"] == p["R"] * Wo <= p["KT"] and p["Wd"] == W + 2 and p["KS"] == p["KT"] // 32
        assert p["nvec"] == -(-p["npos"] // 64) and p["lds_bytes"] == 320 * (p["KT"] + p["npos"]) <= 160 * 1024
        if p["shared"]:
            assert Ho % p["R"] == 0 or p["R"] % Ho == 0
            assert p["images"] == max(p["R"] // Ho, 1)
            rows = stride * min(p["R"], Ho) + 3 - stride
            assert p["npos"] == p["images"] * rows * p["Wd"]
        else:
            assert p["images"] == 0 and p["npos"] == 3 * p["R"] * p["Wd"]
    else:
        assert form in ("auto", "gather") and p["chunks"] == -(-N * Ho * Wo // 64)


def test_wgrad_main_cases_cover_the_regimes():
    """Between them the GPU cases hold every layout and every way a chunk run can end."""
    r = {c: regime(c) for c in MAIN_CASES}
    strides = {c: c[5] for c in MAIN_CASES}
    Ho = {c: out_hw(c[3], c[4], c[5])[0] for c in MAIN_CASES}

    def some(pred):
        return any(pred(c, v) for c, v in r.items())

    assert some(lambda c, v: not v.window)
    for KT in (64, 128):
        assert some(lambda c, v: v.window and not v.shared and v.KT == KT)
        assert some(lambda c, v: v.window and v.shared and v.KT == KT)
    for s in (1, 2):
        assert some(lambda c, v: v.shared and v.images >= 2 and strides[c] == s)
    # per-row windows whose chunks straddle images: more rows than an image, and fewer that do not divide it
    assert some(lambda c, v: v.window and not v.shared and v.R > Ho[c])
    assert some(lambda c, v: v.window and not v.shared and 1 < v.R < Ho[c] and Ho[c] % v.R != 0)
    for splits in (8, 16):
        assert some(lambda c, v: v.xcd and v.cps >= 3 and v.splits == splits)
    assert some(lambda c, v: v.cps % 2 == 1) and some(lambda c, v: v.cps % 2 == 0)
    assert some(lambda c, v: v.window and strides[c] == 2) and some(lambda c, v: not v.window and strides[c] == 2)
    assert some(lambda c, v: v.window and v.partial) and some(lambda c, v: v.window and not v.partial)
    assert some(lambda c, v: not v.window and v.partial)
    # the non-finite cases: gather, per-row window, shared rows at either stride; a partial last chunk each
    kinds = {(r[c].window, r[c].shared, strides[c] if r[c].shared else 0) for c in NONFINITE_CASES}
    assert kinds == {(0, 0, 0), (1, 0, 0), (1, 1, 1), (1, 1, 2)}
    assert all(r[c].partial for c in NONFINITE_CASES)


def test_wgrad_small_shapes_run_at_most_two_chunks_per_split():
    """The record of the gap the main-loop cases close: of the 72 small cases (SHAPES in every form,
    kept) 71 give every split one chunk and one gives two (with a one-chunk last split), so neither
    kernel's loop reaches its steady state there; one of them places its grid by XCD, with one
    chunk per split."""
    two, short, xcd = [], [], []
    for shape in SHAPES:
        for form in FORMS:
            p = launch_plan(*shape, form)
            assert p["cps"] <= 2, (shape, form, p)
            if p["cps"] == 2:
                two.append((shape, form))
            if p["last_split_chunks"] < p["cps"]:
                short.append((shape, form))
            if p["xcd"]:
                xcd.append((shape, form, p["cps"]))
    assert two == [((5, 512, 512, 7, 7, 1), "shared64")]
    assert short == two
    assert xcd == [((2, 64, 128, 131, 5, 2), "window128", 1)]


def test_wgrad_window_instantiations_reached():
    """Which wgrad3x3_win_kernel<NV, KS> the launcher can choose. The two LDS buffers of KT + npos
    rows of 160 bytes fit 160 KiB, so KT + npos <= 512 and nvec = ceil(npos / 64) <= 7 with 64-pixel
    chunks, <= 6 with 128: the launcher's cases (8, 2), (7, 4) and (8, 4) are never taken. The sweep
    reaches every other one."""
    reached = set()
    for form in ("auto", "window64", "window128", "shared64", "shared128"):
        for W in range(1, 131):
            for stride in (1, 2):
                for H in (1, 7, 14):
                    for N in (1, 8):
                        p = launch_plan(N, 64, 64, H, W, stride, form)
                        assert p is not None, (form, N, H, W, stride)  # outside the launcher's switch: refused
                        if p["window"]:
                            assert p["KT"] + p["npos"] <= 512
                            reached.add((p["nvec"], p["KS"]))
    switch = {(nv, ks) for nv in range(1, 9) for ks in (2, 4)}
    assert reached <= switch
    assert not any(nv == 8 for nv, _ in reached) and (7, 4) not in reached
    assert reached == switch - {(8, 2), (7, 4), (8, 4)}


def test_wgrad_launch_plan_refuses_what_the_launcher_refuses():
    lib = _lib.tuning()
    out = (ctypes.c_int64 * _lib.WGRAD_PLAN_WORDS)()
    plan = lib.dauc_conv3x3_wgrad_launch_plan
    assert plan(2, 8, 8, 64, 8, 8, 64, 1, out) == _lib.DAUC_OK
    assert plan(2, 8, 8, 48, 8, 8, 64, 1, out) == _lib.DAUC_EINVAL  # Ci = 48: not a multiple of 64
    assert plan(2, 8, 8, 64, 8, 8, 96, 1, out) == _lib.DAUC_EINVAL
    assert plan(2, 8, 8, 64, 3, 3, 64, 3, out) == _lib.DAUC_EINVAL  # stride 3
    assert plan(2, 8, 8, 64, 8, 8, 64, 2, out) == _lib.DAUC_EINVAL  # 8 x 8 is not the stride-2 output size
    assert plan(2, 8, 8, 64, 4, 4, 64, 2, out) == _lib.DAUC_OK
    assert plan(0, 8, 8, 64, 8, 8, 64, 1, out) == _lib.DAUC_EINVAL
    assert plan(2, 8, 8, 64, 8, 8, 64, 1, None) == _lib.DAUC_EINVAL
    assert not hasattr(_lib.load(), "dauc_conv3x3_wgrad_launch_plan") or _lib.load() is lib  # tuning builds only


def test_wgrad_launch_plan_honours_the_forced_form():
    """dauc_set_wgrad_form acts on the plan as on the launch: a forced window form where it fits, the
    gather form where it does not, and the automatic choice again afterwards."""
    shape = (2, 64, 64, 9, 11, 1)
    assert launch_plan(*shape, "gather")["window"] == 0
    for form, KT, shared in (("window64", 64, 0), ("window128", 128, 0), ("shared64", 64, 1), ("shared128", 128, 1)):
        p = launch_plan(*shape, form)
        assert (p["window"], p["KT"], p["shared"]) == (1, KT, shared), (form, p)
    assert launch_plan(1, 64, 64, 3, 70, 1, "window64")["window"] == 0  # Wo = 70 > 64: falls back
    assert launch_plan(*shape)["window"] == 1
