"""Shapes of the 3x3 weight-gradient tests and the loops of csrc/conv_wgrad.hip each one runs.

Both kernels give a workgroup one split: a run of cps consecutive chunks (64 output pixels in the
gather form, R whole output rows in the window form). The gather kernel stages chunk c and loads
chunk c + 1 into registers before it multiplies; the window kernel has two LDS buffers, stages
chunk c + 1 into the other one and loads chunk c + 2. With cps == 1 only the prologue and the exit
run; from cps == 3 on both buffer parities are staged inside the loop and the prefetch index is
unclamped at least once, and a last split with fewer chunks ends the loop on another parity or
count. Which of these a shape runs follows from the launch plan (dauc_conv3x3_wgrad_launch_plan of
the tuning build, include/dauc_tuning.h: the function the launcher launches from).
tests/test_wgrad_plan_host.py asserts, from that plan, that the shapes below reach what the GPU
tests of tests/test_conv_wgrad_gpu.py rely on.
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import NamedTuple

FORMS = {"auto": 0, "gather": 1, "window64": 2, "window128": 3, "shared64": 4, "shared128": 5}

# the small shapes of test_conv3x3_wgrad_matches_fp64 (each run in every form): one chunk per split
# in all but one of them
SHAPES = [(2, 64, 64, 9, 11, 1), (3, 128, 64, 14, 14, 2), (1, 64, 192, 7, 5, 1), (4, 64, 128, 15, 13, 2),
          (2, 256, 256, 14, 14, 1), (5, 512, 512, 7, 7, 1), (1, 64, 64, 1, 1, 1), (2, 64, 64, 2, 3, 2),
          (3, 64, 64, 70, 9, 1), (2, 64, 128, 131, 5, 2), (1, 64, 64, 3, 70, 1), (2, 64, 64, 5, 131, 2)]

PLAN_NAMES = ("window", "KT", "shared", "R", "KP", "Wd", "npos", "nvec", "images", "tiles", "chunks", "cps", "splits",
              "last_split_chunks", "last_chunk", "xcd", "lds_bytes", "KS")


class Regime(NamedTuple):
    """What a case runs: the layout, the split of its chunks, and what its last chunk holds."""
    window: int      # 0 gather, 1 window
    KT: int
    shared: int
    R: int           # output rows per chunk (0: gather)
    nvec: int
    images: int      # images per chunk (0: not shared)
    chunks: int
    cps: int
    splits: int
    last_split: int  # chunks of the last split
    last_chunk: int  # output rows (window) or pixels (gather) of the last chunk
    partial: bool    # the last chunk holds fewer than the others
    xcd: int


# (N, Ci, Co, H, W, stride, form) -> regime. The smallest shapes at which every split but the last
# runs its chunk loop 3 or more times and the last split fewer: 512 x 512 channels are 64 tiles,
# hence 4 splits, so 10 chunks give 3 + 3 + 3 + 1.
MAIN_CASES = {
    (7, 512, 512, 9, 33, 2, "auto"): Regime(0, 64, 0, 0, 0, 0, 10, 3, 4, 1, 19, True, 0),
    (7, 512, 512, 7, 33, 1, "auto"): Regime(1, 128, 0, 3, 5, 0, 17, 5, 4, 2, 1, True, 0),
    (10, 512, 512, 10, 7, 1, "auto"): Regime(1, 128, 1, 10, 2, 1, 10, 3, 4, 1, 10, False, 0),
    (19, 512, 512, 4, 11, 1, "auto"): Regime(1, 128, 1, 8, 3, 2, 10, 3, 4, 1, 4, True, 0),
    (19, 512, 512, 3, 21, 2, "auto"): Regime(1, 64, 1, 4, 4, 2, 10, 3, 4, 1, 2, True, 0),
    (10, 384, 384, 9, 20, 1, "auto"): Regime(1, 64, 1, 3, 2, 1, 30, 4, 8, 2, 3, False, 1),
    (8, 384, 384, 14, 20, 1, "auto"): Regime(1, 128, 0, 5, 6, 0, 23, 3, 8, 2, 2, True, 1),
    (11, 512, 512, 5, 14, 1, "gather"): Regime(0, 64, 0, 0, 0, 0, 13, 4, 4, 1, 2, True, 0),
    (7, 256, 256, 9, 33, 1, "window64"): Regime(1, 64, 0, 1, 2, 0, 63, 4, 16, 3, 1, False, 1),
    (9, 512, 512, 10, 7, 1, "window64"): Regime(1, 64, 0, 9, 4, 0, 10, 3, 4, 1, 9, False, 0),
    (11, 512, 512, 9, 20, 2, "window64"): Regime(1, 64, 0, 6, 7, 0, 10, 3, 4, 1, 1, True, 0),
    (12, 512, 512, 14, 5, 1, "window128"): Regime(1, 128, 0, 18, 6, 0, 10, 3, 4, 1, 6, True, 0),
    (6, 512, 512, 9, 20, 1, "shared64"): Regime(1, 64, 1, 3, 2, 1, 18, 5, 4, 3, 3, False, 0),
    (28, 512, 512, 3, 18, 2, "shared128"): Regime(1, 128, 1, 6, 5, 3, 10, 3, 4, 1, 2, True, 0),
}

# non-finite x: one gather, one per-row window, one shared stride 1, one shared stride 2; each with
# a partial last chunk
NONFINITE_CASES = [(7, 512, 512, 9, 33, 2, "auto"), (7, 512, 512, 7, 33, 1, "auto"),
                   (19, 512, 512, 4, 11, 1, "auto"), (19, 512, 512, 3, 21, 2, "auto")]


def case_id(case) -> str:
    return "{6}-{0}x{1}x{2}-{3}x{4}-s{5}".format(*case)


def out_hw(H: int, W: int, stride: int) -> tuple:
    return (H - 1) // stride + 1, (W - 1) // stride + 1


@contextlib.contextmanager
def forced(form: str):
    """The tuning build's form switch set for the block (dauc_set_wgrad_form), then back to automatic."""
    from distributedauc_amd import _lib

    lib = _lib.tuning()
    _lib.check(lib.dauc_set_wgrad_form(FORMS[form]), "dauc_set_wgrad_form")
    try:
        yield lib
    finally:
        lib.dauc_set_wgrad_form(0)


def launch_plan(N: int, Ci: int, Co: int, H: int, W: int, stride: int, form: str = "auto"):
    """dauc_conv3x3_wgrad_launch_plan under `form` as a dict (host arithmetic in the tuning build; no
    GPU), or None where the launcher refuses the shape."""
    from distributedauc_amd import _lib

    Ho, Wo = out_hw(H, W, stride)
    out = (ctypes.c_int64 * _lib.WGRAD_PLAN_WORDS)()
    with forced(form) as lib:
        rc = lib.dauc_conv3x3_wgrad_launch_plan(N, H, W, Ci, Ho, Wo, Co, stride, out)
    if rc == _lib.DAUC_EINVAL:
        return None
    _lib.check(rc, "dauc_conv3x3_wgrad_launch_plan")
    return dict(zip(PLAN_NAMES, (int(v) for v in out)))


def regime(case) -> Regime:
    N, Ci, Co, H, W, stride, form = case
    p = launch_plan(N, Ci, Co, H, W, stride, form)
    Ho, Wo = out_hw(H, W, stride)
    full = p["R"] if p["window"] else 64
    total = N * Ho if p["window"] else N * Ho * Wo
    assert p["chunks"] == -(-total // full) and 0 < p["last_chunk"] <= full
    assert p["splits"] == -(-p["chunks"] // p["cps"]) and 0 < p["last_split_chunks"] <= p["cps"]
    return Regime(p["window"], p["KT"], p["shared"], p["R"], p["nvec"], p["images"], p["chunks"], p["cps"],
                  p["splits"], p["last_split_chunks"], p["last_chunk"], p["last_chunk"] < full, p["xcd"])
