"""Table sizes of the sorted exact-AUC path's tests and what csrc/radix_sort.hip and csrc/auc_sort.hip
run at each one.

The sorted path sorts the smaller class (radix_sort_keys), keeps every k-th sorted key as a splitter
of a 5-ary LDS tree (prepare_table: k the smallest power of two with at most kMaxSplit splitters) and
counts with query_count_kernel<K, TABLE_POS> or query_labeled_kernel<K, LT>, K = k up to 32 and 0 past
it (buckets finished by binary searches in global memory). Which scan form the sort runs, which K
counts and how long the runs of the two one-workgroup scans are follows from tuning constants
(kMaxSplit, kFusedScanTiles, the tile sizes), so the plan is read from the library
(dauc_sort_table_plan of the tuning build, include/dauc_tuning.h: the functions the launchers launch
from). tests/test_sort_plan_host.py pins the sizes below to the kernels that
tests/test_auc_tree_gpu.py relies on; a retune that takes a kernel out of their reach fails there,
without a GPU.
"""
from __future__ import annotations

import ctypes

PLAN_NAMES = ("tiles", "scan", "nsum", "per", "k", "S", "H", "nodes", "lds", "pad", "K", "dk_tiles", "dk_per",
              "dk_max", "ci_max_table", "max_split")

# words 13..15 are constants of the build, the same for every M
CONSTANTS = {"dk_max": 14_000, "ci_max_table": 219_838, "max_split": 40_000}

# M -> (tiles, scan, nsum, per, k, S, H, nodes, lds, pad, K, dk_tiles, dk_per): the tree cases. Every K
# template; S at the cap (1,280,000); k = 64 with a one-key last bucket (1,280,001) and a full one
# (1,280,064); k = 256; the scan forms of their sorts and two or more distinct-key tiles per thread.
TREE_PLANS = {
    30_011: (15, 0, 4, 1, 1, 30_011, 7, 7_512, 120_192, 0, 1, 30, 1),
    40_001: (20, 0, 5, 1, 2, 20_001, 7, 5_010, 80_160, 1, 2, 40, 1),
    80_001: (40, 0, 10, 1, 4, 20_001, 7, 5_010, 80_160, 3, 4, 79, 1),
    160_001: (79, 0, 20, 1, 8, 20_001, 7, 5_010, 80_160, 7, 8, 157, 1),
    320_001: (157, 0, 40, 1, 16, 20_001, 7, 5_010, 80_160, 15, 16, 313, 1),
    640_001: (313, 1, 79, 1, 32, 20_001, 7, 5_010, 80_160, 31, 32, 626, 1),
    1_280_000: (625, 1, 157, 1, 32, 40_000, 7, 10_008, 160_128, 0, 32, 1_250, 2),
    1_280_001: (626, 1, 157, 1, 64, 20_001, 7, 5_010, 80_160, 0, 0, 1_251, 2),
    1_280_064: (626, 1, 157, 1, 64, 20_001, 7, 5_010, 80_160, 0, 0, 1_251, 2),
    5_120_001: (2_501, 1, 626, 1, 256, 20_001, 7, 5_010, 80_160, 0, 0, 5_001, 5),
}

# the unlabeled tests' tables (both table sides, modes 0 and 1) and the labeled tests' (every label type;
# 5,120,001 with int8 labels only)
UNLABELED_MS = (30_011, 40_001, 80_001, 160_001, 320_001, 640_001, 1_280_000, 1_280_001, 1_280_064)
LABELED_MS = (640_001, 1_280_000, 1_280_001, 5_120_001)
# the product's routes: the smaller class of about 2.7 M scores
ROUTE_M = 1_300_000

# k = 1 tables at the tree-height boundaries: S = M -> (H, stored nodes). 5^(H-1) <= S + 1 <= 5^H.
HEIGHT_PLANS = {1: (1, 2), 4: (1, 2), 5: (2, 4), 24: (2, 8), 25: (3, 10), 124: (3, 34), 125: (4, 36), 624: (4, 160),
                625: (5, 162), 3_124: (5, 786), 3_125: (6, 788), 15_624: (6, 3_912), 15_625: (7, 3_914)}

# n -> (tiles, scan, nsum, per): the sizes of the key-for-key sort test. One key; around a wave, a
# scatter wave's 512 keys and a tile; whole and ragged tile counts; the last fused sort (256 tiles) and
# the first with scan launches (257 tiles: 65 scan blocks, the last one partial); 1024 tiles (256 whole
# scan blocks); 4097 tiles (1025 block sums: two per scan_sums_kernel thread).
SORT_PLANS = {
    1: (1, 0, 1, 1), 63: (1, 0, 1, 1), 64: (1, 0, 1, 1), 65: (1, 0, 1, 1), 511: (1, 0, 1, 1), 512: (1, 0, 1, 1),
    513: (1, 0, 1, 1), 2_047: (1, 0, 1, 1), 2_048: (1, 0, 1, 1), 2_049: (2, 0, 1, 1), 3 * 2_048: (3, 0, 1, 1),
    4 * 2_048: (4, 0, 1, 1), 5 * 2_048 + 1: (6, 0, 2, 1), 7 * 2_048: (7, 0, 2, 1), 524_288: (256, 0, 64, 1),
    524_289: (257, 1, 65, 1), 2_097_152: (1_024, 1, 256, 1), 8_390_651: (4_097, 1, 1_025, 2),
}
# the sizes that also run the structured inputs (all equal, alternating, ascending, descending, one byte)
SORT_PATTERN_NS = (5 * 2_048 + 1, 524_289)


def plan(M: int) -> dict:
    """dauc_sort_table_plan as a dict (host arithmetic in the tuning build; no GPU)."""
    from distributedauc_amd import _lib

    out = (ctypes.c_int64 * _lib.SORT_PLAN_WORDS)()
    _lib.check(_lib.tuning().dauc_sort_table_plan(M, out), "dauc_sort_table_plan")
    return dict(zip(PLAN_NAMES, (int(v) for v in out)))
