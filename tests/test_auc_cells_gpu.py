"""The search structures of the sort method (auc_sort.hip, count_index.hip, count_query.hip;
dauc_set_search_mode of the tuning build, include/dauc_tuning.h) vs the C oracle.

The labeled query pass (dauc_auc_counts_sorted_labeled, and through it dauc_auc_eval_counts)
locates every negative among the sorted positives through one of: the count index (mode 0, the
default where it fits: top 11 key bits -> bucket, multiply-high -> cell, per-8-cell LDS words of
base + nibble counts, one 16-byte window for non-empty cells; for a table it cannot hold -- more
than 1.5 keys per cell, or a cell of 15+ keys -- the device falls back to the distinct-key index
where that holds the table, else to the tree), the LDS search tree (mode 1), or the LDS
distinct-key index with the tree behind it (mode 2). Every case here runs in modes 0 and 1, so the
skewed cases also cover mode 0's device-side fallback; the tile-boundary case runs all three.
Bar: the integers (W, T) bit-exact against oracle/auc_oracle.c (sklearn's _binary_clf_curve counts,
main.py:79-81) on the same scores.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import coracle

pytestmark = pytest.mark.gpu

MODES = (0, 1)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture
def ops(dev):
    """The ops run against the tuning build of the library, where the search mode is selectable."""
    from distributedauc_amd import _lib
    from distributedauc_amd import ops as o

    with _lib.using(_lib.tuning()):
        try:
            yield o
        finally:
            o.set_search_mode(0)
            o.set_direct_fault(0)
            o.set_index_form(0)


def _oracle_slice(s, y, begin, end):
    """(W, T) of all positives against the slice's non-positives (labels != 1)."""
    pos = s[y == 1]
    neg = s[begin:end][y[begin:end] != 1]
    yy = np.concatenate([np.ones(pos.size, np.int64), -np.ones(neg.size, np.int64)])
    e = coracle.auc_counts(yy, np.concatenate([pos, neg]))
    return e["wins"], e["ties"]


def _check(ops, dev, s, y, begin=0, end=None, modes=MODES, what=""):
    end = s.size if end is None else end
    ref = _oracle_slice(s, y, begin, end)
    ts, ty = T(s, dev), T(y, dev)
    tpos = T(s[y == 1], dev)
    for m in modes:
        ops.set_search_mode(m)
        wt = torch.zeros(3, dtype=torch.int64, device=dev)
        ops.auc_counts_sorted_labeled(tpos, ts, ty, begin, end, wt, nonfinite=wt[2:])
        got = tuple(wt[:2].cpu().tolist())
        assert got == ref, (what, m, got, ref)
        assert int(wt[2]) == 0, (what, m)


def _labels(rng, n, p, dtype=np.int8):
    return np.where(rng.random(n) < p, 1, -1).astype(dtype)


def test_cells_uniform_scores(dev, ops):
    """The bench's distribution (U(0,1) fp32, loader.synthetic_scores) at table sizes that need
    mu = 4, 5 and 6 keys per cell (134k, 168k, 200k positives) and a few small tables."""
    rng = np.random.default_rng(1)
    for n, P in ((1 << 20, 1), (1 << 20, 2), (1 << 20, 17), (1 << 20, 4_000), (1 << 21, 134_447),
                 (1 << 21, 168_478), (1 << 21, 200_000)):
        s = rng.random(n, dtype=np.float32)
        y = -np.ones(n, np.int8)
        y[rng.choice(n, P, replace=False)] = 1
        _check(ops, dev, s, y, what=(n, P))


def test_cells_signed_wide_and_special_values(dev, ops):
    """Normal scores of both signs over 60 binades, +-0, subnormals, the largest finite values:
    keys spread over many top buckets, empty buckets between them, ties between -0 and +0."""
    rng = np.random.default_rng(2)
    n = 1 << 20
    s = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 3.4e38, -3.4e38, 1.0, -1.0], np.float32)
    k = rng.random(n) < 0.02
    s[k] = rng.choice(special, int(k.sum()))
    y = _labels(rng, n, 0.03)
    _check(ops, dev, s, y, what="wide")
    # all positives at the two extremes of the key range (first and last top buckets)
    s2 = rng.random(n, dtype=np.float32) - 0.5
    y2 = _labels(rng, n, 0.0)
    y2[:50] = 1
    s2[:25] = -3.4e38
    s2[25:50] = 3.4e38
    _check(ops, dev, s2, y2, what="extremes")


def test_cells_ties_and_overflowing_cells(dev, ops):
    """Quantised scores: runs of equal keys longer than a cell's nibble can count (the count
    index finds a cell of 15+ keys and leaves the table to the distinct-key index or the tree),
    and a run of 20 equal keys in one cell with the rest of the table uniform, ties across cell
    edges."""
    rng = np.random.default_rng(3)
    n = 1 << 20
    for levels, p in ((3001, 0.01), (97, 0.05), (5, 0.2), (1, 0.01)):
        s = (np.floor(rng.random(n) * levels) / levels).astype(np.float32)
        y = _labels(rng, n, p)
        _check(ops, dev, s, y, what=("levels", levels))
    s = rng.random(n, dtype=np.float32)
    y = _labels(rng, n, 0.02)
    pos_idx = np.flatnonzero(y == 1)
    s[pos_idx[:20]] = np.float32(0.625)        # one cell holds a 20-key run of 0.625
    neg_idx = np.flatnonzero(y == -1)
    s[neg_idx[:1000]] = np.float32(0.625)      # negatives tied with it
    s[neg_idx[1000:2000]] = np.nextafter(np.float32(0.625), np.float32(1))
    s[neg_idx[2000:3000]] = np.nextafter(np.float32(0.625), np.float32(0))
    _check(ops, dev, s, y, what="run of 20")


def test_cells_clustered_table(dev, ops):
    """90 % of the positives inside a 1e-4-wide interval: the cells of their top bucket hold
    hundreds of keys each (the count index marks the table skewed on the device; the
    distinct-key index or the tree counts it)."""
    rng = np.random.default_rng(4)
    n = 1 << 20
    s = rng.random(n, dtype=np.float32)
    y = _labels(rng, n, 0.01)
    pos_idx = np.flatnonzero(y == 1)
    c = pos_idx[: int(0.9 * pos_idx.size)]
    s[c] = (0.7 + 1e-4 * rng.random(c.size)).astype(np.float32)
    neg_idx = np.flatnonzero(y == -1)
    s[neg_idx[:50_000]] = (0.7 + 1e-4 * rng.random(50_000)).astype(np.float32)
    _check(ops, dev, s, y, what="cluster")


@pytest.mark.parametrize("ldtype", [np.int8, np.int32, np.int64])
def test_cells_label_types_and_ranges(dev, ops, ldtype):
    """Unaligned [begin, end) slices (the sharded evaluation's index ranges), labels 0 (a
    negative for pos_label=1), every label dtype."""
    rng = np.random.default_rng(5)
    n = 300_001
    s = rng.random(n, dtype=np.float32)
    y = _labels(rng, n, 0.02, ldtype)
    y[rng.random(n) < 0.01] = 0
    for begin, end in ((0, n), (3, n - 5), (1, 2), (n // 3, 2 * n // 3 + 1), (7, 7)):
        _check(ops, dev, s, y, begin, end, what=(begin, end))


TILE_N = 20_011
TILE_PS = (1, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
TILE_RANGES = ((0, TILE_N), (3, TILE_N - 5))


@pytest.fixture(scope="module")
def tile_cases():
    """One score vector and, per table size, the positives' places and the oracle's (W, T) over
    both query ranges -- computed once for the three label dtypes."""
    rng = np.random.default_rng(20_011)
    s = rng.random(TILE_N, dtype=np.float32)
    cases = []
    for P in TILE_PS:
        y = -np.ones(TILE_N, np.int8)
        y[rng.choice(TILE_N, P, replace=False)] = 1
        cases.append((P, y, {r: _oracle_slice(s, y, *r) for r in TILE_RANGES}))
    return s, cases


@pytest.mark.parametrize("ldtype", [np.int8, np.int32, np.int64])
def test_cells_tile_boundaries(dev, ops, tile_cases, ldtype):
    """Tables of 1 .. 4097 positives inside 20,011 scores: one key, and one below / at / one past
    a distinct-key tile (1024 keys), a sort tile (2048) and two sort tiles -- the sizes at which a
    tile's tail, or a workspace region carved a region too early, first shows. Every search mode
    (count index, tree, distinct-key index), every label dtype, the whole range and an unaligned
    one; no non-finite score is counted."""
    s, cases = tile_cases
    ts = T(s, dev)
    for P, y, refs in cases:
        ty, tpos = T(y.astype(ldtype), dev), T(s[y == 1], dev)
        for m in (0, 1, 2):
            ops.set_search_mode(m)
            for (begin, end), ref in refs.items():
                wt = torch.zeros(3, dtype=torch.int64, device=dev)
                ops.auc_counts_sorted_labeled(tpos, ts, ty, begin, end, wt, nonfinite=wt[2:])
                assert tuple(wt[:2].cpu().tolist()) == ref, (P, m, begin, end)
                assert int(wt[2]) == 0, (P, m, begin, end)


def test_cells_table_size_limits(dev, ops):
    """Table sizes around the count index's limit of 1.5 keys per cell (219,838 keys at most):
    215,040 and 215,041 are within it, 400,000 and the two larger tables are past it and have far
    more than 14,000 distinct keys, so the tree counts them in every mode."""
    rng = np.random.default_rng(6)
    n = 1 << 22
    for P in (215_040, 215_041, 400_000, 573_440, 573_441):
        s = rng.random(n, dtype=np.float32)
        y = -np.ones(n, np.int8)
        y[rng.choice(n, P, replace=False)] = 1
        _check(ops, dev, s, y, what=P)


def test_cells_one_call_eval(dev, ops):
    """dauc_auc_eval_counts in every mode, the speculative table size included (the same data
    twice, then other data of the same length)."""
    rng = np.random.default_rng(7)
    n = 1 << 21
    data = [(rng.random(n, dtype=np.float32), _labels(rng, n, p)) for p in (0.001, 0.01, 0.001)]
    for m in MODES:
        ops.set_search_mode(m)
        for s, y in (data[0], data[0], data[1], data[2], data[2]):
            W, Tt, P, N, bad, other = ops.auc_eval_counts(T(s, dev), T(y, dev))
            e = coracle.auc_counts(y.astype(np.int64), s)
            assert (W, Tt, P, N, bad) == (e["wins"], e["ties"], e["P"], e["N"], 0), m


def test_cells_rejects_nonfinite_queries(dev, ops):
    """A NaN / inf negative is counted by the cell pass too (sklearn _ranking.py:868-869)."""
    rng = np.random.default_rng(8)
    n = 100_003
    for m in MODES:
        ops.set_search_mode(m)
        for bad in (np.nan, np.inf, -np.inf):
            s = rng.random(n, dtype=np.float32)
            y = _labels(rng, n, 0.01)
            s[int(np.flatnonzero(y == -1)[5])] = bad
            wt = torch.zeros(3, dtype=torch.int64, device=dev)
            ops.auc_counts_sorted_labeled(T(s[y == 1], dev), T(s, dev), T(y, dev), 0, n, wt, nonfinite=wt[2:])
            assert int(wt[2]) == 1, (m, bad)


def test_search_mode_rejects_unknown(dev, ops):
    from distributedauc_amd._lib import DaucError

    with pytest.raises(DaucError):
        ops.set_search_mode(3)


@pytest.mark.parametrize("fault", [1, 2, 3])
def test_direct_build_guards_bad_indices(dev, ops, fault):
    """The direct count-index build checks every cell index and counter before its scatter stores
    (count_index.hip, direct_scatter_kernel): the tuning build corrupts one key's cell (past the last
    cell / moved to the next cell) or one cell's counter between the count and scatter passes, and
    the evaluation reports verdict 2 -- the blocking call then takes the sorted path and returns
    the oracle's exact counts. Without the fault the same data is counted by the index (verdict 1)."""
    ops.set_index_form(1)  # round 5's direct build (the slotted build has no scatter to guard)
    rng = np.random.default_rng(9 + fault)
    n = 1 << 21
    data = [(rng.random(n, dtype=np.float32), _labels(rng, n, p)) for p in (0.01, 0.001)]
    for s, y in data:
        e = coracle.auc_counts(y.astype(np.int64), s)
        ts, ty = T(s, dev), T(y, dev)
        ops.set_direct_fault(0)
        rec = ops.auc_eval_enqueue(ts, ty, 0, 1).cpu().tolist()
        assert rec[7] == 1 and tuple(rec[:2]) == (e["wins"], e["ties"]), rec
        ops.set_direct_fault(fault)
        rec = ops.auc_eval_enqueue(ts, ty, 0, 1).cpu().tolist()
        assert rec[7] == 2, (fault, rec)
        W, Tt, P, N, bad, other = ops.auc_eval_counts(ts, ty)
        assert (W, Tt, P, N, bad, other) == (e["wins"], e["ties"], e["P"], e["N"], 0, 0), fault
        ops.set_direct_fault(0)
        W, Tt, P, N, bad, other = ops.auc_eval_counts(ts, ty)
        assert (W, Tt, P, N) == (e["wins"], e["ties"], e["P"], e["N"])


@pytest.mark.parametrize("case", ["uniform", "ties", "cells_5_14", "cell_15", "p_over_half"])
def test_index_forms_agree_one_call(dev, ops, case):
    """The one-call evaluation (dauc_auc_eval_enqueue / _counts) with the count index built by round 5's
    direct build (form 1: count, blocks, scatter) and by round 6's slotted build (form 0, the
    product's): the same record, word for word, and the C oracle's counts. Cases: uniform scores;
    tie-heavy quantised scores; positives repeated 5..14 times in one cell (the secondary window and
    the tertiary run); a cell of 15 (both forms refuse the index: verdict 2, then the sorted path);
    more positives than negatives."""
    rng = np.random.default_rng({"uniform": 1, "ties": 2, "cells_5_14": 3, "cell_15": 4, "p_over_half": 5}[case])
    n = 1_000_003
    s = rng.random(n, dtype=np.float32)
    p = 0.6 if case == "p_over_half" else 0.02
    y = np.where(rng.random(n) < p, 1, -1).astype(np.int8)
    if case == "ties":
        s = (np.floor(s * 20000) / 20000).astype(np.float32)
    if case in ("cells_5_14", "cell_15"):
        s = (s * np.float32(0.25)).astype(np.float32)
        pos, neg = np.flatnonzero(y == 1), np.flatnonzero(y == -1)
        at = 0
        for j, m in enumerate((5, 8, 9, 14) if case == "cells_5_14" else (15,)):
            v = np.float32(0.3 + 0.1 * j)
            s[pos[at:at + m]] = v
            at += m
            s[neg[50 * j:50 * j + 9]] = v
            s[neg[50 * j + 9:50 * j + 12]] = np.nextafter(v, np.float32(1))
    e = coracle.auc_counts(y.astype(np.int64), s)
    ts, ty = T(s, dev), T(y, dev)
    recs = {}
    for form in (1, 0):
        ops.set_index_form(form)
        recs[form] = ops.auc_eval_enqueue(ts, ty, 0, 1).cpu().tolist()
        W, Tt, P, N, bad, other = ops.auc_eval_counts(ts, ty)
        assert (W, Tt, P, N, bad) == (e["wins"], e["ties"], e["P"], e["N"], 0), (case, form)
    assert recs[0] == recs[1], (case, recs)
    want = 2 if case in ("cell_15", "p_over_half") else 1
    assert recs[0][7] == want, (case, recs[0])


SHAPE_NMAX = 1 << 25


@pytest.fixture(scope="module")
def shape_data():
    """U(0,1) fp32 scores and int8 labels with 0.1 % positives, 2^25 of each (33.7 k positives: well
    inside the count index's 219,838); every shape case below is a prefix."""
    rng = np.random.default_rng(11)
    return rng.random(SHAPE_NMAX, dtype=np.float32), _labels(rng, SHAPE_NMAX, 0.001)


@pytest.mark.parametrize("n,label_offset", [((1 << 23) - 1, 0), (1 << 23, 0), ((1 << 25) - 1, 0), (1 << 25, 0),
                                            ((1 << 23) + 1, 1)])
def test_compaction_shapes_one_call(dev, shape_data, n, label_offset):
    """The product library's one-call evaluation at the sizes where the unordered compaction changes
    shape (auc_count.hip, compact_unordered): 256 threads x 8 label groups below 2^23 labels, 512 x 8
    from 2^23, 256 x 32 from 2^25 -- the smallest inputs that reach the 512-thread and the wide shape,
    so a launcher that pairs a shape with the wrong block size shows here. The last case hands over
    the labels as a [1:] view of a larger array: not 16-byte aligned, so the 512-thread shape runs its
    per-group bounds-checked label loads. (W, T, P, N) exact against the C oracle."""
    from distributedauc_amd import ops

    s, y = shape_data[0][:n], shape_data[1][:n]
    e = coracle.auc_counts(y.astype(np.int64), s)
    ty = T(np.concatenate([np.zeros(label_offset, np.int8), y]), dev)[label_offset:]
    assert ty.data_ptr() % 16 == label_offset
    W, Tt, P, N, bad, other = ops.auc_eval_counts(T(s, dev), ty)
    assert (W, Tt, P, N) == (e["wins"], e["ties"], e["P"], e["N"]), (n, label_offset)
