"""The sorted exact-AUC path where its tree search and its sort's scans run (csrc/auc_sort.hip,
csrc/radix_sort.hip), against the C oracle and numpy's sort: exact integers and keys throughout.

The LDS search tree counts only a table that neither the count index nor the distinct-key index takes:
more than 14,000 distinct keys, and in the labeled call's automatic mode also more than 219,838 keys.
Every table here is spread fp32 scores with far more distinct keys than that (asserted on the CPU
before any GPU call, with the limit read from the plan), so the tree kernels count in mode 0 as in
mode 1. The sizes come from tests/sort_cases.py, whose plan words tests/test_sort_plan_host.py pins
without a GPU: every K template of query_count_kernel / query_labeled_kernel (K = 0: two walks and
binary searches in global memory), the tree at its cap of 40,000 splitters, every tree height, the
three-launch scan of the sort and the run loop of its block-sum scan.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import coracle
from sort_cases import HEIGHT_PLANS, LABELED_MS, ROUTE_M, SORT_PATTERN_NS, SORT_PLANS, UNLABELED_MS, plan

pytestmark = pytest.mark.gpu

RUN_LONG, RUN_K = np.float32(0.25), np.float32(-0.375)  # planted 3k + 5 times and exactly k times


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


def keys_of(v):
    """The order-preserving uint32 keys of fp32 scores (-0 and +0 on one key), as test_radix_sort_keys computes them."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(v == 0, np.uint32(0x80000000), np.where(u >> 31, ~u, u | np.uint32(0x80000000))).astype(np.uint32)


# ---- (a) tree data ----------------------------------------------------------------------------------

def tree_data(M, L, seed, n_split=1000):
    """A table of M keys and L queries for it.

    Table: spread scores of both signs in [-1, 1); one value 3k + 5 times and one exactly k times (runs
    of equal keys across bucket boundaries, k the plan's bucket size); 50 copies each of -0.0 and +0.0
    (planted where the table has room for them). Queries: about 70 % spread over [-1.05, 1.05) (some
    below the table's minimum, some above its maximum), 20 % the table's own values, the first n_split
    splitters sorted[::k], the largest splitter sorted[(S - 1) k] and the largest key, each also one
    float up and one down, and the planted values and +-0. Returns (table, queries, distinct keys)."""
    p = plan(M)
    k, S = p["k"], p["S"]
    rng = np.random.default_rng(seed)
    table = rng.random(M, dtype=np.float32) * np.float32(2) - np.float32(1)
    runs = ((RUN_LONG, 3 * k + 5), (RUN_K, k), (np.float32(-0.0), 50), (np.float32(0.0), 50))
    if M >= 2 * sum(c for _, c in runs):
        at = rng.choice(M, sum(c for _, c in runs), replace=False)
        for v, c in runs:
            table[at[:c]] = v
            at = at[c:]
    srt = np.sort(table)
    sp = np.concatenate([srt[::k][:n_split], srt[(S - 1) * k:(S - 1) * k + 1], srt[-1:]])
    up, down = np.float32(np.inf), np.float32(-np.inf)
    sp = np.concatenate([sp, np.nextafter(sp, up), np.nextafter(sp, down)]).astype(np.float32)
    extra = np.array([RUN_LONG, RUN_K, 0.0, -0.0], np.float32)
    n_own = L // 5
    n_spread = L - n_own - sp.size - extra.size
    assert n_spread >= 0, (M, L, sp.size)
    spread = rng.random(n_spread, dtype=np.float32) * np.float32(2.1) - np.float32(1.05)
    q = np.concatenate([spread, rng.choice(table, n_own), sp, extra]).astype(np.float32)
    rng.shuffle(q)
    assert q.size == L and np.isfinite(q).all()
    return table, q, int(np.unique(keys_of(table)).size)


def _assert_tree_counts(M, distinct):
    """More distinct keys than the distinct-key index holds: the tree counts in every mode."""
    assert distinct > plan(M)["dk_max"], (M, distinct)


def _oracle(pos, neg):
    y = np.concatenate([np.ones(pos.size, np.int64), -np.ones(neg.size, np.int64)])
    e = coracle.auc_counts(y, np.concatenate([pos, neg]))
    return e["wins"], e["ties"]


def _unlabeled(ops, dev, pos, neg, modes, ref, what):
    tp, tn = T(pos, dev), T(neg, dev)
    for m in modes:
        ops.set_search_mode(m)
        wt = torch.zeros(2, dtype=torch.int64, device=dev)
        ops.auc_counts_sorted(tp, tn, wt)
        assert tuple(wt.cpu().tolist()) == ref, (what, m, wt.cpu().tolist(), ref)


# ---- (b) unlabeled ------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", UNLABELED_MS)
def test_tree_unlabeled_every_bucket_size(dev, ops, M):
    """query_count_kernel<K, TABLE_POS> at every K (1, 2, 4, 8, 16, 32 and 0), the table as the positives
    and as the negatives, in modes 0 (the distinct-key index refuses the table on the device) and 1;
    S at its cap at 1,280,000; at k = 64 a one-key and a full last bucket, and the queries also from
    an address that is not 16-byte aligned (the scalar query loop). (W, T) against the C oracle."""
    L = M + M // 20
    table, q, distinct = tree_data(M, L, seed=M)
    _assert_tree_counts(M, distinct)
    k = plan(M)["k"]
    for table_pos in (True, False):
        pos, neg = (table, q) if table_pos else (q, table)
        ref = _oracle(pos, neg)
        _unlabeled(ops, dev, pos, neg, (0, 1), ref, (M, table_pos))
        if k == 64:
            tq = T(np.concatenate([np.zeros(1, np.float32), q]), dev)[1:]
            assert tq.data_ptr() % 16 == 4 and tq.is_contiguous()
            tt = T(table, dev)
            for m in (0, 1):
                ops.set_search_mode(m)
                wt = torch.zeros(2, dtype=torch.int64, device=dev)
                ops.auc_counts_sorted(*((tt, tq) if table_pos else (tq, tt)), wt)
                assert tuple(wt.cpu().tolist()) == ref, (M, table_pos, m, "unaligned")


@pytest.mark.parametrize("S", list(HEIGHT_PLANS))
def test_tree_height_boundaries(dev, ops, S):
    """k = 1 tables of 5^h - 1 and 5^h keys, h = 1 .. 6 (and one key): the last table of every tree
    height and the first of the next, walked (mode 1) with the table on either side, against the brute
    force pair count. The queries are one more than the table where fewer would make them the table
    (P * N stays within 10^7 up to 3,125 keys; 2.4 * 10^8 pairs, under a second, at 15,624 and 15,625)."""
    M = S
    L = max(M + 1, min(4000, 10 ** 7 // M))
    table, q, _ = tree_data(M, L, seed=77 + S, n_split=min(1000, L // 8))
    for table_pos in (True, False):
        pos, neg = (table, q) if table_pos else (q, table)
        _unlabeled(ops, dev, pos, neg, (1,), coracle.pair_count_bruteforce(pos, neg), (S, table_pos))


# ---- (c) labeled --------------------------------------------------------------------------------------

N_NEG = 300_000
_labeled_cache: dict = {}


def _labeled_case(M):
    """Scores and int8 labels: the table's M positives and N_NEG queries (labels -1, some 0) in one
    shuffled array; the oracle's (W, T) over the whole range and a ragged one. Computed once per M."""
    if M not in _labeled_cache:
        table, q, distinct = tree_data(M, N_NEG, seed=3 * M)
        rng = np.random.default_rng(M + 1)
        yq = np.where(rng.random(q.size) < 0.05, 0, -1).astype(np.int8)
        perm = rng.permutation(M + q.size)
        s = np.concatenate([table, q])[perm]
        y = np.concatenate([np.ones(M, np.int8), yq])[perm]
        n = s.size
        refs = {}
        for begin, end in ((0, n), (3, n - 5)):
            neg = s[begin:end][y[begin:end] != 1]
            refs[(begin, end)] = _oracle(s[y == 1], neg)
        _labeled_cache.clear()  # one case at a time: the 5 M case is 50 MB
        _labeled_cache[M] = (s, y, refs, distinct)
    return _labeled_cache[M]


@pytest.mark.parametrize("M,ldtype", [(M, t) for M in LABELED_MS[:3] for t in (np.int8, np.int32, np.int64)]
                         + [(LABELED_MS[3], np.int8)])
def test_tree_labeled(dev, ops, M, ldtype):
    """query_labeled_kernel<K, LT> at K = 32 (640,001 positives), with the tree at its cap (1,280,000:
    40,000 splitters, 160,128 bytes of LDS) and at K = 0 (1,280,001: k = 64; 5,120,001: k = 256), per
    label type, in all three modes (each reaches the tree: the table is past the count index's size and
    the distinct-key index's key count), over the whole range and a ragged one. About 300,000 queries,
    some with label 0. (W, T) against the C oracle over the positives and the slice's non-positives."""
    s, y, refs, distinct = _labeled_case(M)
    _assert_tree_counts(M, distinct)
    ts, ty, tpos = T(s, dev), T(y.astype(ldtype), dev), T(s[y == 1], dev)
    for m in (0, 1, 2):
        ops.set_search_mode(m)
        for (begin, end), ref in refs.items():
            wt = torch.zeros(3, dtype=torch.int64, device=dev)
            ops.auc_counts_sorted_labeled(tpos, ts, ty, begin, end, wt, nonfinite=wt[2:])
            assert tuple(wt[:2].cpu().tolist()) == ref, (M, m, begin, end, wt.cpu().tolist(), ref)
            assert int(wt[2]) == 0, (M, m, begin, end)


# ---- (d) the product's routes -------------------------------------------------------------------------

@pytest.mark.parametrize("table_pos", [True, False])
def test_tree_product_routes(dev, table_pos):
    """The product library's one-call evaluation of 2.7 M spread scores whose smaller class has
    1,300,000 (k = 64): fewer positives than negatives -- the labeled tree kernel, K = 0 -- and fewer
    negatives than positives -- the split, then the unlabeled kernel with the negatives as the table,
    K = 0. (W, T, P, N) against the C oracle."""
    from distributedauc_amd import ops

    M, L = ROUTE_M, ROUTE_M + 100_000
    table, q, distinct = tree_data(M, L, seed=5)
    _assert_tree_counts(M, distinct)
    rng = np.random.default_rng(6)
    perm = rng.permutation(M + L)
    s = np.concatenate([table, q])[perm]
    y = np.concatenate([np.full(M, 1 if table_pos else -1, np.int8), np.full(L, -1 if table_pos else 1, np.int8)])[perm]
    e = coracle.auc_counts(y.astype(np.int64), s)
    assert (e["P"], e["N"]) == ((M, L) if table_pos else (L, M))
    got = ops.auc_eval_counts(T(s, dev), T(y, dev))
    assert got == (e["wins"], e["ties"], e["P"], e["N"], 0, 0), (table_pos, got, e)


# ---- (e) the sort, key for key ------------------------------------------------------------------------

def _finite_patterns(rng, n):
    """Random 32-bit patterns with the exponent 0xFF removed: finite floats of every sign, exponent and
    mantissa byte (subnormals and zeros among them)."""
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    b[(b >> 23) & 0xff == 0xff] &= np.uint32(~(1 << 23) & 0xffffffff)
    return b.view(np.float32)


def _floats_of_keys(k):
    k = k.astype(np.uint32)
    return np.where(k >> 31, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def _sort_and_check(dev, v, what, dirty=True):
    from distributedauc_amd import _lib, ops

    if dirty:  # whatever the workspace held before must not matter
        ops.workspaces.get(dev, "sort", int(_lib.load().dauc_sort_workspace_size(v.size))).fill_(0xA5)
    assert np.isfinite(v).all(), what
    got = ops.sort_keys(T(v, dev)).cpu().numpy().view(np.uint32)
    want = np.sort(keys_of(v))
    assert got.shape == want.shape and np.array_equal(got, want), (what, int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize("n", list(SORT_PLANS))
def test_sort_keys_every_scan_form(dev, n):
    """dauc_sort_keys key for key against numpy's sort of the keys, on keys that use every value of every
    digit, in a workspace filled with 0xA5: one key, sizes around a wave, a scatter wave and a tile, the
    last sort whose scatter scans the histogram itself (256 tiles), the first with the three scan
    launches (257 tiles, a partial last scan block), 1024 tiles, and 4097 tiles (1025 block sums: two
    per thread of scan_sums_kernel, with a short last run)."""
    v = _finite_patterns(np.random.default_rng(n), n)
    if n >= 524_288:
        k = keys_of(v)
        assert all(np.unique((k >> s) & 0xff).size == 256 for s in (0, 8, 16, 24))
    _sort_and_check(dev, v, n)


@pytest.mark.parametrize("n", SORT_PATTERN_NS)
def test_sort_keys_structured_inputs(dev, n):
    """All keys equal, two values alternating, ascending and descending input, and keys that differ in
    exactly one byte (three passes move nothing, one moves everything), once per byte; in the fused
    form (10,241 keys) and with scan launches (524,289)."""
    rng = np.random.default_rng(1000 + n)
    _sort_and_check(dev, np.full(n, -1.5, np.float32), (n, "equal"))
    alt = np.empty(n, np.float32)
    alt[0::2], alt[1::2] = 3.0e38, -1e-40
    _sort_and_check(dev, alt, (n, "alternating"))
    asc = np.sort(_finite_patterns(rng, n))
    _sort_and_check(dev, asc, (n, "ascending"))
    _sort_and_check(dev, asc[::-1].copy(), (n, "descending"))
    base = np.uint32(0xBF404040)
    for byte in range(4):
        lo, hi = (1, 255) if byte == 3 else (0, 256)  # top byte 0x00 / 0xFF with this base: exponent 0xFF
        r = rng.integers(lo, hi, n, dtype=np.uint64).astype(np.uint32)
        keys = (base & np.uint32(~(0xff << (8 * byte)) & 0xffffffff)) | (r << np.uint32(8 * byte))
        v = _floats_of_keys(keys)
        assert np.array_equal(keys_of(v), keys)
        _sort_and_check(dev, v, (n, "byte", byte))


def test_sort_keys_small_after_large_in_one_workspace(dev):
    """524,289 keys (scan launches), then 2049 keys (fused) in the same cached workspace, which still
    holds the first sort's keys, histogram and block sums."""
    from distributedauc_amd import _lib, ops

    rng = np.random.default_rng(9)
    _sort_and_check(dev, _finite_patterns(rng, 524_289), "large")
    ws = ops.workspaces.get(dev, "sort", int(_lib.load().dauc_sort_workspace_size(2049)))
    assert ws.numel() >= int(_lib.load().dauc_sort_workspace_size(524_289))  # the large sort's workspace, reused
    _sort_and_check(dev, _finite_patterns(rng, 2049), "small", dirty=False)
