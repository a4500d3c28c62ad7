// Exact AUC by sorting: LSD radix sort of the SMALLER class's order-preserving keys,
// then every score of the larger class is located in it with an LDS-resident search
// tree. O(M log M + L log M) work (M = min(P, N), L = max(P, N)) instead of the pair
// count's O(P*N); the counts are the same integers (W, T).
//
// Reference: imagenet/main.py:79-81 -> sklearn roc_curve/auc, whose
// _binary_clf_curve (sklearn/metrics/_ranking.py:826-908) also sorts the scores
// (a stable mergesort on the CPU, :886). SURVEY §8f row 1.
//
// Keys: an fp32 score maps to a uint32 that orders like the float, with -0 and
// +0 on one key (fp32 equality semantics): k = bits ^ (sign ? 0xffffffff : 0x80000000).
//
// Sort: radix_sort.hip (radix_sort_keys).
// Search: every k-th sorted key (k a power of two, at most kMaxSplit splitters) is a key of a
//   5-ary search tree of 16-byte nodes (4 keys, one ds_read_b128 per level) that every query
//   workgroup copies into LDS; each level stores only its real prefix plus one all-padding
//   node. A query x, clamped below the largest splitter, walks <= 7 levels (p <- 5p + #(node
//   keys <= x)), then one 16-byte load of its k-key bucket from the (L2-resident) sorted table
//   finishes upper_bound and lower_bound. The queries are streamed once with float4 loads;
//   per-block integer sums, one 64-bit atomic each.
//   table = positives: W += M - ub(x), T += ub - lb;  table = negatives: W += lb(x), T += ub - lb.
// The count index built straight from the unsorted positives and the query pass through it -- the
// product's hot path -- are count_index.hip and count_query.hip; the count index behind the sort
// (ci_*_kernel, prepare_count) and the distinct-key index of tie-heavy tables (dk_*_kernel) are here.
// Entry points: dauc_auc_counts_sorted, dauc_auc_counts_sorted_labeled, and counts_sorted_labeled
// for the evaluation's verdict-2 fallback (auc_eval.hip).

#include <type_traits>

#include "auc_eval_internal.h"
#include "auc_query.h"
#ifdef DAUC_TUNING
#include "dauc_tuning.h"
#endif

namespace dauc {
namespace {

// the distinct-key index of tie-heavy tables (dk_*_kernel below)
constexpr int kDkUse = 0, kDkD = 1;              // meta words; kCiOk, kCiCells, kCiBlocks: the plan's
constexpr int kDkScanThreads = 1024;
// tiles each thread of the one-workgroup dk_scan_kernel takes (2 or more past 1,048,576 table keys)
__host__ __device__ inline int64_t dk_scan_run(int64_t ntiles) { return (ntiles + kDkScanThreads - 1) / kDkScanThreads; }

__device__ __forceinline__ bool dk_ci_in_use(const unsigned* __restrict__ ci_meta) {
    return ci_meta != nullptr && count_index_in_use(ci_meta);
}

// ---- search ---------------------------------------------------------------------------

// The S splitters are the in-order keys of a perfect 5-ary search tree of height H (5^(H-1) <= S
// + 1 <= 5^H): a node is 4 keys (16 B, one ds_read_b128) and routes a query to child
// #(keys <= x), so a walk is H <= 7 dependent LDS reads (a binary tree needs ~16). Key i of node
// j on level d has in-order rank (5j + i + 1) * 5^(H-1-d) - 1; keys of rank >= S are padding
// (+inf). The nodes holding at least one real key form a prefix of every level (n_d nodes),
// stored level after level and followed by ONE all-padding node: a walk at position p of level
// d reads node off_d + min(p, n_d), and p <- 5p + #(node keys <= x); after H levels p =
// #splitters <= x. The sorted table is padded with kPadKey to a whole number of buckets.
constexpr int kTreeArity = 5;  // 4-key nodes, one ds_read_b128 (3-ary 8-byte nodes measured the same)
constexpr int kNodeKeys = kTreeArity - 1;
constexpr int kMaxTreeH = 7;  // 5^7 - 1 >= kMaxSplit
static_assert(kMaxSplit <= 78124, "tree height bound");

struct TreeGeom {
    int S, H;
    int nd[kMaxTreeH];   // stored real nodes of level d
    int off[kMaxTreeH];  // first node of level d
    int nodes;           // total stored nodes (incl. the per-level padding nodes)
};

// (round 2 measured the tree's top levels held in SGPRs instead of LDS: no faster)
struct TopKeys {
    unsigned last;  // the largest splitter (a finite score's key, so >= 0x007fffff > 0)
};

TreeGeom tree_geom(int S) {
    TreeGeom g{};
    g.S = S;
    int64_t pw = 1;
    g.H = 0;
    while (pw * kTreeArity - 1 < S) {
        pw *= kTreeArity;
        ++g.H;
    }
    ++g.H;  // A^(H-1) <= S + 1 <= A^H
    int off = 0;
    int64_t div = pw;  // A^(H-1-d)
    for (int d = 0; d < g.H; ++d) {
        const int64_t t = S / div;
        g.nd[d] = static_cast<int>((t + kTreeArity - 1) / kTreeArity);  // j with A j + 1 <= t
        g.off[d] = off;
        off += g.nd[d] + 1;
        div /= kTreeArity;
    }
    g.nodes = off;
    return g;
}

// The search plan of a table of M keys, from M alone: prepare_table builds the tree from it and both
// query launchers launch from it (the tuning build's dauc_sort_table_plan reports it).
struct TablePlan {
    int k;        // keys per bucket: the smallest power of two with at most kMaxSplit splitters
    int S;        // splitters = buckets
    int K;        // the query kernels' template: k where a bucket is read whole (k <= 32), else 0
    int64_t pad;  // kPadKey keys written past M to fill the last bucket (k <= 32; larger buckets are
                  // binary-searched with bounds: k - 1 < 64 keys of slack in the sort workspace)
    TreeGeom g;
    size_t lds;   // the query kernels' dynamic LDS: the stored tree
};

TablePlan table_plan(int64_t M) {
    TablePlan p{};
    p.k = 1;
    while ((M + p.k - 1) / p.k > kMaxSplit) p.k *= 2;
    p.S = static_cast<int>((M + p.k - 1) / p.k);
    p.K = p.k <= 32 ? p.k : 0;
    p.pad = p.K ? int64_t(p.S) * p.k - M : 0;
    p.g = tree_geom(p.S);
    p.lds = size_t(p.g.nodes) * sizeof(TreeNode);
    return p;
}

// the largest table the count index is built for (1.5 keys per cell at most)
constexpr int64_t kCiMaxTable = 3 * int64_t(kCiMaxCells) / 2;

__device__ __forceinline__ void store_node(uint4* t, int64_t c, const unsigned (&k)[4]) { t[c] = uint4{k[0], k[1], k[2], k[3]}; }

__global__ __launch_bounds__(256) void build_tree_kernel(unsigned* __restrict__ sorted, int64_t M, int64_t pad, int k,
                                                         TreeGeom g, TreeNode* __restrict__ tree,
                                                         unsigned* __restrict__ ci_first, int n_first) {
    const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (c < g.nodes) {
        int d = 0;
        while (d + 1 < g.H && c >= g.off[d + 1]) ++d;
        const int j = static_cast<int>(c) - g.off[d];
        int64_t pw = 1;
        for (int e = d + 1; e < g.H; ++e) pw *= kTreeArity;
        unsigned key[4] = {kPadKey, kPadKey, kPadKey, kPadKey};
#pragma unroll
        for (int i = 0; i < kNodeKeys; ++i) {
            const int64_t r = (int64_t(kTreeArity) * j + i + 1) * pw - 1;  // in-order rank
            key[i] = (j < g.nd[d] && r < g.S) ? sorted[r * k] : kPadKey;
        }
        store_node(tree, c, key);
    }
    // keys M .. S*k of the last bucket (and at least 8 past M, for the count index's windows):
    // +inf, so bucket compares need no bounds
    if (c < pad || c < 8) sorted[M + c] = kPadKey;
    if (c < n_first) ci_first[c] = static_cast<unsigned>(M);  // count index: "no key in this bucket"
}

// p <- 5 p + #(node keys <= x): the compares' carries feed the adds (a carry-free form with
// saturating subtracts, 12 VALU instead of 8, measured 5 % slower in round 2)
__device__ __forceinline__ unsigned tree_step(unsigned p, uint4 n, unsigned x) {
    unsigned r = p * 5u;
    asm("v_cmp_le_u32_e32 vcc, %1, %5\n\t"
        "v_addc_co_u32_e32 %0, vcc, 0, %0, vcc\n\t"
        "v_cmp_le_u32_e32 vcc, %2, %5\n\t"
        "v_addc_co_u32_e32 %0, vcc, 0, %0, vcc\n\t"
        "v_cmp_le_u32_e32 vcc, %3, %5\n\t"
        "v_addc_co_u32_e32 %0, vcc, 0, %0, vcc\n\t"
        "v_cmp_le_u32_e32 vcc, %4, %5\n\t"
        "v_addc_co_u32_e32 %0, vcc, 0, %0, vcc"
        : "+v"(r)
        : "v"(n.x), "v"(n.y), "v"(n.z), "v"(n.w), "v"(x)
        : "vcc");
    return r;
}

// Q walks of the tree in lockstep: p[q] ends as #splitters <= x[q]. The level geometry is
// wave-uniform (kernel arguments, scalar registers).
template <int Q>
__device__ __forceinline__ void tree_walk(const unsigned (&x)[Q], unsigned (&p)[Q], const TreeNode* __restrict__ tree,
                                          const TreeGeom& g, const TopKeys& top) {
#pragma unroll
    for (int q = 0; q < Q; ++q) p[q] = 0;
    // A walk for x below the largest splitter only visits stored nodes: its node at level d is
    // floor(r / 5^(H-d)) for r = #splitters <= x <= S - 1, at most the level's one padding node
    // (n_d). So x is clamped below the largest splitter (no per-level index clamp) and the
    // queries at or above it get p = S.
    unsigned xc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) xc[q] = x[q] < top.last ? x[q] : top.last - 1u;
#pragma unroll
    for (int d = 0; d < kMaxTreeH; ++d) {
        if (d < g.H) {
            const unsigned off = static_cast<unsigned>(g.off[d]);
            TreeNode v[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) v[q] = tree[off + p[q]];
#pragma unroll
            for (int q = 0; q < Q; ++q) p[q] = tree_step(p[q], v[q], xc[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) p[q] = x[q] < top.last ? p[q] : static_cast<unsigned>(g.S);
}

// #keys of bucket b (keys sorted[b*k .. min(b*k + k, M))) that are <= x, and that are < x;
// first = the bucket's smallest key (its splitter)
template <int K>
__device__ __forceinline__ void bucket_counts(const unsigned* __restrict__ sorted, int64_t M, int64_t b,
                                              unsigned x, int& le, int& lt, unsigned& first) {
    const int64_t base = b * K;
    unsigned v[K];
    if constexpr (K >= 4) {
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            const uint4 u = reinterpret_cast<const uint4*>(sorted + base)[q];
            v[4 * q] = u.x;
            v[4 * q + 1] = u.y;
            v[4 * q + 2] = u.z;
            v[4 * q + 3] = u.w;
        }
    } else if constexpr (K == 2) {
        const uint2 u = *reinterpret_cast<const uint2*>(sorted + base);
        v[0] = u.x;
        v[1] = u.y;
    } else {
        v[0] = sorted[base];
    }
    first = v[0];
    le = 0;
    lt = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {  // the tail bucket is padded with kPadKey (> every finite key)
        le += v[j] <= x;
        lt += v[j] < x;
    }
}

// #keys in sorted[lo, hi) that are < x (LT) or <= x (!LT): binary search in global memory
template <bool LT>
__device__ __forceinline__ int64_t count_below(const unsigned* __restrict__ a, int64_t lo, int64_t hi, unsigned x) {
    int64_t len = hi - lo, base = lo;
    while (len > 0) {
        const int64_t half = len >> 1;
        const unsigned v = a[base + half];
        if (LT ? v < x : v <= x) {
            base += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return base - lo;
}

// One query (K = 0: buckets of k > 32 keys, finished by binary searches in global memory).
template <int K, bool TABLE_POS>
__device__ __forceinline__ void count_query(unsigned x, const TreeNode* __restrict__ tree, const TreeGeom& g,
                                            const TopKeys& top, int k,
                                            const unsigned* __restrict__ sorted, int64_t M,
                                            unsigned long long& w, unsigned long long& t) {
    // splitters <= x (walk 0) and < x = <= x - 1 (walk 1; finite keys are >= 0x00800000, so
    // x - 1 never wraps)
    int64_t ub = 0, lb = 0;
    if constexpr (K <= 1) {
        const unsigned xs[2] = {x, x - 1u};
        unsigned i[2];
        tree_walk<2>(xs, i, tree, g, top);
        const int64_t su = i[0], sl = i[1];
        if constexpr (K == 1) {
            ub = su;
            lb = sl;
        } else {
            if (su > 0) {
                const int64_t b0 = (su - 1) * k, b1 = (b0 + k < M) ? b0 + k : M;
                ub = b0 + count_below<false>(sorted, b0, b1, x);
            }
            if (sl > 0) {
                const int64_t b0 = (sl - 1) * k, b1 = (b0 + k < M) ? b0 + k : M;
                lb = b0 + count_below<true>(sorted, b0, b1, x);
            }
        }
    } else {
        // one walk for x; the walk for x - 1 is needed only when the last splitter <= x
        // equals x (a run of x may then start in an earlier bucket)
        const unsigned xs[1] = {x};
        unsigned i[1];
        tree_walk<1>(xs, i, tree, g, top);
        const int64_t su = i[0];
        if (su > 0) {
            int le = 0, lt = 0;
            unsigned first = 0;
            bucket_counts<K>(sorted, M, su - 1, x, le, lt, first);
            ub = (su - 1) * K + le;
            if (first < x) {
                lb = (su - 1) * K + lt;
            } else {
                const unsigned xm[1] = {x - 1u};
                tree_walk<1>(xm, i, tree, g, top);
                const int64_t sl = i[0];
                if (sl > 0) {
                    bucket_counts<K>(sorted, M, sl - 1, x, le, lt, first);
                    lb = (sl - 1) * K + lt;
                }
            }
        }
    }
    w += TABLE_POS ? static_cast<unsigned long long>(M - ub) : static_cast<unsigned long long>(lb);
    t += static_cast<unsigned long long>(ub - lb);
}

// Q queries walked in lockstep (K = 1 .. 32): Q independent chains of LDS reads (and then Q
// bucket loads) in flight per lane. use[q] = false: the slot is walked but not counted.
template <int K>
constexpr int lockstep_queries() {
    return K <= 8 ? 4 : (K == 16 ? 2 : 1);
}

template <int K, int Q, bool TABLE_POS>
__device__ __forceinline__ void count_queries(const unsigned (&x)[Q], const bool (&use)[Q],
                                              const TreeNode* __restrict__ tree, const TreeGeom& g,
                                              const TopKeys& top,
                                              const unsigned* __restrict__ sorted, int64_t M,
                                              unsigned long long& w, unsigned long long& t) {
    static_assert(K >= 1 && K <= 32, "bucketed lockstep walk");
    if constexpr (K == 1) {
        // the tree holds every key: splitters <= x and <= x - 1 directly
        unsigned xs[2 * Q], i[2 * Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            xs[q] = x[q];
            xs[Q + q] = x[q] - 1u;
        }
        tree_walk<2 * Q>(xs, i, tree, g, top);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (!use[q]) continue;
            const int64_t ub = i[q], lb = i[Q + q];
            w += TABLE_POS ? static_cast<unsigned long long>(M - ub) : static_cast<unsigned long long>(lb);
            t += static_cast<unsigned long long>(ub - lb);
        }
    } else {
        unsigned su[Q];
        tree_walk<Q>(x, su, tree, g, top);
        // every bucket load issued before any is examined (su = 0: bucket 0 is read, unused)
        int le[Q], lt[Q];
        unsigned first[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) bucket_counts<K>(sorted, M, su[q] ? su[q] - 1u : 0u, x[q], le[q], lt[q], first[q]);
        // 32-bit and branch-free: lb below is exact unless the bucket starts with x itself (then
        // a run of x may begin in an earlier bucket); those rare queries are fixed up after
        // the Q queries' counts summed in 32 bits (Q * M < 2^32), one 64-bit add each
        bool slow = false;
        unsigned wl = 0u, tl = 0u;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const unsigned base = su[q] ? (su[q] - 1u) * static_cast<unsigned>(K) : 0u;
            const unsigned ub = su[q] ? base + static_cast<unsigned>(le[q]) : 0u;
            const unsigned lb = su[q] ? base + static_cast<unsigned>(lt[q]) : 0u;
            const unsigned wq = TABLE_POS ? static_cast<unsigned>(M) - ub : lb;
            wl += use[q] ? wq : 0u;
            tl += use[q] ? ub - lb : 0u;
            slow |= use[q] && su[q] != 0u && first[q] >= x[q];
        }
        w += wl;
        t += tl;
        if (slow) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                if (!(use[q] && su[q] != 0u && first[q] >= x[q])) continue;
                const unsigned xm[1] = {x[q] - 1u};
                unsigned j[1];
                tree_walk<1>(xm, j, tree, g, top);
                unsigned lb_true = 0u;
                if (j[0] != 0u) {
                    int le2 = 0, lt2 = 0;
                    unsigned f2 = 0;
                    bucket_counts<K>(sorted, M, j[0] - 1u, x[q], le2, lt2, f2);
                    lb_true = (j[0] - 1u) * static_cast<unsigned>(K) + static_cast<unsigned>(lt2);
                }
                const unsigned lb_fast = (su[q] - 1u) * static_cast<unsigned>(K);  // lt = 0: the bucket starts with x
                t += lb_fast - lb_true;                                             // ties: ub - lb_true
                if (!TABLE_POS) w -= lb_fast - lb_true;                             // wins: lb_true
            }
        }
    }
}

// Four keys (one float4 slot) with per-key use flags, through count_queries in groups of Q
// (K = 0, buckets > 32 keys finished in global memory: one key at a time).
template <int K, bool TABLE_POS>
__device__ __forceinline__ void count4(const unsigned (&x)[4], const bool (&use)[4], const TreeNode* __restrict__ tree,
                                       const TreeGeom& g, const TopKeys& top, int k, const unsigned* __restrict__ sorted, int64_t M,
                                       unsigned long long& w, unsigned long long& t) {
    if constexpr (K == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (use[q]) count_query<0, TABLE_POS>(x[q], tree, g, top, k, sorted, M, w, t);
    } else {
        constexpr int Q = lockstep_queries<K>();
#pragma unroll
        for (int b = 0; b < 4; b += Q) {
            unsigned xs[Q];
            bool us[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                xs[q] = x[b + q];
                us[q] = use[b + q];
            }
            count_queries<K, Q, TABLE_POS>(xs, us, tree, g, top, sorted, M, w, t);
        }
    }
}

// the top levels' keys, read once per workgroup with uniform (scalar) loads
__device__ __forceinline__ TopKeys load_top(const TreeNode* __restrict__ gtree, const TreeGeom& g,
                                           const unsigned* __restrict__ sorted, int k) {
    (void)gtree;
    (void)g;
    TopKeys t{};
    t.last = sorted[int64_t(g.S - 1) * k];
    return t;
}

template <int K, bool TABLE_POS>
__global__ __launch_bounds__(kQueryThreads) void query_count_kernel(const float* __restrict__ q, int64_t L,
                                                                   const TreeNode* __restrict__ gtree, TreeGeom g,
                                                                   int k, const unsigned* __restrict__ sorted,
                                                                   int64_t M, unsigned long long* __restrict__ out,
                                                                   const unsigned* __restrict__ dk_meta) {
    if (dk_meta != nullptr && dk_meta[kDkUse] != 0u) return;  // the distinct-key index counts instead
    extern __shared__ TreeNode tree[];
    for (int i = threadIdx.x; i < g.nodes; i += kQueryThreads) tree[i] = gtree[i];
    const TopKeys top = load_top(gtree, g, sorted, k);
    __syncthreads();
    unsigned long long w = 0, t = 0;
    const bool vec = (reinterpret_cast<uintptr_t>(q) & 15u) == 0;
    const int64_t nvec = vec ? L / 4 : 0;
    const int64_t stride = int64_t(gridDim.x) * kQueryThreads;
    const bool all[4] = {true, true, true, true};
    for (int64_t v = int64_t(blockIdx.x) * kQueryThreads + threadIdx.x; v < nvec; v += stride) {
        const f32x4 f = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q) + v);
        const unsigned x[4] = {key_of(f.x), key_of(f.y), key_of(f.z), key_of(f.w)};
        count4<K, TABLE_POS>(x, all, tree, g, top, k, sorted, M, w, t);
    }
    for (int64_t i = nvec * 4 + int64_t(blockIdx.x) * kQueryThreads + threadIdx.x; i < L; i += stride)
        count_query<K, TABLE_POS>(key_of(q[i]), tree, g, top, k, sorted, M, w, t);
    __shared__ unsigned long long red[2][kQueryThreads / kWave];
    w = wave_sum(w);
    t = wave_sum(t);
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    if (lane == 0) {
        red[0][wid] = w;
        red[1][wid] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long bw = 0, bt = 0;
        for (int i = 0; i < kQueryThreads / kWave; ++i) {
            bw += red[0][i];
            bt += red[1][i];
        }
        if (bw) atomicAdd(out + 0, bw);
        if (bt) atomicAdd(out + 1, bt);
    }
}

// Labeled queries: the negatives are not materialised. Elements [begin, end) of the full score
// and label arrays are streamed (float4 + 4 labels per slot); every element whose label is
// not +1 is a query against the sorted positives (table = positives).
template <typename LT>
__device__ __forceinline__ void label4(const LT* __restrict__ lab, int64_t i, bool full, int64_t end, bool (&neg)[4]) {
    if (full && sizeof(LT) == 1) {
        const char4 c = *reinterpret_cast<const char4*>(lab + i);
        neg[0] = c.x != 1;
        neg[1] = c.y != 1;
        neg[2] = c.z != 1;
        neg[3] = c.w != 1;
    } else if (full && sizeof(LT) == 4) {
        const int4 c = *reinterpret_cast<const int4*>(lab + i);
        neg[0] = c.x != 1;
        neg[1] = c.y != 1;
        neg[2] = c.z != 1;
        neg[3] = c.w != 1;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) neg[q] = i + q < end && lab[i + q] != LT(1);
    }
}

// search structure: 0 automatic (the count index where it holds the table, else the distinct-key
// index where it holds it, else the tree); the tuning build can force the tree
// (dauc_set_search_mode(1)) or the distinct-key index (2) to test them on any table
#ifdef DAUC_TUNING
int g_search_mode = 0;
#else
constexpr int g_search_mode = 0;
#endif

// ---- count index (the default search where it fits: dauc_set_search_mode 0) -----------------
//
// The tree's cost per query is its one 16-byte bucket gather from L2 plus 7 dependent LDS reads
// and ~140 VALU. The count index answers ~40 % of the queries with no gather at all and the rest
// with one, from 2 LDS reads and ~60 VALU:
//   * the key's top 11 bits pick a top bucket t (sign, exponent, 2 mantissa bits); its n_t table
//     keys get C_t = ceil(n_t * R) cells that split its 2^21 low key values evenly
//     (cell = off_t + mulhi(low21 << 11, C_t)), R = cells per table key (~1.1 for the 2^27 @
//     0.1 % table, so ~40 % of the cells -- and of the queries -- are empty);
//   * LDS holds {off_t, C_t} (2048 x 8 B) and, per block of 8 cells, {the table keys before the
//     block, the 8 cells' key counts as nibbles} (8 B): 1 B per cell, 146,559 cells;
//   * rank_lo = block base + the nibbles below the cell = #(table keys < the cell) and cnt = the
//     cell's nibble: the aligned 16-byte window of the sorted table at rank_lo & ~3 (loaded only
//     by the lanes with cnt > 0; a second one when the cell runs past it, a binary search past 8
//     keys) gives lb and ub by counting its keys < x and <= x -- keys before the cell are < x,
//     keys after it > x or the +inf padding; cnt = 0 gives lb = ub = rank_lo.
// The builder keeps the tree (a device word both query kernels read) when the table needs more
// than 1.5 keys per cell or a cell holds 15 or more keys (a nibble): clustered or tie-heavy
// tables, for which the tree's cost does not depend on the key distribution.

constexpr int kCiPlanThreads = 1024;

// first[t] = the first table index of top bucket t, for the buckets holding keys (first[] was set
// to M by build_tree_kernel)
__global__ __launch_bounds__(256) void ci_first_kernel(const unsigned* __restrict__ sorted, int64_t M,
                                                       unsigned* __restrict__ first) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= M) return;
    const unsigned t = sorted[i] >> kCiLowBits;
    if (i == 0 || (sorted[i - 1] >> kCiLowBits) != t) first[t] = static_cast<unsigned>(i);
}

// One workgroup: n_t from the suffix minima of first[] (thread i owns the buckets 2047 - 2i and
// 2046 - 2i: descending, so the suffix minima are prefix minima over the threads), the cells per
// bucket C_t = ceil(n_t * num / M), num = min(cells left after one per used bucket, 2 M) (so
// sum C_t fits), and the first cell of every bucket (prefix sum).
// (the body is shared with the distinct-key index's plan: dk_index_kernel; `first` and `l1` may be
// LDS or global, `max_cells` the cells the consumer's LDS holds)
__device__ __forceinline__ void ci_plan_body(int64_t M, const unsigned* first, uint2* l1, unsigned* __restrict__ meta,
                                             int64_t max_cells, unsigned* wtot, unsigned* incl_min, unsigned* totals,
                                             int per_key = 2) {
    static_assert(kCiTop == 2 * kCiPlanThreads, "two top buckets per thread");
    const unsigned m32 = static_cast<unsigned>(M);
    int tj[2];
    unsigned st[2], run = ~0u;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        tj[j] = kCiTop - 1 - 2 * static_cast<int>(threadIdx.x) - j;
        const unsigned f = first[tj[j]];
        run = f < run ? f : run;
        st[j] = run;
    }
    const unsigned incl = block_incl_scan1024<true>(run, wtot);
    incl_min[threadIdx.x] = incl;
    __syncthreads();
    unsigned n[2];
    {
        const unsigned above = threadIdx.x == 0 ? m32 : incl_min[threadIdx.x - 1];
        unsigned hi = above < m32 ? above : m32;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned s0 = st[j] < hi ? st[j] : hi;
            n[j] = hi - s0;
            hi = s0;
        }
    }
    const unsigned used = block_incl_scan1024<false>((n[0] != 0u) + (n[1] != 0u), wtot);
    if (threadIdx.x == kCiPlanThreads - 1) totals[0] = used;
    __syncthreads();
    const int64_t avail = max_cells - int64_t(totals[0]);
    const int64_t num = avail < per_key * M ? avail : per_key * M;
    unsigned C[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) C[j] = n[j] ? static_cast<unsigned>((int64_t(n[j]) * num + M - 1) / M) : 0u;
    const unsigned csum = C[0] + C[1];
    const unsigned incl_c = block_incl_scan1024<false>(csum, wtot);
    if (threadIdx.x == kCiPlanThreads - 1) totals[1] = incl_c;
    __syncthreads();
    const unsigned total = totals[1];
    unsigned upto = incl_c - csum;  // cells of the buckets above this thread's
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        upto += C[j];
        l1[tj[j]] = uint2{total - upto, C[j]};
    }
    if (threadIdx.x == 0) {
        meta[kCiOk] = (3 * num >= 2 * M && total <= static_cast<unsigned>(max_cells)) ? 1u : 0u;  // <= 1.5 keys/cell
        meta[kCiCells] = total;
        meta[kCiBlocks] = (total + 1 + kCiBlock - 1) / kCiBlock;
        meta[kCiSkew] = 0u;
    }
}

__global__ __launch_bounds__(kCiPlanThreads) void ci_plan_kernel(int64_t M, const unsigned* __restrict__ first,
                                                                 uint2* __restrict__ l1,
                                                                 unsigned* __restrict__ meta) {
    __shared__ unsigned wtot[kCiPlanThreads / kWave];
    __shared__ unsigned incl_min[kCiPlanThreads];
    __shared__ unsigned totals[2];
    ci_plan_body(M, first, l1, meta, kCiMaxCells, wtot, incl_min, totals);
}

// One thread per table index i in [0, M] (i = M: past the last cell): cells (c(i-1), c(i)] start at i
__global__ __launch_bounds__(256) void ci_cells_kernel(const unsigned* __restrict__ sorted, int64_t M,
                                                       const uint2* __restrict__ l1, const unsigned* __restrict__ meta,
                                                       unsigned* __restrict__ cstart) {
    if (meta[kCiOk] == 0u) return;
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i > M) return;
    auto cell = [&](int64_t j) -> int64_t {
        const unsigned key = sorted[j];
        return ci_cell(key, l1[key >> kCiLowBits]);
    };
    const int64_t ci = i < M ? cell(i) : int64_t(meta[kCiCells]) + 1;
    const int64_t cp = i > 0 ? cell(i - 1) : -1;
    for (int64_t c = cp + 1; c <= ci; ++c) cstart[c] = static_cast<unsigned>(i);
}

// One thread per block of 8 cells: the table keys before the block and the cells' counts as
// nibbles; a count of 15 or more marks the table skewed (the tree is used)
__global__ __launch_bounds__(256) void ci_blocks_kernel(const unsigned* __restrict__ cstart,
                                                        unsigned* __restrict__ meta, uint2* __restrict__ blk) {
    if (meta[kCiOk] == 0u) return;
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int nb = static_cast<int>(meta[kCiBlocks]);
    const int last = static_cast<int>(meta[kCiCells]) + 1;  // cstart[0 .. last] are written
    bool skew = false;
    if (b < nb) {
        unsigned w = 0;
        const int c0 = b * kCiBlock;
        unsigned prev = cstart[c0 < last ? c0 : last];
        const unsigned base = prev;
#pragma unroll
        for (int j = 0; j < kCiBlock; ++j) {
            const int c = c0 + j + 1;
            const unsigned nxt = cstart[c < last ? c : last];
            const unsigned cnt = nxt - prev;
            skew |= cnt >= 15u;
            w |= (cnt < 15u ? cnt : 15u) << (4 * j);
            prev = nxt;
        }
        blk[b] = uint2{base, w};
    }
    if (__ballot(skew) != 0ull && (threadIdx.x & (kWave - 1)) == 0) atomicOr(meta + kCiSkew, 1u);
}

// Every queried score is also checked to be finite (sklearn rejects NaN / inf scores,
// _ranking.py:868-869): nonfinite (nullable) += #queried non-finite scores. The negatives are
// never materialised, so this is the only pass that reads their scores. With a cell index
// built (meta != nullptr) the kernel returns at once unless the builder kept the tree.
template <int K, typename LT>
__global__ __launch_bounds__(kQueryThreads) void query_labeled_kernel(const float* __restrict__ s,
                                                                     const LT* __restrict__ lab, int64_t begin,
                                                                     int64_t end, const TreeNode* __restrict__ gtree,
                                                                     TreeGeom g, int k,
                                                                     const unsigned* __restrict__ sorted,
                                                                     int64_t M, unsigned long long* __restrict__ out,
                                                                     unsigned long long* __restrict__ nonfinite,
                                                                     const unsigned* __restrict__ meta,
                                                                     const unsigned* __restrict__ dk_meta) {
    // meta: the count index's builder verdict, dk_meta the distinct-key index's (the tree runs only
    // when neither is used)
    if (meta != nullptr && count_index_in_use(meta)) return;
    if (dk_meta != nullptr && dk_meta[kDkUse] != 0u) return;
    extern __shared__ TreeNode tree[];
    for (int i = threadIdx.x; i < g.nodes; i += kQueryThreads) tree[i] = gtree[i];
    const TopKeys top = load_top(gtree, g, sorted, k);
    __syncthreads();
    unsigned long long w = 0, t = 0;
    unsigned nf = 0;
    // scalar head up to a 4-element boundary, then float4 slots, then the scalar tail
    const int64_t a0 = (begin + 3) & ~int64_t(3);
    const int64_t head = a0 < end ? a0 : end;
    const int64_t stride = int64_t(gridDim.x) * kQueryThreads;
    const int64_t tid = int64_t(blockIdx.x) * kQueryThreads + threadIdx.x;
    for (int64_t i = begin + tid; i < head; i += stride) {
        if (lab[i] != LT(1)) {
            nf += !isfinite(s[i]);
            count_query<K, true>(key_of(s[i]), tree, g, top, k, sorted, M, w, t);
        }
    }
    const int64_t nvec = end > head ? (end - head) / 4 : 0;
    const bool aligned = (reinterpret_cast<uintptr_t>(s + head) & 15u) == 0 &&
                         (reinterpret_cast<uintptr_t>(lab + head) & (4 * sizeof(LT) - 1)) == 0;
    if (aligned) {
        // U float4 slots (4 queries each) per iteration, and the NEXT iteration's loads issued
        // before this one's walks: each walk is a chain of dependent LDS reads and a bucket load,
        // so without this the stream's HBM latency sits between every two iterations of a wave.
        // slots per iteration (prefetched one iteration ahead): register-bound
        constexpr int U = sizeof(LT) == 8 ? 2 : 4;
        f32x4 fc[U], fn[U];
        LabelWords<LT> lc[U], ln[U];
        auto load = [&](int64_t v0, f32x4 (&f)[U], LabelWords<LT> (&l)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t v = v0 + int64_t(u) * stride;
                if (v < nvec) {
                    const int64_t i = head + v * 4;
                    f[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s + i));
                    l[u].load(lab + i);
                } else {
                    f[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                    l[u].set_positive();  // past the end: no query
                }
            }
        };
        load(tid, fc, lc);
        for (int64_t v0 = tid; v0 < nvec; v0 += int64_t(U) * stride) {
            auto keys = [&](int u, unsigned (&x)[4], bool (&neg)[4]) {
                const float f[4] = {fc[u].x, fc[u].y, fc[u].z, fc[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    neg[q] = lc[u].not_positive(q);
                    x[q] = key_of(f[q]);
                    nf += neg[q] && !isfinite(f[q]);
                }
            };
            load(v0 + int64_t(U) * stride, fn, ln);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                bool neg[4];
                unsigned x[4];
                keys(u, x, neg);
                count4<K, true>(x, neg, tree, g, top, k, sorted, M, w, t);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                fc[u] = fn[u];
                lc[u] = ln[u];
            }
        }
    } else {
        for (int64_t v = tid; v < nvec; v += stride) {
            const int64_t i = head + v * 4;
            float f[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) f[q] = s[i + q];
            bool neg[4];
            label4(lab, i, false, end, neg);
            unsigned x[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x[q] = key_of(f[q]);
                nf += neg[q] && !isfinite(f[q]);
            }
            count4<K, true>(x, neg, tree, g, top, k, sorted, M, w, t);
        }
    }
    for (int64_t i = head + nvec * 4 + tid; i < end; i += stride) {
        if (lab[i] != LT(1)) {
            nf += !isfinite(s[i]);
            count_query<K, true>(key_of(s[i]), tree, g, top, k, sorted, M, w, t);
        }
    }
    __shared__ unsigned long long red[3][kQueryThreads / kWave];
    w = wave_sum(w);
    t = wave_sum(t);
    const unsigned long long nfw = wave_sum(static_cast<unsigned long long>(nf));
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    if (lane == 0) {
        red[0][wid] = w;
        red[1][wid] = t;
        red[2][wid] = nfw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long bw = 0, bt = 0, bn = 0;
        for (int i = 0; i < kQueryThreads / kWave; ++i) {
            bw += red[0][i];
            bt += red[1][i];
            bn += red[2][i];
        }
        if (bw) atomicAdd(out + 0, bw);
        if (bt) atomicAdd(out + 1, bt);
        if (bn && nonfinite) atomicAdd(nonfinite, bn);
    }
}

// ---- distinct-key index: tie-heavy tables (round 6) ---------------------------------------------
//
// The count index refuses a table whose cells hold 15+ keys. In practice that is a table of FEW
// DISTINCT values -- rounded scores, or the probabilities of a bf16 model (2^27 @ 0.1 % rounded to
// bf16: 134,447 positives on 1,329 values) -- whose equal keys no cell split can separate, and the
// tree it fell back to ran 1.05 ms at 2^27 (vs 0.47 ms for the index on spread scores). Its distinct
// keys, each with the number of table keys <= it (cum), answer a query exactly: #(table <= x) = the
// cum of the last distinct key <= x, #(== x) = that cum minus the previous one when the key IS x.
// Up to kDkMax distinct keys the whole structure fits the query's LDS: the count index's top-bucket
// plan over the distinct keys (l1, 16 KB), one word per cell {first distinct key, distinct keys in
// the cell} (2 cells per distinct key: <= 72 KB), and {key, cum} per distinct key (<= 64 KB). A
// query is then 3 dependent LDS reads -- l1, its cell word, the two entries at the cell's start --
// and no table gather at all; a cell of 2+ distinct keys (rare) adds a binary search over them.
// Built behind prepare_count from the sorted table in 4 small launches (mark, scan, write, index),
// every one deciding on the device (the count index in use: they return at once; more than kDkMax
// distinct keys: the tree runs), so the sorted path still needs no host readback. Round 6.
// the tile's 4 keys per thread and whether each is the LAST copy of its key (the table is +inf
// padded past M, and no finite key is +inf's)
__device__ __forceinline__ unsigned dk_flags(const unsigned* __restrict__ sorted, int64_t M, int64_t i0,
                                             unsigned (&k)[4]) {
    unsigned f = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = i0 + j < M ? sorted[i0 + j] : kPadKey;
    const unsigned nxt = i0 + 4 < M ? sorted[i0 + 4] : kPadKey;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned after = j < 3 ? k[j + 1] : nxt;
        f |= unsigned(i0 + j < M && k[j] != after) << j;
    }
    return f;
}

__global__ __launch_bounds__(kDkTile / 4) void dk_mark_kernel(const unsigned* __restrict__ sorted, int64_t M,
                                                              const unsigned* __restrict__ ci_meta,
                                                              unsigned* __restrict__ tcnt) {
    if (dk_ci_in_use(ci_meta)) return;
    __shared__ unsigned wsum[kDkTile / 4 / kWave];
    unsigned k[4];
    const unsigned f = dk_flags(sorted, M, int64_t(blockIdx.x) * kDkTile + 4 * int64_t(threadIdx.x), k);
    unsigned c = static_cast<unsigned>(__popc(f));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = c;
    __syncthreads();
    if (threadIdx.x == 0) tcnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup: the tiles' exclusive prefix in place, D, and whether the index is used
__global__ __launch_bounds__(kDkScanThreads) void dk_scan_kernel(const unsigned* __restrict__ ci_meta, DkWs dk,
                                                                 int64_t ntiles) {
    if (dk_ci_in_use(ci_meta)) return;
    __shared__ unsigned wtot[kDkScanThreads / kWave];
    const int64_t per = dk_scan_run(ntiles);
    const int64_t t0 = int64_t(threadIdx.x) * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    unsigned long long mine = 0;
    for (int64_t t = t0; t < t1; ++t) mine += dk.tcnt[t];
    // a thread's run past kDkMax: saturated (the total is then past it too, and nothing else is read)
    const unsigned m = mine > unsigned(kDkMax) ? unsigned(kDkMax) + 1u : static_cast<unsigned>(mine);
    const unsigned incl = block_incl_scan1024<false>(m, wtot);
    unsigned run = incl - m;
    for (int64_t t = t0; t < t1; ++t) {
        const unsigned c = dk.tcnt[t];
        dk.tcnt[t] = run;
        run += c;
    }
    if (threadIdx.x == kDkScanThreads - 1) {
        dk.meta[kDkD] = incl;
        dk.meta[kDkUse] = (incl >= 1u && incl <= static_cast<unsigned>(kDkMax)) ? 1u : 0u;
    }
}

// the distinct keys and their cums: the last copy of key kd[d] is table index cd[d] - 1
__global__ __launch_bounds__(kDkTile / 4) void dk_write_kernel(const unsigned* __restrict__ sorted, int64_t M,
                                                               const unsigned* __restrict__ ci_meta, DkWs dk) {
    if (dk_ci_in_use(ci_meta) || dk.meta[kDkUse] == 0u) return;
    __shared__ unsigned wsum[kDkTile / 4 / kWave];
    unsigned k[4];
    const int64_t i0 = int64_t(blockIdx.x) * kDkTile + 4 * int64_t(threadIdx.x);
    const unsigned f = dk_flags(sorted, M, i0, k);
    const unsigned c = static_cast<unsigned>(__popc(f));
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    unsigned incl = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned t = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += t;
    }
    if (lane == kWave - 1) wsum[wid] = incl;
    __syncthreads();
    unsigned d = dk.tcnt[blockIdx.x] + incl - c;
    for (int w = 0; w < wid; ++w) d += wsum[w];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if ((f >> j) & 1u) {
            dk.kd[d] = k[j];
            dk.cd[d] = static_cast<unsigned>(i0 + j + 1);
            ++d;
        }
    }
}

// one workgroup: the plan over the distinct keys (the count index's, ci_plan_body) and the first
// distinct key of every cell (cells (c(d-1), c(d)] start at d; d = D: up to the virtual last cell)
__global__ __launch_bounds__(kCiPlanThreads) void dk_index_kernel(const unsigned* __restrict__ ci_meta, DkWs dk) {
    if (dk_ci_in_use(ci_meta) || dk.meta[kDkUse] == 0u) return;
    __shared__ unsigned first[kCiTop];
    __shared__ uint2 l1[kCiTop];
    __shared__ unsigned wtot[kCiPlanThreads / kWave];
    __shared__ unsigned incl_min[kCiPlanThreads];
    __shared__ unsigned totals[2];
    const unsigned D = dk.meta[kDkD];
    for (int t = threadIdx.x; t < kCiTop; t += kCiPlanThreads) first[t] = D;
    __syncthreads();
    for (unsigned d = threadIdx.x; d < D; d += kCiPlanThreads) {
        const unsigned t = dk.kd[d] >> kCiLowBits;
        if (d == 0 || (dk.kd[d - 1] >> kCiLowBits) != t) first[t] = d;
    }
    __syncthreads();
    // up to 4 cells per distinct key while the LDS holds them (fewer cells of 2+ keys: less searching)
    ci_plan_body(D, first, l1, dk.meta, kDkMaxCells, wtot, incl_min, totals, 4);
    __syncthreads();
    for (int t = threadIdx.x; t < kCiTop; t += kCiPlanThreads) dk.l1[t] = l1[t];
    const unsigned cells = totals[1];
    auto cell = [&](unsigned d) -> int64_t {
        const unsigned key = dk.kd[d];
        return ci_cell(key, l1[key >> kCiLowBits]);
    };
    for (unsigned d = threadIdx.x; d <= D; d += kCiPlanThreads) {
        const int64_t cd = d < D ? cell(d) : int64_t(cells) + 1;
        const int64_t cp = d > 0 ? cell(d - 1) : -1;
        for (int64_t c = cp + 1; c <= cd; ++c) dk.cstart[c] = d;
    }
}

// Two LDS layouts of the index; the kernel built for the other one returns at once. Up to
// kDkSmall distinct keys (4 cells each) a cell word is 8 bytes {the cum before the cell, its first
// distinct key | its count << 16}: a query reads its cell word and, in a cell that holds keys, the
// cell's first {key, cum} -- 2 random LDS reads. Past it, to kDkMax, a cell word is 16 bits {first
// distinct key (14 bits), count saturated at 3} and a query reads the two entries at the cell's
// start -- 3 random reads. (The pass is bound by the LDS bank conflicts of those reads.)
constexpr int kDkSmall = 3200;
constexpr int kDkSmallCells = 4 * kDkSmall + kCiTop;

// the query kernels' LDS: l1, then {0, 0}, {key, cum} of every distinct key, {+inf, M} (read, never
// counted, past the last), then the cell words
template <bool SMALL>
struct DkLds {
    uint2* l1;
    uint2* kc;
    std::conditional_t<SMALL, uint2*, unsigned short*> cw;
};
template <bool SMALL>
__device__ __forceinline__ DkLds<SMALL> dk_load_lds(uint2* lds, const DkWs& dk, int64_t M) {
    constexpr int kMax = SMALL ? kDkSmall : kDkMax;
    using CW = std::conditional_t<SMALL, uint2*, unsigned short*>;
    DkLds<SMALL> r{lds, lds + kCiTop, reinterpret_cast<CW>(lds + kCiTop + kMax + 2)};
    const unsigned D = dk.meta[kDkD], cells = dk.meta[kCiCells];
    for (int i = threadIdx.x; i < kCiTop; i += blockDim.x) r.l1[i] = dk.l1[i];
    for (unsigned i = threadIdx.x; i < D + 2; i += blockDim.x)
        r.kc[i] = i == 0 ? uint2{0u, 0u}
                         : (i <= D ? uint2{dk.kd[i - 1], dk.cd[i - 1]} : uint2{kPadKey, static_cast<unsigned>(M)});
    for (unsigned c = threadIdx.x; c <= cells + (SMALL ? 0u : 1u); c += blockDim.x) {
        const unsigned a = dk.cstart[c], n = c <= cells ? dk.cstart[c + 1] - a : 0u;
        if constexpr (SMALL)
            r.cw[c] = uint2{a ? dk.cd[a - 1] : 0u, a | (n << 16)};
        else
            r.cw[c] = static_cast<unsigned short>(a | (min(n, 3u) << 14));
    }
    __syncthreads();
    return r;
}

// NQ queries of one lane: W += M - #(table <= x), T += #(table == x) for the queries in `use`
// (TABLE_POS false: the table is the negatives and the queries positives, W += #(table < x))
template <int NQ, bool TABLE_POS = true, bool SMALL = false>
__device__ __forceinline__ void dk_count(const unsigned (&x)[NQ], unsigned use, const DkLds<SMALL>& ld,
                                         unsigned long long M, unsigned long long& w, unsigned long long& t) {
    const uint2* kc = ld.kc;
    unsigned s0[NQ], n[NQ], cb[NQ], c[NQ];  // cb: the cum before s0 (SMALL)
    uint2 e[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) e[q] = ld.l1[x[q] >> kCiLowBits];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        c[q] = ci_cell(x[q], e[q]);
        if constexpr (SMALL) {
            const uint2 v = ld.cw[c[q]];
            cb[q] = v.x;
            s0[q] = v.y & 0xffffu;
            n[q] = v.y >> 16;
        } else {
            const unsigned v = ld.cw[c[q]];
            s0[q] = v & 0x3fffu;
            n[q] = v >> 14;
        }
    }
    bool many = false;
#pragma unroll
    for (int q = 0; q < NQ; ++q) many |= n[q] > 1u;
    if (many) {  // a cell of 2+ distinct keys: s0 <- the last one <= x (n = 1), or none (n = 0)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (n[q] > 1u) {
                unsigned lo = s0[q], cnt = n[q];
                if constexpr (!SMALL) cnt = n[q] < 3u ? n[q] : (ld.cw[c[q] + 1] & 0x3fffu) - s0[q];
                while (cnt > 0u) {
                    const unsigned h = cnt >> 1;
                    if (kc[lo + h + 1].x <= x[q]) {
                        lo += h + 1;
                        cnt -= h + 1;
                    } else {
                        cnt = h;
                    }
                }
                if constexpr (SMALL) {  // the cum before the last key <= x, when that is not the cell's first
                    if (lo > s0[q] + 1) cb[q] = kc[lo - 1].y;
                }
                n[q] = lo > s0[q] ? 1u : 0u;
                s0[q] = lo > s0[q] ? lo - 1 : s0[q];
            }
        }
    }
    // kc[s0] = the distinct key before the cell's (or {0, 0}), kc[s0 + 1] = the cell's first one
    uint2 a[NQ], b[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if constexpr (SMALL) {
            a[q] = uint2{0u, cb[q]};
            b[q] = uint2{kPadKey, 0u};
            if (n[q]) b[q] = kc[s0[q] + 1];  // only the lanes whose cell holds keys read it
        } else {
            a[q] = kc[s0[q]];
            b[q] = kc[s0[q] + 1];
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const bool in = n[q] != 0u && b[q].x <= x[q];
        const bool eq = in && b[q].x == x[q];
        const unsigned le = in ? b[q].y : a[q].y;
        const unsigned lt = eq ? a[q].y : le;
        if ((use >> q) & 1u) {
            w += TABLE_POS ? M - le : lt;
            t += le - lt;
        }
    }
}

// the block's W, T (and non-finite count) into out[0..1] (and *nonfinite)
__device__ __forceinline__ void dk_reduce(unsigned long long w, unsigned long long t, unsigned nf,
                                          unsigned long long* __restrict__ out,
                                          unsigned long long* __restrict__ nonfinite) {
    __shared__ unsigned long long red[3][kQueryThreads / kWave];
    w = wave_sum(w);
    t = wave_sum(t);
    const unsigned long long nfw = wave_sum(static_cast<unsigned long long>(nf));
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    if (lane == 0) {
        red[0][wid] = w;
        red[1][wid] = t;
        red[2][wid] = nfw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long bw = 0, bt = 0, bn = 0;
        for (int i = 0; i < kQueryThreads / kWave; ++i) {
            bw += red[0][i];
            bt += red[1][i];
            bn += red[2][i];
        }
        if (bw) atomicAdd(out + 0, bw);
        if (bt) atomicAdd(out + 1, bt);
        if (bn && nonfinite) atomicAdd(nonfinite, bn);
    }
}

// dauc_auc_counts_sorted's form: every element of q[0, L) is a query (no labels); the table is the
// positives (TABLE_POS) or the negatives
template <bool TABLE_POS, bool SMALL>
__global__ __launch_bounds__(kQueryThreads) void dk_plain_kernel(const float* __restrict__ q, int64_t L, DkWs dk,
                                                                 int64_t M, unsigned long long* __restrict__ out) {
    if (dk.meta[kDkUse] == 0u || (dk.meta[kDkD] <= unsigned(kDkSmall)) != SMALL) return;
    extern __shared__ uint2 dk_lds[];
    const DkLds<SMALL> ld = dk_load_lds<SMALL>(dk_lds, dk, M);
    const unsigned long long MM = static_cast<unsigned long long>(M);
    unsigned long long w = 0, t = 0;
    const bool vec = (reinterpret_cast<uintptr_t>(q) & 15u) == 0;
    const int64_t nvec = vec ? L / 4 : 0;
    const int64_t stride = int64_t(gridDim.x) * kQueryThreads;
    const int64_t tid = int64_t(blockIdx.x) * kQueryThreads + threadIdx.x;
    if (nvec > 0) {
        constexpr int U = 2, NQ = 4 * U;
        f32x4 fc[U], fn[U];
        auto load = [&](int64_t v0, f32x4 (&f)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t v = v0 + int64_t(u) * stride;
                f[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q) + (v < nvec ? v : 0));
            }
        };
        load(tid, fc);
        for (int64_t v0 = tid; v0 < nvec; v0 += int64_t(U) * stride) {
            load(v0 + int64_t(U) * stride, fn);
            unsigned x[NQ], use = 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float f[4] = {fc[u].x, fc[u].y, fc[u].z, fc[u].w};
                const unsigned in = v0 + int64_t(u) * stride < nvec ? 0xfu : 0u;
                use |= in << (4 * u);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[4 * u + j] = key_fast(f[j]);
            }
            dk_count<NQ, TABLE_POS, SMALL>(x, use, ld, MM, w, t);
#pragma unroll
            for (int u = 0; u < U; ++u) fc[u] = fn[u];
        }
    }
    for (int64_t i = nvec * 4 + tid; i < L; i += stride) {
        const unsigned x[1] = {key_fast(q[i])};
        dk_count<1, TABLE_POS, SMALL>(x, 1u, ld, MM, w, t);
    }
    dk_reduce(w, t, 0u, out, nullptr);
}

// The labeled query pass over the distinct-key index (the stream and checks of query_labeled_kernel);
// returns at once unless the count index is not in use and the distinct-key index is, in this layout
template <typename LT, bool SMALL, int U = 2>
__global__ __launch_bounds__(kQueryThreads) void dk_query_kernel(const float* __restrict__ s, const LT* __restrict__ lab,
                                                                 int64_t begin, int64_t end,
                                                                 const unsigned* __restrict__ ci_meta, DkWs dk,
                                                                 int64_t M, unsigned long long* __restrict__ out,
                                                                 unsigned long long* __restrict__ nonfinite) {
    if (dk_ci_in_use(ci_meta) || dk.meta[kDkUse] == 0u || (dk.meta[kDkD] <= unsigned(kDkSmall)) != SMALL) return;
    extern __shared__ uint2 dk_lds[];
    const DkLds<SMALL> ld = dk_load_lds<SMALL>(dk_lds, dk, M);
    const unsigned long long MM = static_cast<unsigned long long>(M);
    unsigned long long w = 0, t = 0;
    unsigned nf = 0;
    auto one = [&](int64_t i) {
        if (lab[i] != LT(1)) {
            const float f = s[i];
            nf += !isfinite(f);
            const unsigned x[1] = {key_fast(f)};
            dk_count<1, true, SMALL>(x, 1u, ld, MM, w, t);
        }
    };
    const int64_t a0 = (begin + 3) & ~int64_t(3);
    const int64_t head = a0 < end ? a0 : end;
    const int64_t stride = int64_t(gridDim.x) * kQueryThreads;
    const int64_t tid = int64_t(blockIdx.x) * kQueryThreads + threadIdx.x;
    for (int64_t i = begin + tid; i < head; i += stride) one(i);
    const int64_t nvec = end > head ? (end - head) / 4 : 0;
    const bool aligned = (reinterpret_cast<uintptr_t>(s + head) & 15u) == 0 &&
                         (reinterpret_cast<uintptr_t>(lab + head) & (4 * sizeof(LT) - 1)) == 0;
    if (aligned && nvec > 0) {
        // U float4 slots per iteration, the next iteration's loaded before this one's lookups
        constexpr int NQ = 4 * U;
        f32x4 fc[U], fn[U];
        LabelWords<LT> lc[U], ln[U];
        auto load = [&](int64_t v0, f32x4 (&f)[U], LabelWords<LT> (&l)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t v = v0 + int64_t(u) * stride;
                const int64_t i = head + (v < nvec ? v : 0) * 4;
                f[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s + i));
                l[u].load(lab + i);
                if (v >= nvec) l[u].set_positive();  // past the end: no query
            }
        };
        load(tid, fc, lc);
        for (int64_t v0 = tid; v0 < nvec; v0 += int64_t(U) * stride) {
            load(v0 + int64_t(U) * stride, fn, ln);
            unsigned x[NQ], use = 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float f[4] = {fc[u].x, fc[u].y, fc[u].z, fc[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool neg = lc[u].not_positive(q);
                    use |= unsigned(neg) << (4 * u + q);
                    x[4 * u + q] = key_fast(f[q]);
                    nf += neg && !isfinite(f[q]);
                }
            }
            dk_count<NQ, true, SMALL>(x, use, ld, MM, w, t);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                fc[u] = fn[u];
                lc[u] = ln[u];
            }
        }
    } else if (!aligned) {
        for (int64_t i = head + tid; i < head + nvec * 4; i += stride) one(i);
    }
    for (int64_t i = head + nvec * 4 + tid; i < end; i += stride) one(i);
    dk_reduce(w, t, nf, out, nonfinite);
}
constexpr size_t kDkQueryLds = (size_t(kCiTop) + kDkMax + 2) * 8 + (size_t(kDkMaxCells) + 2) * 2;
constexpr size_t kDkQueryLdsSmall = (size_t(kCiTop) + kDkSmall + 2) * 8 + (size_t(kDkSmallCells) + 1) * 8;
static_assert(kDkQueryLds + 3 * (kQueryThreads / kWave) * 8 <= 160 * 1024, "the distinct-key query's LDS");
static_assert(kDkQueryLdsSmall + 3 * (kQueryThreads / kWave) * 8 <= 160 * 1024, "the distinct-key query's LDS");

template <bool TABLE_POS>
int launch_query(const TablePlan& p, const float* q, int64_t L, const TreeNode* tree, const unsigned* sorted,
                 int64_t M, unsigned long long* out, hipStream_t st, const unsigned* dk_meta = nullptr) {
    const dim3 grid(query_grid(L)), block(kQueryThreads);
#define DAUC_QC(KV)                                                                                              \
    hipLaunchKernelGGL((query_count_kernel<KV, TABLE_POS>), grid, block, p.lds, st, q, L, tree, p.g, p.k, sorted, M, \
                       out, dk_meta)
    switch (p.K) {
        case 1: DAUC_QC(1); break;
        case 2: DAUC_QC(2); break;
        case 4: DAUC_QC(4); break;
        case 8: DAUC_QC(8); break;
        case 16: DAUC_QC(16); break;
        case 32: DAUC_QC(32); break;
        default: DAUC_QC(0); break;
    }
#undef DAUC_QC
    return launch_status();
}

// the count index behind the sort and the tree (first[] was reset by build_tree_kernel): 4 small
// launches; the verdict (usable, skewed) stays on the device
int prepare_count(const unsigned* sorted, int64_t M, const CountWs& cw, hipStream_t st) {
    hipLaunchKernelGGL(ci_first_kernel, dim3(static_cast<unsigned>((M + 255) / 256)), dim3(256), 0, st, sorted, M,
                       cw.first);
    hipLaunchKernelGGL(ci_plan_kernel, dim3(1), dim3(kCiPlanThreads), 0, st, M, cw.first, cw.l1, cw.meta);
    hipLaunchKernelGGL(ci_cells_kernel, dim3(static_cast<unsigned>((M + 1 + 255) / 256)), dim3(256), 0, st, sorted, M,
                       cw.l1, cw.meta, cw.cstart);
    hipLaunchKernelGGL(ci_blocks_kernel, dim3((kCiMaxBlocks + 255) / 256), dim3(256), 0, st, cw.cstart, cw.meta,
                       cw.blk);
    return launch_status();
}

// the distinct-key index behind prepare_count (ci_meta: the count index's verdict, or nullptr when
// it was not built): 4 small launches, each returning at once when the index is not needed / not used
int prepare_dk(const unsigned* sorted, int64_t M, const unsigned* ci_meta, const DkWs& dk, hipStream_t st) {
    const int64_t nt = dk_tiles(M);
    hipLaunchKernelGGL(dk_mark_kernel, dim3(static_cast<unsigned>(nt)), dim3(kDkTile / 4), 0, st, sorted, M, ci_meta,
                       dk.tcnt);
    hipLaunchKernelGGL(dk_scan_kernel, dim3(1), dim3(kDkScanThreads), 0, st, ci_meta, dk, nt);
    hipLaunchKernelGGL(dk_write_kernel, dim3(static_cast<unsigned>(nt)), dim3(kDkTile / 4), 0, st, sorted, M, ci_meta,
                       dk);
    hipLaunchKernelGGL(dk_index_kernel, dim3(1), dim3(kCiPlanThreads), 0, st, ci_meta, dk);
    return launch_status();
}

template <bool TABLE_POS>
int launch_dk_plain(const float* q, int64_t L, const DkWs& dk, int64_t M, unsigned long long* out, hipStream_t st) {
    // both layouts enqueued: the one the device's distinct count does not select returns at once
    hipLaunchKernelGGL((dk_plain_kernel<TABLE_POS, true>), dim3(query_grid(L)), dim3(kQueryThreads), kDkQueryLdsSmall,
                       st, q, L, dk, M, out);
    hipLaunchKernelGGL((dk_plain_kernel<TABLE_POS, false>), dim3(query_grid(L)), dim3(kQueryThreads), kDkQueryLds, st,
                       q, L, dk, M, out);
    return launch_status();
}

// (in both launchers `lab` is q.labels with its element type)
template <typename LT>
int launch_dk(const LabeledQueries& q, const LT* lab, const unsigned* ci_meta, const DkWs& dk, int64_t M,
              hipStream_t st) {
    // both layouts enqueued: the one the device's distinct count does not select returns at once
    const dim3 grid(query_grid(q.end - q.begin));
    hipLaunchKernelGGL((dk_query_kernel<LT, true>), grid, dim3(kQueryThreads), kDkQueryLdsSmall, st, q.scores, lab,
                       q.begin, q.end, ci_meta, dk, M, q.wins_ties, q.nonfinite);
    hipLaunchKernelGGL((dk_query_kernel<LT, false>), grid, dim3(kQueryThreads), kDkQueryLds, st, q.scores, lab, q.begin,
                       q.end, ci_meta, dk, M, q.wins_ties, q.nonfinite);
    return launch_status();
}

template <typename LT>
int launch_labeled(const TablePlan& p, const LabeledQueries& q, const LT* lab, const TreeNode* tree,
                   const unsigned* sorted, int64_t M, const unsigned* meta, hipStream_t st,
                   const unsigned* dk_meta = nullptr) {
    const dim3 grid(query_grid(q.end - q.begin)), block(kQueryThreads);
#define DAUC_QL(KV)                                                                                              \
    hipLaunchKernelGGL((query_labeled_kernel<KV, LT>), grid, block, p.lds, st, q.scores, lab, q.begin, q.end, tree, \
                       p.g, p.k, sorted, M, q.wins_ties, q.nonfinite, meta, dk_meta)
    switch (p.K) {
        case 1: DAUC_QL(1); break;
        case 2: DAUC_QL(2); break;
        case 4: DAUC_QL(4); break;
        case 8: DAUC_QL(8); break;
        case 16: DAUC_QL(16); break;
        case 32: DAUC_QL(32); break;
        default: DAUC_QL(0); break;
    }
#undef DAUC_QL
    return launch_status();
}

// sort the table, build the tree of its plan (table_plan(M)) into ws.tree
int prepare_table(const float* table, int64_t M, const TablePlan& p, const SortWorkspace& ws, hipStream_t st,
                  const unsigned** sorted, unsigned* ci_first = nullptr) {
    int rc = radix_sort_keys(table, M, ws.sort, st, sorted);
    if (rc) return rc;
    const int n_first = ci_first ? kCiTop : 0;
    int64_t nthreads = (p.g.nodes > p.pad) ? p.g.nodes : p.pad;
    if (nthreads < 8) nthreads = 8;
    if (nthreads < n_first) nthreads = n_first;
    hipLaunchKernelGGL(build_tree_kernel, dim3(static_cast<unsigned>((nthreads + 255) / 256)), dim3(256), 0, st,
                       const_cast<unsigned*>(*sorted), M, p.pad, p.k, p.g, ws.tree, ci_first, n_first);
    return launch_status();
}

}  // namespace

bool direct_enabled() { return g_search_mode == 0; }

int counts_sorted_labeled(const float* pos, int64_t P, const LabeledQueries& q, void* workspace,
                          size_t workspace_bytes, hipStream_t st, bool count_index) {
    if (!q.valid() || P < 0 || (P > 0 && pos == nullptr)) return DAUC_EINVAL;
    if (P == 0 || q.empty()) return DAUC_OK;
    if (workspace == nullptr || workspace_bytes < dauc_sort_workspace_size(P) || P > 0xffffffffLL) return DAUC_EINVAL;
    const SortWorkspace ws = sort_workspace(workspace, P);
    const unsigned* sorted = nullptr;
    const TablePlan plan = table_plan(P);
    // the search structure: mode 0 the count index where the table can use it, else the
    // distinct-key index where it holds the table, else the tree (every choice made on the device);
    // 1 the tree; 2 the distinct-key index, else the tree
    const int mode = g_search_mode;
    const bool count = count_index && mode == 0 && P <= kCiMaxTable;
    const bool distinct = mode == 0 || mode == 2;  // the distinct-key index where the count index is not used
    const CountWs& nw = ws.count;
    const DkWs& dk = ws.dk;
    int rc = prepare_table(pos, P, plan, ws, st, &sorted, count ? nw.first : nullptr);
    if (rc) return rc;
    if (count && (rc = prepare_count(sorted, P, nw, st))) return rc;
    const unsigned* meta = count ? nw.meta : nullptr;
    if (distinct && (rc = prepare_dk(sorted, P, meta, dk, st))) return rc;
    rc = with_labels(q.labels, q.label_dtype, [&](auto* lab) {
        return launch_labeled(plan, q, lab, ws.tree, sorted, P, meta, st, distinct ? dk.meta : nullptr);
    });
    if (rc == DAUC_OK && count) rc = launch_ci(q, nw, sorted, P, st, CiForm::sorted());
    if (rc == DAUC_OK && distinct)
        rc = with_labels(q.labels, q.label_dtype, [&](auto* lab) { return launch_dk(q, lab, meta, dk, P, st); });
    return rc;
}

}  // namespace dauc

using namespace dauc;

extern "C" {

size_t dauc_sort_workspace_size(int64_t n) { return sort_workspace(nullptr, n < 1 ? 1 : n).bytes; }

#ifdef DAUC_TUNING
int dauc_set_search_mode(int mode) {
    if (mode < 0 || mode > 2) return DAUC_EINVAL;
    g_search_mode = mode;
    return DAUC_OK;
}

// tuning builds: the plan of the sorted path for a table of M keys (include/dauc_tuning.h), from the
// functions the launchers launch from (sort_layout, table_plan, dk_tiles) and the run lengths the
// two one-workgroup scans compute from them; host arithmetic only
int dauc_sort_table_plan(int64_t M, int64_t out[DAUC_SORT_PLAN_WORDS]) {
    if (out == nullptr || M < 1 || M > 0xffffffffLL) return DAUC_EINVAL;
    WsWalker w(nullptr);
    const SortWs s = sort_layout(w, M);
    const TablePlan p = table_plan(M);
    out[0] = s.ntiles;
    out[1] = s.fused_scan ? 0 : 1;
    out[2] = s.nsum;
    out[3] = scan_sums_run(s.nsum);
    out[4] = p.k;
    out[5] = p.S;
    out[6] = p.g.H;
    out[7] = p.g.nodes;
    out[8] = static_cast<int64_t>(p.lds);
    out[9] = p.pad;
    out[10] = p.K;
    out[11] = dk_tiles(M);
    out[12] = dk_scan_run(dk_tiles(M));
    out[13] = kDkMax;
    out[14] = kCiMaxTable;
    out[15] = kMaxSplit;
    return DAUC_OK;
}
#endif

int dauc_auc_counts_sorted(const float* pos, int64_t P, const float* neg, int64_t N,
                           unsigned long long* wins_ties, void* workspace, size_t workspace_bytes,
                           dauc_stream_t stream) {
    if (P < 0 || N < 0 || wins_ties == nullptr || (P > 0 && pos == nullptr) ||
        (N > 0 && neg == nullptr))
        return DAUC_EINVAL;
    if (P == 0 || N == 0) return DAUC_OK;
    // the smaller class is sorted (the table); the larger one streams through the search
    const bool table_pos = P <= N;
    const int64_t M = table_pos ? P : N, L = table_pos ? N : P;
    if (workspace == nullptr || workspace_bytes < dauc_sort_workspace_size(M) || M > 0xffffffffLL) return DAUC_EINVAL;
    hipStream_t st = as_hip(stream);
    const SortWorkspace ws = sort_workspace(workspace, M);
    const TreeNode* tree = ws.tree;
    const unsigned* sorted = nullptr;
    const TablePlan plan = table_plan(M);
    int rc = prepare_table(table_pos ? pos : neg, M, plan, ws, st, &sorted);
    if (rc) return rc;
    const float* q = table_pos ? neg : pos;
    // the distinct-key index where it holds the table (tie-heavy), else the tree: chosen on the device
    const bool distinct = g_search_mode != 1;
    const DkWs& dk = ws.dk;
    if (distinct && (rc = prepare_dk(sorted, M, nullptr, dk, st))) return rc;
    const unsigned* dkm = distinct ? dk.meta : nullptr;
    rc = table_pos ? launch_query<true>(plan, q, L, tree, sorted, M, wins_ties, st, dkm)
                   : launch_query<false>(plan, q, L, tree, sorted, M, wins_ties, st, dkm);
    if (rc || !distinct) return rc;
    return table_pos ? launch_dk_plain<true>(q, L, dk, M, wins_ties, st)
                     : launch_dk_plain<false>(q, L, dk, M, wins_ties, st);
}

int dauc_auc_counts_sorted_labeled(const float* pos, int64_t P, const float* scores, const void* labels,
                                   int label_dtype, int64_t begin, int64_t end, unsigned long long* wins_ties,
                                   unsigned long long* nonfinite, void* workspace, size_t workspace_bytes,
                                   dauc_stream_t stream) {
    return counts_sorted_labeled(pos, P, LabeledQueries{scores, labels, label_dtype, begin, end, wins_ties, nonfinite},
                                 workspace, workspace_bytes, as_hip(stream), true);
}

}  // extern "C"
