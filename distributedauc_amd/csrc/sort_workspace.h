// The sort workspace (dauc_sort_workspace_size): ONE description of every region in it, walked once
// for the size (base = nullptr) and once for the pointers, so a size cannot disagree with its carve.
// Regions, in this order, each starting on a 256-byte boundary (valid_args and the kernels' vector
// loads rely on it):
//   sort buffers | search tree | the direct build's group totals | count index | distinct-key index
#pragma once

#include "count_index.h"

namespace dauc {

// A cursor over a workspace: take<T>(count) returns the region at the cursor and advances it by the
// region's bytes rounded up to 256. On a null base the pointers are offsets and used() is the size.
struct WsWalker {
    uintptr_t base, at;
    explicit WsWalker(void* ws) : base(reinterpret_cast<uintptr_t>(ws)), at(base) {}
    template <typename T>
    T* take(size_t count) {
        T* r = reinterpret_cast<T*>(at);
        at += (count * sizeof(T) + 255) / 256 * 256;
        return r;
    }
    size_t used() const { return at - base; }
};

// ---- sort buffers -----------------------------------------------------------------------------
constexpr int kSortThreads = 256;
constexpr int kPerThread = 8;  // keys per thread per pass tile
constexpr int kTile = kSortThreads * kPerThread;  // 2048 keys (8 per thread: the hist pass 4.9 vs 6.1 us at 134k keys)
constexpr int kRadix = 256;
constexpr int kScanBlock = 1024;
// A sort of up to kFusedScanTiles tiles has no scan launches: every scatter workgroup derives its own
// offsets from the raw histogram (radix_sort.hip, radix_scatter_kernel<., true>); a larger one scans
// the histogram in three launches (blocks, block sums, add back).
constexpr int64_t kFusedScanTiles = 256;

inline int64_t tiles_for(int64_t n) { return (n + kTile - 1) / kTile; }

// block sums each thread of the one-workgroup scan_sums_kernel takes (its run loop: 2 or more from
// 1025 block sums on, i.e. more than 4096 tiles)
__host__ __device__ inline int64_t scan_sums_run(int64_t nb) { return (nb + kScanBlock - 1) / kScanBlock; }

// The sort's plan and buffers: radix_sort_keys launches from these fields alone, and the tuning
// build's dauc_sort_table_plan reports them.
struct SortWs {
    unsigned* keys_a;
    unsigned* keys_b;
    unsigned* hist;
    unsigned* sums;
    int64_t ntiles, m, nsum;  // tiles; histogram entries (256 per tile); scan blocks of 1024 entries
    bool fused_scan;          // ntiles <= kFusedScanTiles: no scan launches
};

inline SortWs sort_layout(WsWalker& w, int64_t n) {
    SortWs s;
    s.ntiles = tiles_for(n);
    s.m = int64_t(kRadix) * s.ntiles;
    s.nsum = (s.m + kScanBlock - 1) / kScanBlock;
    s.fused_scan = s.ntiles <= kFusedScanTiles;
    s.keys_a = w.take<unsigned>(n + 64);  // + room for the last bucket's kPadKey tail
    s.keys_b = w.take<unsigned>(n + 64);
    s.hist = w.take<unsigned>(s.m);
    s.sums = w.take<unsigned>(s.nsum);
    return s;
}

// dauc_sort_keys' workspace: the sort buffers alone
inline SortWs sort_ws(void* ws, int64_t n) {
    WsWalker w(ws);
    return sort_layout(w, n);
}
inline size_t sort_ws_bytes(int64_t n) {
    WsWalker w(nullptr);
    sort_layout(w, n);
    return w.used();
}

// ---- search tree ------------------------------------------------------------------------------
// Splitters (every k-th sorted key, k a power of two) kept in LDS: at most kMaxSplit of them
// (4 B each: 40000 -> 156 KB of the CU's 160 KB), so a bucket holds k <= 4 keys -- ONE 16-byte
// load -- up to M = 160,000 table keys (2^27 scores at 0.1 % positives: M = 134,447 -> k = 4).
constexpr int kMaxSplit = 40000;
constexpr size_t kTreeBytes = (size_t(kMaxSplit) + 64) * 4;  // nodes of 4 keys + per-level padding nodes
typedef uint4 TreeNode;

// ---- the direct build's 72 group totals (grp) ---------------------------------------------------
constexpr size_t kGrpBytes = 512;

// ---- count index ------------------------------------------------------------------------------
struct CountWs {
    unsigned* meta;    // [16]
    unsigned* first;   // [kCiTop]      first table index of every top bucket (M = none)
    uint2* l1;         // [kCiTop]      {first cell, cells} of every top bucket
    unsigned* cstart;  // [kCiMaxCells + 2] first table index of every cell
    uint2* blk;        // [kCiMaxBlocks] {keys before the block, 8 nibble counts}
};

// the cstart region in words: the direct build's per-cell counters
constexpr int64_t kCiCntWords = ((int64_t(kCiMaxCells) + 2) * 4 + 255) / 256 * 64;

inline CountWs count_layout(WsWalker& w) {
    CountWs c;
    c.meta = w.take<unsigned>(64);
    c.first = w.take<unsigned>(kCiTop);
    c.l1 = w.take<uint2>(kCiTop);
    c.cstart = w.take<unsigned>(size_t(kCiMaxCells) + 2);
    c.blk = w.take<uint2>(kCiMaxBlocks);
    return c;
}

// ---- distinct-key index of tie-heavy tables (dk_*_kernel, auc_sort.hip) -----------------------
constexpr int kDkMax = 14000;
static_assert(kDkMax < 16384, "the query's LDS holds a cell's first distinct key in 14 bits");
// the plan's cells: 4 per distinct key (up to 3,500 of them), fewer but at least 1 past that, + 1 per used bucket
constexpr int kDkMaxCells = kDkMax + kCiTop;
constexpr int kDkTile = 1024;                     // table keys per tile of the mark / write passes (4 per thread)

inline int64_t dk_tiles(int64_t M) { return (M + kDkTile - 1) / kDkTile; }

// DkWs is a parameter of the dk_* kernels, so its namespace is part of their mangled names: it stays
// in an anonymous namespace, as in the source these kernels came from, to keep their symbols (the
// kernel-by-kernel comparison of device code goes by symbol) -- and with it what holds one. Every
// including unit gets its own copy of these types; none crosses a unit boundary.
namespace {
struct DkWs {
    unsigned* meta;    // [16]
    uint2* l1;         // [kCiTop]
    unsigned* cstart;  // [kDkMaxCells + 2] the first distinct key of every cell
    unsigned* kd;      // [kDkMax] the distinct keys, ascending
    unsigned* cd;      // [kDkMax] #(table keys <= kd[i])
    unsigned* tcnt;    // [tiles] distinct keys whose last copy is in the tile -> their exclusive prefix
};

inline DkWs dk_layout(WsWalker& w, int64_t M) {
    DkWs d;
    d.meta = w.take<unsigned>(64);
    d.l1 = w.take<uint2>(kCiTop);
    d.cstart = w.take<unsigned>(size_t(kDkMaxCells) + 2);
    d.kd = w.take<unsigned>(kDkMax);
    d.cd = w.take<unsigned>(kDkMax);
    d.tcnt = w.take<unsigned>(size_t(dk_tiles(M < 1 ? 1 : M)));
    return d;
}

// ---- the whole workspace for a table of up to n keys --------------------------------------------
struct SortWorkspace {
    SortWs sort;
    TreeNode* tree;
    unsigned* grp;  // [kDirectMaxGroups]
    CountWs count;
    DkWs dk;
    size_t bytes;
};

inline SortWorkspace sort_workspace(void* ws, int64_t n) {
    WsWalker w(ws);
    SortWorkspace s;
    s.sort = sort_layout(w, n);
    s.tree = w.take<TreeNode>(kTreeBytes / sizeof(TreeNode));
    s.grp = w.take<unsigned>(kGrpBytes / 4);
    s.count = count_layout(w);
    s.dk = dk_layout(w, n);
    s.bytes = w.used();
    return s;
}
}  // namespace

// radix_sort.hip: sorts the keys of in[0..n) into the sort buffers; *sorted = the sorted array
int radix_sort_keys(const float* in, int64_t n, const SortWs& w, hipStream_t st, const unsigned** sorted);

}  // namespace dauc
