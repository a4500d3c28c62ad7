// The labeled query pass through the count index (count_index.h): query_ci_kernel, which locates
// every score of [begin, end) whose label is not +1 among the positives' table. The product's hot
// path ends here: compaction (auc_count.hip), slotted count pass (count_index.hip), then
// query_ci_kernel<LT, CHECK, SLOT, SEC> -- SLOT for the slotted table, CHECK for the two-step
// evaluation's check word. Reached through launch_ci (sort_workspace.h) from count_index.hip's
// counts_labeled_* (dauc_auc_eval_*) and from the sorted path (auc_sort.hip,
// dauc_auc_counts_sorted_labeled; the index and its cost are described there and in count_index.h).

#include "auc_query.h"
#include "auc_eval_internal.h"

namespace dauc {
namespace {

// a 16-byte window of the L2-resident table
__device__ __forceinline__ uint4 win_load(const unsigned* p) { return *reinterpret_cast<const uint4*>(p); }

// Counting in VGPRs only: gt01(a, b) = min(sat(a - b), 1) is 1 when a > b, else 0. A compare into
// an SGPR read back by a v_cndmask / v_addc costs the VALU-writes-SGPR hazard's wait states on
// every key (the round-3 loop issued 110 VALU per query, s_nop-padded, ~75 % of the SIMDs' issue
// cycles: DESIGN §3).
__device__ __forceinline__ unsigned gt01(unsigned a, unsigned b) {
    return min(__builtin_elementwise_sub_sat(a, b), 1u);
}
// the window's keys <= x and < x
__device__ __forceinline__ void win_le_lt(const uint4& k, unsigned x, unsigned& le, unsigned& lt) {
    le = 4u - (gt01(k.x, x) + gt01(k.y, x) + gt01(k.z, x) + gt01(k.w, x));
    lt = gt01(x, k.x) + gt01(x, k.y) + gt01(x, k.z) + gt01(x, k.w);
}

// Phase 1 of one query: cell, rank_lo, count and (lanes with cnt > 0) the window load
__device__ __forceinline__ void ci_locate(unsigned x, const uint2* __restrict__ l1, const uint2* __restrict__ blk,
                                          const unsigned* __restrict__ sorted, unsigned& rl, unsigned& cnt,
                                          uint4& k) {
    const unsigned c = ci_cell(x, l1[x >> kCiLowBits]);
    const uint2 b = blk[c / kCiBlock];
    const unsigned sh = 4u * (c % kCiBlock);
    const unsigned below = __builtin_amdgcn_ubfe(b.y, 0u, sh);           // nibbles of the cells before
    const unsigned bytes = (below & 0x0f0f0f0fu) + ((below >> 4) & 0x0f0f0f0fu);
    rl = b.x + __builtin_amdgcn_sad_u8(bytes, 0u, 0u);
    cnt = __builtin_amdgcn_ubfe(b.y, sh, 4u);
    k = uint4{kPadKey, kPadKey, kPadKey, kPadKey};
    if (cnt) k = *reinterpret_cast<const uint4*>(sorted + (rl & ~3u));
}

// Phase 2: lb, ub from the window (W += M - ub, T += ub - lb for use); returns whether the cell
// runs past the window (then ci_fix recounts it)
__device__ __forceinline__ bool ci_count(unsigned x, bool use, unsigned rl, unsigned cnt, const uint4& k, unsigned M,
                                         unsigned& wl, unsigned& tl) {
    const unsigned base = cnt ? (rl & ~3u) : rl;
    const unsigned lt = (k.x < x) + (k.y < x) + (k.z < x) + (k.w < x);
    const unsigned le = (k.x <= x) + (k.y <= x) + (k.z <= x) + (k.w <= x);
    wl += use ? M - (base + le) : 0u;
    tl += use ? le - lt : 0u;
    return use && (rl & 3u) + cnt > 4u;
}

// a cell past its window: the next 4 keys (or, past 8, every key of the cell); corrects W and T
__device__ __forceinline__ void ci_fix(unsigned x, unsigned rl, unsigned cnt, const uint4& k,
                                       const unsigned* __restrict__ sorted, unsigned long long& w,
                                       unsigned long long& t) {
    const unsigned a = rl & ~3u;
    const unsigned lt0 = (k.x < x) + (k.y < x) + (k.z < x) + (k.w < x);
    const unsigned le0 = (k.x <= x) + (k.y <= x) + (k.z <= x) + (k.w <= x);
    int64_t lb, ub;
    if ((rl & 3u) + cnt <= 8u) {
        const uint4 k2 = *reinterpret_cast<const uint4*>(sorted + a + 4);
        lb = int64_t(a) + lt0 + (k2.x < x) + (k2.y < x) + (k2.z < x) + (k2.w < x);
        ub = int64_t(a) + le0 + (k2.x <= x) + (k2.y <= x) + (k2.z <= x) + (k2.w <= x);
    } else {
        // <= 14 keys (a cell of 15+ keys marks the table skewed): counted one by one, so the order
        // of the keys inside the cell does not matter (the direct build orders the table by cell only)
        lb = rl;
        ub = rl;
        for (unsigned j = rl; j < rl + cnt; ++j) {
            const unsigned v = sorted[j];
            lb += v < x;
            ub += v <= x;
        }
    }
    const int64_t lbf = int64_t(a) + lt0, ubf = int64_t(a) + le0;
    w -= static_cast<unsigned long long>(ub - ubf);
    t += static_cast<unsigned long long>((ub - lb) - (ubf - lbf));
}

// SLOT: keys 8 .. cnt - 1 of cell c (its tertiary run), counted one by one after the two windows
// counted the first 8: W += M - ub loses the run's keys <= x, T gains its keys == x
__device__ __forceinline__ void slot_tertiary(unsigned x, unsigned c, unsigned cnt, const unsigned* __restrict__ tab,
                                              unsigned cells, unsigned long long& w, unsigned long long& t) {
    const unsigned* r = tab + slot_ter(cells, c);
    for (unsigned j = 0; j + 8u < cnt; ++j) {
        const unsigned v = r[j];
        w -= v <= x;
        t += (v <= x) - (v < x);
    }
}

// The labeled query pass over the count index (same stream and checks as query_labeled_kernel);
// returns at once when the builder kept the tree, so it is enqueued unconditionally. Per
// iteration every slot's window loads are issued BEFORE the next iteration's stream loads:
// vmcnt retires loads in issue order, so a wait for a window would otherwise also wait out a
// streaming load's HBM latency. CHECK (the two-step evaluation): *check += #queries over [begin,
// end) (mod 2^32) -- also when the index is not used (the pass then only reads the range for it) --
// so the caller can compare the range's positives with the ones another rank compacted from it.
// The loop runs at the 128-VGPR bound of 4 waves per SIMD, so the query count rides in the high
// half of the non-finite counter (per lane both stay far below 2^16): no extra register.
//
// SLOT (round 6): the cell-slotted table of direct_count_slots_kernel<true> (count_index.h). `blkg`
// is then the raw per-cell byte counts (8 per block: the block words' size), turned into block words
// in LDS by the workgroup itself (each thread sums its run of 18 blocks, one workgroup scan, written
// back in place); `sorted` is the slotted table of `slot_cells` cells. A cell's keys are its primary
// window (+inf past its count), its secondary window past 4 keys and, past 8 (rare), its tertiary
// run: W += M - (rank_lo + #keys <= x), T += #(== x); no straddling windows.
// SEC (SLOT only; round 6): ONE secondary window per lane per group of 4 queries instead of one per
// query: cells of 5+ keys are ~0.6 % of the queries, so a lane loads the secondary window of its
// group's first such query (the +inf pad when there is none) with the group's primaries, and counts
// it with them; a second such query in the same group (~2e-4 of lane-groups) is counted at once.
// 12 fewer live VGPRs per group and ~69 fewer VALU per group.
// (SEC is only instantiated true; the per-query form went with its tuning knob.)
template <typename LT, bool CHECK = false, bool SLOT = false, bool SEC = true>
__global__ __launch_bounds__(kQueryThreads) void query_ci_kernel(const float* __restrict__ s,
                                                                const LT* __restrict__ lab, int64_t begin,
                                                                int64_t end, unsigned* __restrict__ meta,
                                                                const uint2* __restrict__ l1g,
                                                                const uint2* __restrict__ blkg,
                                                                const unsigned* __restrict__ sorted, int64_t M,
                                                                unsigned long long* __restrict__ out,
                                                                unsigned long long* __restrict__ nonfinite,
                                                                unsigned* __restrict__ verdict,
                                                                const unsigned* __restrict__ grp,
                                                                const unsigned long long* __restrict__ Mp,
                                                                unsigned* __restrict__ check, unsigned slot_cells = 0u,
                                                                unsigned long long* __restrict__ red8 = nullptr) {
    const unsigned pad_word = 4u * slot_cells;  // SLOT: the all-+inf primary slot past the last cell
    // SLOT: the index's loads (the l1 plan, the byte counts of every block the workspace holds) are
    // issued BEFORE the meta words are read, so the prologue waits one round trip, not two (meta ->
    // block count -> loads); blocks past the count are loaded and never stored
    constexpr int kL1Per = kCiTop / kQueryThreads;                                 // 2
    constexpr int kBlkPer = (kCiMaxBlocks + kQueryThreads - 1) / kQueryThreads;  // 18
    uint2 pre_a[SLOT ? kL1Per : 1], pre_v[SLOT ? kBlkPer : 1];
    if constexpr (SLOT) {
#pragma unroll
        for (int j = 0; j < kL1Per; ++j) pre_a[j] = l1g[j * kQueryThreads + threadIdx.x];
#pragma unroll
        for (int j = 0; j < kBlkPer; ++j) {
            const int i = j * kQueryThreads + threadIdx.x;
            pre_v[j] = i < kCiMaxBlocks ? blkg[i] : uint2{0u, 0u};
        }
    }
    const bool in_use = count_index_in_use(meta);
    if (Mp != nullptr) M = static_cast<int64_t>(*Mp);  // the direct build: the table size on the device
    if constexpr (SLOT) {
        // the slotted state is consumed (read after every count-pass workgroup finished: stream order)
        if (blockIdx.x == 0 && threadIdx.x == 0) meta[kCiConsumed] = 1u;
    }
    // the end-of-kernel reduction's rows (W, T, #non-finite, CHECK: #queries); static LDS on top of
    // the index's 163,232 dynamic bytes: the 160 KB limit leaves room for 4 rows, no more
    __shared__ unsigned long long red[CHECK ? 4 : 3][kQueryThreads / kWave];
    if (verdict != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *verdict = in_use ? 1u : 2u;
    if (!in_use) {
        if constexpr (CHECK) {
            // the consistency word and the finiteness of every query, whatever the table
            unsigned nf = 0u, chk = 0u;
            for (int64_t i = begin + int64_t(blockIdx.x) * kQueryThreads + threadIdx.x; i < end;
                 i += int64_t(gridDim.x) * kQueryThreads) {
                if (lab[i] != LT(1)) {
                    nf += !isfinite(s[i]);
                    chk += 1u;
                }
            }
            // one atomic per workgroup and word (per-wave atomics on one address serialise)
            const unsigned long long nfw = wave_sum(static_cast<unsigned long long>(nf));
            const unsigned long long ckw = wave_sum(static_cast<unsigned long long>(chk));
            if ((threadIdx.x & (kWave - 1)) == 0) {
                red[0][threadIdx.x / kWave] = nfw;
                red[1][threadIdx.x / kWave] = ckw;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned long long bn = 0, bc = 0;
                for (int i = 0; i < kQueryThreads / kWave; ++i) {
                    bn += red[0][i];
                    bc += red[1][i];
                }
                if (bn && nonfinite != nullptr) atomicAdd(nonfinite, bn);
                if (bc) atomicAdd(check, static_cast<unsigned>(bc));
            }
            return;
        }
        // no positives at all: nothing to count, but the queries are still checked for finiteness
        // (sklearn raises on a non-finite score before its one-class warning, _ranking.py:868-869)
        if (M == 0 && nonfinite != nullptr) {
            unsigned nf = 0;
            for (int64_t i = begin + int64_t(blockIdx.x) * kQueryThreads + threadIdx.x; i < end;
                 i += int64_t(gridDim.x) * kQueryThreads)
                nf += lab[i] != LT(1) && !isfinite(s[i]);
            const unsigned long long nfw = wave_sum(static_cast<unsigned long long>(nf));
            if ((threadIdx.x & (kWave - 1)) == 0 && nfw) atomicAdd(nonfinite, nfw);
        }
        return;
    }
    extern __shared__ uint2 ci_lds[];
    const int nb = static_cast<int>(meta[kCiBlocks]);
    uint2* l1 = ci_lds;          // [2048]
    uint2* blk = ci_lds + kCiTop;  // [nb]
    {
        // the index into LDS with every load of a thread in flight before its first LDS store (a
        // load-store loop waits out one L2 round trip per iteration: 18 of them per thread)
        uint2 a[kL1Per], v[kBlkPer];
        if constexpr (SLOT) {  // (loaded above)
#pragma unroll
            for (int j = 0; j < kL1Per; ++j) a[j] = pre_a[j];
#pragma unroll
            for (int j = 0; j < kBlkPer; ++j)
                v[j] = uint2(pre_v[j]);  // (through a temporary: a plain assignment schedules differently)
        } else {
#pragma unroll
            for (int j = 0; j < kL1Per; ++j) a[j] = l1g[j * kQueryThreads + threadIdx.x];
#pragma unroll
            for (int j = 0; j < kBlkPer; ++j) {
                const int i = j * kQueryThreads + threadIdx.x;
                v[j] = i < nb ? blkg[i] : uint2{0u, 0u};
            }
        }
        if (grp != nullptr) {
            // the direct build's block words hold prefixes within groups of 256 blocks: add the groups'
            unsigned* pre = reinterpret_cast<unsigned*>(blk + kCiMaxBlocks);
            group_prefix(grp, (nb + kDirectGroup - 1) / kDirectGroup, pre);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kBlkPer; ++j) v[j].x += pre[(j * kQueryThreads + threadIdx.x) / kDirectGroup];
        }
#pragma unroll
        for (int j = 0; j < kL1Per; ++j) l1[j * kQueryThreads + threadIdx.x] = a[j];
#pragma unroll
        for (int j = 0; j < kBlkPer; ++j) {
            const int i = j * kQueryThreads + threadIdx.x;
            if (i < nb) blk[i] = v[j];
        }
    }
    if constexpr (SLOT) {
        // byte counts -> block words {keys before the block, the 8 counts as nibbles}, in place:
        // thread t owns blocks [18 t, 18 t + 18); its run total, one workgroup scan, then each
        // block rewritten with its exclusive prefix (counts <= 14: a skewed table never gets here)
        constexpr int kOwn = (kCiMaxBlocks + kQueryThreads - 1) / kQueryThreads;  // 18
        __syncthreads();
        const int b0 = threadIdx.x * kOwn;
        unsigned run = 0u;
#pragma unroll
        for (int j = 0; j < kOwn; ++j) {
            if (b0 + j < nb) {
                const uint2 r = blk[b0 + j];
                run += __builtin_amdgcn_sad_u8(r.x, 0u, 0u) + __builtin_amdgcn_sad_u8(r.y, 0u, 0u);
            }
        }
        unsigned before = block_incl_scan1024<false>(run, reinterpret_cast<unsigned*>(&red[0][0])) - run;
#pragma unroll
        for (int j = 0; j < kOwn; ++j) {
            if (b0 + j < nb) {
                const uint2 r = blk[b0 + j];
                // bytes b0..b3 (each <= 14) -> nibbles: 0x0b3b2b1b0 per half
                const unsigned tl = (r.x & 0x000f000fu) | ((r.x >> 4) & 0x00f000f0u);
                const unsigned th = (r.y & 0x000f000fu) | ((r.y >> 4) & 0x00f000f0u);
                const unsigned nib = (tl & 0xffu) | ((tl >> 8) & 0xff00u) | ((th & 0xffu) << 16) | ((th >> 8) & 0xff00u) << 16;
                blk[b0 + j] = uint2{before, nib};
                before += __builtin_amdgcn_sad_u8(r.x, 0u, 0u) + __builtin_amdgcn_sad_u8(r.y, 0u, 0u);
            }
        }
    }
    __syncthreads();
    const unsigned M32 = static_cast<unsigned>(M);
    unsigned long long w = 0, t = 0;
    unsigned nf = 0;  // CHECK: + #queries << 16
    const int64_t a0 = (begin + 3) & ~int64_t(3);
    const int64_t head = a0 < end ? a0 : end;
    const int64_t stride = int64_t(gridDim.x) * kQueryThreads;
    const int64_t tid = int64_t(blockIdx.x) * kQueryThreads + threadIdx.x;
    auto one = [&](int64_t i) {
        if (lab[i] != LT(1)) {
            nf += !isfinite(s[i]) + (CHECK ? 0x10000u : 0u);
            const unsigned x = key_fast(s[i]);
            if constexpr (SLOT) {
                const unsigned c = ci_cell(x, l1[x >> kCiLowBits]);
                unsigned rl, cnt;
                ci_decode(c, blk[c / kCiBlock], rl, cnt);
                const uint4 k = win_load(sorted + (cnt ? 4u * c : pad_word));
                const uint4 k2 = win_load(sorted + (cnt > 4u ? slot_sec(slot_cells, c) : pad_word));
                unsigned le, lt, le2, lt2;
                win_le_lt(k, x, le, lt);
                win_le_lt(k2, x, le2, lt2);
                w += M32 - (rl + le + le2);
                t += (le - lt) + (le2 - lt2);
                if (cnt > 8u) slot_tertiary(x, c, cnt, sorted, slot_cells, w, t);
            } else {
                unsigned rl, cnt, wl = 0u, tl = 0u;
                uint4 k;
                ci_locate(x, l1, blk, sorted, rl, cnt, k);
                const bool more = ci_count(x, true, rl, cnt, k, M32, wl, tl);
                w += wl;
                t += tl;
                if (more) ci_fix(x, rl, cnt, k, sorted, w, t);
            }
        }
    };
    for (int64_t i = begin + tid; i < head; i += stride) one(i);
    const int64_t nvec = end > head ? (end - head) / 4 : 0;
    const bool aligned = (reinterpret_cast<uintptr_t>(s + head) & 15u) == 0 &&
                         (reinterpret_cast<uintptr_t>(lab + head) & (4 * sizeof(LT) - 1)) == 0;
    if (aligned) {
        // Software-pipelined over groups of NQ queries (U float4 slots per thread): the LDS lookups
        // of group g run while group g-1's window loads and group g+1's stream loads are in
        // flight, and group g-1 is counted after group g's windows are issued. Per group, in
        // issue order: keys(g) [waits for the stream loads issued one group earlier], stream
        // loads of g+1, LDS lookups of g, window loads of g, count of g-1 [waits for the windows
        // issued one group earlier; the younger loads stay in flight: vmcnt retires in order].
        constexpr int U = 1;  // one float4 slot per lane per group (more slots spill registers)
        constexpr int NQ = 4 * U;
        const int64_t step = int64_t(U) * stride;
        // two sets of every per-group register (A and B, used alternately by an unrolled pair of
        // iterations): a loop that rotated one set into the other would copy loaded registers at
        // its back-edge, i.e. wait there for the loads it had just issued
        struct Stream {
            f32x4 f[U];
            LabelWords<LT> l[U];
        };
        // Every load of the loop is issued unconditionally (out-of-range slots re-read slot 0 and are
        // masked; a lane without a window reads the table's first one): a load under a branch
        // leaves the number of younger loads in flight unknown, and the compiler then waits with
        // vmcnt(0) -- for every load in flight -- instead of a counted wait.
        auto load = [&](Stream& sg, int64_t v0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t v = v0 + int64_t(u) * stride;
                const int64_t i = head + (v < nvec ? v : 0) * 4;
                sg.f[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s + i));
                sg.l[u].load(lab + i);
                if (v >= nvec) sg.l[u].set_positive();
            }
        };
        // one group in flight: its keys, rank_lo | count << 28 (rank_lo < 2^28: M <= 2^27 here),
        // window and query mask
        constexpr bool ONE2 = SLOT && SEC;  // one secondary window per lane per group (see SEC)
        struct Group {
            unsigned x[NQ], rc[NQ];
            uint4 k[NQ];
            uint4 k2[ONE2 ? 1 : NQ];  // the next window, for cells that run past the first
            unsigned xs;              // ONE2: the key of the query k2[0] belongs to
            unsigned use;             // bit q: query q counts; ONE2: bit 8 + q: q's cell has 5+ keys
        };
        auto keys = [&](Group& g, const Stream& sg) {
            g.use = 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float f[4] = {sg.f[u].x, sg.f[u].y, sg.f[u].z, sg.f[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool use = sg.l[u].not_positive(q);
                    g.use |= unsigned(use) << (4 * u + q);
                    g.x[4 * u + q] = key_fast(f[q]);
                    nf += use && !isfinite(f[q]);
                }
            }
            // (a slot past the end loads as positive: no use bit, so it counts no query)
            if constexpr (CHECK) nf += static_cast<unsigned>(__builtin_popcount(g.use)) << 16;
        };
        // phase by phase over the group, so that every query's LDS read of a phase is issued before
        // the first wait (a per-query chain with its conditional window load in between keeps the
        // compiler from interleaving the queries: one LDS round trip per read per query)
        auto locate_lds = [&](Group& g, unsigned (&c)[NQ]) {
            uint2 e[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) e[q] = l1[g.x[q] >> kCiLowBits];
#pragma unroll
            for (int q = 0; q < NQ; ++q) c[q] = ci_cell(g.x[q], e[q]);
            uint2 b[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) b[q] = blk[c[q] / kCiBlock];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const unsigned sh = 4u * (c[q] % kCiBlock);
                const unsigned below = __builtin_amdgcn_ubfe(b[q].y, 0u, sh);
                const unsigned bytes = (below & 0x0f0f0f0fu) + ((below >> 4) & 0x0f0f0f0fu);
                const unsigned rl = b[q].x + __builtin_amdgcn_sad_u8(bytes, 0u, 0u);
                const unsigned cnt = __builtin_amdgcn_ubfe(b[q].y, sh, 4u);
                g.rc[q] = rl | (cnt << 28);
            }
        };
        // an aligned window of +inf keys (the table is padded with at least 8 past M): the lanes with
        // no window to gather read it, so their counts need no mask
        const unsigned padoff = SLOT ? pad_word : (M32 + 3u) & ~3u;
        auto locate_win = [&](Group& g, const unsigned (&c)[NQ]) {
            if constexpr (SLOT) {
                // the cell's primary window (its first 4 keys), and its secondary one past 4 keys
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const unsigned cnt = g.rc[q] >> 28;
                    g.k[q] = win_load(sorted + (cnt && ((g.use >> q) & 1u) ? 4u * c[q] : padoff));
                }
                if constexpr (ONE2) {
                    unsigned pend = 0u;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) pend |= unsigned(((g.use >> q) & 1u) && (g.rc[q] >> 28) > 4u) << q;
                    unsigned xs = 0u, cs = 0u;
#pragma unroll
                    for (int q = NQ - 1; q >= 0; --q) {  // the lowest such query
                        xs = (pend >> q) & 1u ? g.x[q] : xs;
                        cs = (pend >> q) & 1u ? c[q] : cs;
                    }
                    g.xs = xs;
                    g.use |= pend << 8;
                    g.k2[0] = win_load(sorted + (pend ? slot_sec(slot_cells, cs) : padoff));
                } else {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const unsigned cnt = g.rc[q] >> 28;
                        g.k2[q] = win_load(sorted + (((g.use >> q) & 1u) && cnt > 4u ? slot_sec(slot_cells, c[q]) : padoff));
                    }
                }
                return;
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const unsigned rl = g.rc[q] & 0x0fffffffu, cnt = g.rc[q] >> 28;
                g.k[q] = win_load(sorted + (cnt && ((g.use >> q) & 1u) ? rl & ~3u : padoff));
            }
            // A cell that runs past its first window ((rank_lo & 3) + count > 4: ~7 % of the queries
            // at 1.1 cells per key) also loads the next one here, in the same straight-line issue: as
            // a branch after the count it was waited for with vmcnt(0) -- every load in flight,
            // the stream's included -- in nearly every iteration of every wave. Lanes that do not
            // need it read the +inf window (one shared line).
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const unsigned rl = g.rc[q] & 0x0fffffffu, cnt = g.rc[q] >> 28;
                g.k2[q] = win_load(sorted + (((g.use >> q) & 1u) && (rl & 3u) + cnt > 4u ? (rl & ~3u) + 4u : padoff));
            }
        };
        auto locate = [&](Group& g) {
            unsigned c[NQ];
            locate_lds(g, c);
            locate_win(g, c);
        };
        // ONE2: the group's secondary window, for its first query whose cell has 5+ keys (whose
        // primary window's count lacks the keys past the 4th); any further such query of the group
        // (rare) gets its secondary window now
        auto count_sec = [&](const Group& g) {
            const unsigned pend = (g.use >> 8) & 0xfu;
            unsigned les, lts;
            win_le_lt(g.k2[0], g.xs, les, lts);
            const unsigned hm = 0u - min(pend, 1u);
            w -= static_cast<unsigned long long>(les & hm);
            t += (les - lts) & hm;
            const unsigned rest = pend & (pend - 1u);
            if (__ballot(rest != 0u) != 0ull) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    if ((rest >> q) & 1u) {
                        const unsigned x = g.x[q];
                        const uint4 k2 = win_load(sorted + slot_sec(slot_cells, ci_cell(x, l1[x >> kCiLowBits])));
                        unsigned le2, lt2;
                        win_le_lt(k2, x, le2, lt2);
                        w -= le2;
                        t += le2 - lt2;
                    }
                }
            }
        };
        auto count = [&](const Group& g) {
            unsigned wl = 0u, tl = 0u;
            bool more8 = false;
            if constexpr (ONE2) count_sec(g);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                // lb = base + #(window keys < x), ub = base + #(<= x): the first window's keys before
                // the cell are < x, after it > x (or the +inf window of a lane without keys); the
                // second window (the cell's rest and later cells, or +inf) adds its own counts.
                // W += M - ub, T += ub - lb, for the queries only (um)
                const unsigned x = g.x[q], rl = g.rc[q] & 0x0fffffffu, cnt = g.rc[q] >> 28;
                const unsigned um = 0u - ((g.use >> q) & 1u);
                // rl & ~3 when the cell has keys (its window starts at the aligned rank); SLOT: the
                // window holds exactly the cell's keys, then +inf
                const unsigned base = SLOT ? rl : rl & ~(min(cnt, 1u) * 3u);
                unsigned le, lt, le2 = 0u, lt2 = 0u;
                win_le_lt(g.k[q], x, le, lt);
                if constexpr (!ONE2) win_le_lt(g.k2[q], x, le2, lt2);
                wl += (M32 - (base + le + le2)) & um;
                tl += ((le - lt) + (le2 - lt2)) & um;
                more8 |= um && (SLOT ? cnt : (rl & 3u) + cnt) > 8u;
            }
            w += wl;
            t += tl;
            if (more8) {  // a cell of 6+ keys across both windows: rare (the nibble caps it at 14)
                if constexpr (SLOT) {  // a cell of 9+ keys: its tertiary run, key by key
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const unsigned cnt = g.rc[q] >> 28;
                        if (((g.use >> q) & 1u) && cnt > 8u) {
                            const unsigned x = g.x[q];
                            slot_tertiary(x, ci_cell(x, l1[x >> kCiLowBits]), cnt, sorted, slot_cells, w, t);
                        }
                    }
                    return;
                }
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const unsigned rl = g.rc[q] & 0x0fffffffu, cnt = g.rc[q] >> 28;
                    if (((g.use >> q) & 1u) && (rl & 3u) + cnt > 8u) {
                        // undo the two windows' counts, then count the cell key by key (ci_fix)
                        const unsigned x = g.x[q];
                        const uint4 k2 = g.k2[ONE2 ? 0 : q];
                        w += (k2.x <= x) + (k2.y <= x) + (k2.z <= x) + (k2.w <= x);
                        t -= ((k2.x <= x) + (k2.y <= x) + (k2.z <= x) + (k2.w <= x)) -
                             ((k2.x < x) + (k2.y < x) + (k2.z < x) + (k2.w < x));
                        ci_fix(x, rl, cnt, g.k[q], sorted, w, t);
                    }
                }
            }
        };
        // per group g: keys(g) [its stream loads were issued D groups earlier], stream loads of
        // g + D into the buffer just read, LDS lookups + window loads of g, count of g - 1 [its
        // windows were issued one group earlier; the younger loads stay in flight: vmcnt retires
        // in order]. D stream buffers keep D groups of score/label loads in flight per lane: with
        // one (D = 1) a wave holds 20 B per lane in flight, 5 MB over the chip, which at HBM's
        // loaded latency caps the stream far below the bandwidth.
        // (round 6: D = 2 for the slotted form with a secondary window per query needs 128 VGPRs +
        // 144-200 B of scratch per lane; with SEC's one secondary window per group it fits in 119-123
        // VGPRs for 1- and 4-byte labels, but ran 0.3-0.5 % slower at 2^27 and the same at 2^24)
        constexpr int D = 1;
        // groups in flight (windows issued GD - 1 groups before their count; round 6 measured 3 with
        // SEC: 127-128 VGPRs, the same time as 2 -- more loads in flight do not help)
        constexpr int GD = 2;
        static_assert(GD == 2 || (GD == 3 && D == 1), "the pipeline's unroll");
        constexpr int L = GD == 3 ? 3 : D % 2 == 0 ? D : 2 * D;  // unroll: every buffer index compile-time
        Stream sbuf[D];
        Group gbuf[GD];
#pragma unroll
        for (int j = 0; j < D; ++j) load(sbuf[j], tid + int64_t(j) * step);
#pragma unroll
        for (int p = 0; p < GD - 1; ++p) {  // groups 0 .. GD - 2 located (a group past the end counts nothing)
            keys(gbuf[p], sbuf[p % D]);
            load(sbuf[p % D], tid + int64_t(p + D) * step);
            locate(gbuf[p]);
        }
        int64_t v = tid + int64_t(GD - 1) * step;
        for (;;) {
#pragma unroll
            for (int j = 0; j < L; ++j) {
                // group v sits in stream buffer (j + GD - 1) % D and group slot (j + GD - 1) % GD
                Group& gc = gbuf[(j + GD - 1) % GD];
                Group& gp = gbuf[j % GD];
                if (v >= nvec) {
#pragma unroll
                    for (int p = 0; p < GD - 1; ++p) count(gbuf[(j + p) % GD]);
                    goto ci_stream_done;
                }
                keys(gc, sbuf[(j + GD - 1) % D]);
                load(sbuf[(j + GD - 1) % D], v + int64_t(D) * step);
                asm volatile("" ::: "memory");  // the stream loads stay older than this group's windows
                locate(gc);
                count(gp);
                v += step;
            }
        }
    ci_stream_done:;
    } else {
        for (int64_t v = tid; v < nvec; v += stride)
            for (int q = 0; q < 4; ++q) one(head + v * 4 + q);
    }
    for (int64_t i = head + nvec * 4 + tid; i < end; i += stride) one(i);
    // one atomic per workgroup and word: per-wave atomics on one address serialise across the
    // XCDs (~15 ns each: 4096 of them cost ~60 us)
    w = wave_sum(w);
    t = wave_sum(t);
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    unsigned long long ckw = 0;
    if constexpr (CHECK) {
        ckw = wave_sum(static_cast<unsigned long long>(nf >> 16));
        nf &= 0xffffu;
    }
    const unsigned long long nfw = wave_sum(static_cast<unsigned long long>(nf));
    if (lane == 0) {
        red[0][wid] = w;
        red[1][wid] = t;
        red[2][wid] = nfw;
        if constexpr (CHECK) red[CHECK ? 3 : 0][wid] = ckw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long bw = 0, bt = 0, bn = 0, bc = 0;
        for (int i = 0; i < kQueryThreads / kWave; ++i) {
            bw += red[0][i];
            bt += red[1][i];
            bn += red[2][i];
            if constexpr (CHECK) bc += red[CHECK ? 3 : 0][i];
        }
        if (red8 == nullptr) {
            if (bw) atomicAdd(out + 0, bw);
            if (bt) atomicAdd(out + 1, bt);
            if (bn && nonfinite) atomicAdd(nonfinite, bn);
            if (CHECK && bc) atomicAdd(check, static_cast<unsigned>(bc));
        } else {
            // round 6 (the two-step's query pass): its workgroups finish together, and 3-4 atomics
            // each on the record's one line serialise (~8 us at 256 workgroups and 2^21 queries,
            // measured by an ablation since removed; the one-call pass, 8x the queries per workgroup, measured 1 us
            // slower with the groups and keeps the plain atomics). Group g = blockIdx % 8 adds into
            // its own line of red8 (256 B apart; zeroed by the count pass before this launch), takes
            // the group's ticket after its adds are acknowledged, and the group's last arriver adds
            // the group's sums to the record: <= 8 atomics per record word, 8 chains in parallel
            const unsigned g = blockIdx.x & 7u;
            unsigned long long* L = red8 + 32u * g;
            if (bw) atomicAdd(L + 0, bw);
            if (bt) atomicAdd(L + 1, bt);
            if (bn) atomicAdd(L + 2, bn);
            if (CHECK && bc) atomicAdd(L + 3, bc);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned members = (gridDim.x - g + 7u) / 8u;
            const unsigned tk = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(L + 4), 1u, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
            if (tk == members - 1u) {
                const unsigned long long gw = __hip_atomic_load(L + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long gt = __hip_atomic_load(L + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long gn = __hip_atomic_load(L + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long gc =
                    CHECK ? __hip_atomic_load(L + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
                if (gw) atomicAdd(out + 0, gw);
                if (gt) atomicAdd(out + 1, gt);
                if (gn && nonfinite) atomicAdd(nonfinite, gn);
                if (CHECK && gc) atomicAdd(check, static_cast<unsigned>(gc));
            }
        }
    }
}

// the one place an instantiation is chosen: CHECK by the check word, SLOT by the slotted table's
// byte counts; SEC is only instantiated true (the carried secondary window)
template <typename LT>
auto pick_query(bool check, bool slot) -> decltype(&query_ci_kernel<LT>) {
    if (slot) return check ? &query_ci_kernel<LT, true, true, true> : &query_ci_kernel<LT, false, true, true>;
    return check ? &query_ci_kernel<LT, true> : &query_ci_kernel<LT>;
}

// `lab` is q.labels with its element type
template <typename LT>
int launch_ci_typed(const LabeledQueries& q, const LT* lab, const CountWs& cw, const unsigned* table, int64_t M,
                    hipStream_t st, const CiForm& f) {
    const dim3 grid(query_grid(q.end - q.begin)), block(kQueryThreads);
    const size_t lds = (size_t(kCiTop) + kCiMaxBlocks) * 8 + (f.grp ? size_t(kDirectMaxGroups) * 4 : 0);
    // dynamic + the kernel's static reduction rows must fit the CU's 160 KB of LDS (a launch past it
    // aborts the queue: HSA_STATUS_ERROR_INVALID_ALLOCATION)
    static_assert((size_t(kCiTop) + kCiMaxBlocks) * 8 + size_t(kDirectMaxGroups) * 4 +
                          4 * (kQueryThreads / kWave) * 8 <= 160 * 1024,
                  "the count-index query's LDS");
    const bool slot = f.slot_counts != nullptr;
    hipLaunchKernelGGL(pick_query<LT>(f.check != nullptr, slot), grid, block, lds, st, q.scores, lab, q.begin, q.end,
                       cw.meta, cw.l1, slot ? f.slot_counts : cw.blk, table, M, q.wins_ties, q.nonfinite, f.verdict,
                       f.grp, f.Mp, f.check, f.slot_cells, f.red8);
    return launch_status();
}

}  // namespace

int launch_ci(const LabeledQueries& q, const CountWs& cw, const unsigned* table, int64_t M, hipStream_t st,
              const CiForm& form) {
    return with_labels(q.labels, q.label_dtype,
                       [&](auto* lab) { return launch_ci_typed(q, lab, cw, table, M, st, form); });
}

}  // namespace dauc
