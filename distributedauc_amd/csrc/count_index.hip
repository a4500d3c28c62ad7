// The count index (count_index.h) built straight from the unsorted positives, and the evaluation's
// entry points behind it.
//
// The product's hot path, top to bottom: the compaction (auc_count.hip) has left the positives, their
// top-bucket histogram and a +inf-filled slotted table; ONE count pass here --
// direct_count_kernel<true> for the one-call evaluation (counts_labeled_direct_slotted, reached from
// dauc_auc_eval_counts / dauc_auc_eval_enqueue), direct_count_slots_kernel<true> for the two-step
// one (counts_labeled_slotted, from dauc_auc_eval_query_part) -- plans the cells and inserts every
// key into its cell's slot; then the query pass (count_query.hip, launch_ci).
// Behind it: round 5's direct build (the <false> forms of the two count kernels, then the blocks and
// scatter passes into a cell-ordered table: counts_labeled_direct, counts_labeled_direct_slots; a
// tuning build's dauc_set_index_form(1)) and its fault injection (dauc_set_direct_fault).

#include "auc_eval_internal.h"

namespace dauc {
namespace {

// ---- the count index built straight from the unsorted table (the one-call evaluation) -------
//
// The count index needs the table ordered by CELL only: ci_count and ci_fix count a cell's keys
// whatever their order (keys of earlier cells are < x, of later cells > x). So the one-call
// evaluation skips the radix sort and the tree: a top-bucket histogram, the plan, per-cell counts,
// the block words and their prefix, and a scatter of every key into its cell's range -- 6 small
// launches over the table instead of 8 sort launches + the tree + the 4-launch build behind a
// sort. The table is not sorted inside a cell, so the tree cannot fall back on it: when the plan
// or the block pass finds the table unusable (more than 1.5 keys per cell, a cell of 15+ keys)
// the query kernel reports it (*verdict = 2) and the caller re-runs the sorted path.
constexpr int kDirectPerThread = 8;

// The slotted build's insertion (count_index.h), one key per live lane; every lane of the wave
// calls it. The key's rank in its cell is the byte its returning add on the cell's packed counter
// found (a wave whose keys all fall in one cell -- tie-heavy tables -- adds once and ranks its lanes
// itself); ranks 0-3 go to the primary window, 4-7 to the secondary, 8-13 to the tertiary run.
// Returns true for a key past 14 in its cell (the caller marks the index skewed; a byte past 255
// also carries into the next cell's counter: skewed anyway).
__device__ __forceinline__ bool slot_insert(unsigned x, unsigned c, bool live, unsigned* __restrict__ cnt,
                                            unsigned* __restrict__ stab, unsigned cells, int lane) {
    const unsigned long long act = __ballot(live);
    if (act == 0ull) return false;
    const int first = __ffsll(static_cast<long long>(act)) - 1;
    const unsigned cf = __shfl(c, first, kWave);
    unsigned rank = 0u;
    if (__ballot(live && c == cf) == act) {
        unsigned old = 0u;
        if (lane == first) old = atomicAdd(cnt + (cf >> 2), static_cast<unsigned>(__popcll(act)) << (8u * (cf & 3u)));
        old = __shfl(old, first, kWave);
        const unsigned below = static_cast<unsigned>(__popcll(act & (lane == 0 ? 0ull : (~0ull >> (kWave - lane)))));
        rank = ((old >> (8u * (cf & 3u))) & 0xffu) + below;
    } else if (live) {
        const unsigned old = atomicAdd(cnt + (c >> 2), 1u << (8u * (c & 3u)));
        rank = (old >> (8u * (c & 3u))) & 0xffu;
    }
    if (!live) return false;
    if (rank < 4u) stab[4u * c + rank] = x;
    else if (rank < 8u) stab[slot_sec(cells, c) + rank - 4u] = x;
    else if (rank < kSlotMaxKeys) stab[slot_ter(cells, c) + rank - 8u] = x;
    else return true;
    return false;
}

// The plan of ci_plan_kernel from the bucket sizes themselves, computed by EVERY workgroup of the
// count pass in LDS (2048 buckets, 8 per thread: cheaper than a one-workgroup launch between the
// histogram and the counts): C_t = ceil(n_t * num / M) cells per used bucket, num = min(cells left
// after one per used bucket, 2 M), the first cell of every bucket (ascending). Workgroup 0 also
// writes the plan and the verdict words for the later passes. Then the per-cell key counts (a wave
// whose keys all fall in one cell adds once: tie-heavy tables) and every key's cell.

// SLOT (round 6, the one-call evaluation's default): every key inserted into the cell-slotted
// table instead (slot_insert; the compaction prepared the table, the packed counters and meta).
template <bool SLOT = false>
__global__ __launch_bounds__(kDirectThreads) void direct_count_kernel(const float* __restrict__ pos, int64_t mcap,
                                                                      const unsigned* __restrict__ hist,
                                                                      uint2* __restrict__ l1g,
                                                                      unsigned* __restrict__ meta,
                                                                      unsigned* __restrict__ cnt,
                                                                      unsigned* __restrict__ cell,
                                                                      unsigned* __restrict__ stab = nullptr,
                                                                      unsigned slot_cells = 0u,
                                                                      const unsigned long long* __restrict__ Mp =
                                                                          nullptr) {
    static_assert(kCiTop == 8 * kDirectThreads, "eight top buckets per thread");
    __shared__ uint2 l1[kCiTop];
    __shared__ unsigned wtot[kDirectThreads / kWave];
    __shared__ unsigned totals[3];
    // Mp (round 6, the slotted one-call form): the compaction's P, which is the histogram's total
    // (every positive is in it) -- loaded with the histogram, so only the used buckets are summed
    // (eight ballots per wave, one LDS sum) and the plan needs one workgroup scan instead of three
    const unsigned long long Mdev = Mp != nullptr ? *Mp : 0ull;
    const uint4 h0 = reinterpret_cast<const uint4*>(hist)[2 * threadIdx.x];
    const uint4 h1 = reinterpret_cast<const uint4*>(hist)[2 * threadIdx.x + 1];
    const unsigned n[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
    int64_t M, used_total;
    if (Mp != nullptr) {  // (uniform)
        const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
        unsigned wu = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) wu += static_cast<unsigned>(__popcll(__ballot(n[j] != 0u)));
        if (lane == 0) wtot[wid] = wu;
        __syncthreads();
        unsigned u = 0u;
#pragma unroll
        for (int w = 0; w < kDirectThreads / kWave; ++w) u += wtot[w];
        __syncthreads();  // (wtot is the next scan's)
        M = static_cast<int64_t>(Mdev);
        used_total = u;
    } else {
        unsigned used = 0u, keys = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            used += n[j] != 0u;
            keys += n[j];
        }
        used = block_incl_scan1024<false>(used, wtot);
        if (threadIdx.x == kDirectThreads - 1) totals[0] = used;
        keys = block_incl_scan1024<false>(keys, wtot);  // M = the histogram's total (< 2^32: M <= n / 2)
        if (threadIdx.x == kDirectThreads - 1) totals[2] = keys;
        __syncthreads();
        M = totals[2];
        used_total = totals[0];
    }
    const int64_t avail = int64_t(kCiMaxCells) - used_total;
    const int64_t num = avail < 2 * M ? avail : 2 * M;
    unsigned C[8], csum = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        C[j] = n[j] ? static_cast<unsigned>((int64_t(n[j]) * num + M - 1) / M) : 0u;
        csum += C[j];
    }
    const unsigned incl = block_incl_scan1024<false>(csum, wtot);
    if (threadIdx.x == kDirectThreads - 1) totals[1] = incl;
    unsigned run = incl - csum;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        l1[8 * threadIdx.x + j] = uint2{run, C[j]};
        run += C[j];
    }
    __syncthreads();
    const unsigned total = totals[1];
    // usable: at most 1.5 keys per cell, and the table fits the workspace (M <= mcap)
    const bool ok = num > 0 && 3 * num >= 2 * M && total <= static_cast<unsigned>(kCiMaxCells) && M <= mcap;
    if (blockIdx.x == 0) {
        for (int t = threadIdx.x; t < kCiTop; t += kDirectThreads) l1g[t] = l1[t];
        // SLOT: `cell` is unused as such; it holds the query pass's 8 group lines (query_ci_kernel's
        // red8: 2 KB), zeroed here, before that launch
        if (SLOT && cell != nullptr && threadIdx.x < 256)
            reinterpret_cast<unsigned long long*>(cell)[threadIdx.x] = 0ull;
        if (threadIdx.x == 0) {
            meta[kCiOk] = ok ? 1u : 0u;
            meta[kCiCells] = total;
            meta[kCiBlocks] = (total + 1 + kCiBlock - 1) / kCiBlock;
            if constexpr (!SLOT) meta[kCiSkew] = 0u;  // SLOT: zeroed by the compaction (set by any workgroup)
        }
    }
    if (!ok) return;
    const int lane = threadIdx.x & (kWave - 1);
    if constexpr (SLOT) {
        bool skew = false;
        for (int64_t i0 = int64_t(blockIdx.x) * kDirectThreads; i0 < M; i0 += int64_t(gridDim.x) * kDirectThreads) {
            const int64_t i = i0 + threadIdx.x;
            const bool live = i < M;
            unsigned x = 0u, c = 0u;
            if (live) {
                x = key_fast(pos[i]);
                c = ci_cell(x, l1[x >> kCiLowBits]);
            }
            skew |= slot_insert(x, c, live, cnt, stab, slot_cells, lane);
        }
        if (__ballot(skew) != 0ull && lane == 0) atomicOr(meta + kCiSkew, 1u);
        return;
    }
    for (int64_t i0 = int64_t(blockIdx.x) * kDirectThreads; i0 < M; i0 += int64_t(gridDim.x) * kDirectThreads) {
        const int64_t i = i0 + threadIdx.x;
        const bool live = i < M;
        unsigned c = 0u;
        if (live) {
            const unsigned x = key_fast(pos[i]);
            c = ci_cell(x, l1[x >> kCiLowBits]);
            cell[i] = c;  // the scatter's cell, so it does not walk pos -> key -> plan again
        }
        const unsigned long long act = __ballot(live);
        if (act == 0ull) continue;
        const int first = __ffsll(static_cast<long long>(act)) - 1;
        const unsigned cf = __shfl(c, first, kWave);
        if (__ballot(live && c == cf) == act) {
            if (lane == first) atomicAdd(cnt + cf, static_cast<unsigned>(__popcll(act)));
        } else if (live) {
            atomicAdd(cnt + c, 1u);
        }
    }
}

// The two-step evaluation's count pass straight from the gathered slots (the gather copy folded
// in): every workgroup sums the slots' headers (wave 0: the stored scores' prefix per slot) and
// their histograms (two top buckets per thread), computes the plan as direct_count_kernel does,
// and counts its keys -- each key read from its slot, copied to the table position array `pos`
// (the scatter's input) with its cell. Workgroup 0 also writes the plan, the verdict words, the
// part's record (counts zeroed, P, the check word, the label counts) and m_eff (P, or past the
// index's capacity when a slot overflowed, so the plan refuses the table: verdict 2).
//
// SLOT (round 6, the two-step evaluation's default): the cell-slotted table instead (count_index.h:
// primary / secondary windows +inf filled by the compaction of step 1, a tertiary run), the per-cell
// counters bytes packed four to a word (zeroed by that compaction too), and each key inserted
// straight into its cell: its rank in the cell is the byte its returning atomic add found. No
// position array, no cell array, no block pass and no scatter: the query pass turns the byte counts
// into the block words itself (query_ci_kernel<.., SLOT>). A cell of 15+ keys marks the index skewed
// (verdict 2: the caller's sorted path), as in the direct build; meta[kCiSkew] was zeroed by the
// compaction, because this pass's workgroups set it while workgroup 0 writes the other meta words.
constexpr int kSlotCountThreads = 1024;
template <bool SLOT = false>
__global__ __launch_bounds__(kSlotCountThreads) void direct_count_slots_kernel(SlotSource src, int64_t mcap,
                                                                              uint2* __restrict__ l1g,
                                                                              unsigned* __restrict__ meta,
                                                                              unsigned* __restrict__ cnt,
                                                                              unsigned* __restrict__ cell,
                                                                              float* __restrict__ pos,
                                                                              unsigned* __restrict__ stab,
                                                                              unsigned slot_cells) {
    static_assert(kCiTop == 2 * kSlotCountThreads, "two top buckets per thread");
    __shared__ uint2 l1[kCiTop];
    __shared__ unsigned wtot[kSlotCountThreads / kWave];
    __shared__ unsigned totals[3];
    __shared__ unsigned long long off[kMaxSlotParts + 1];  // stored scores before slot r
    __shared__ unsigned long long hs[5];                   // P, #non-finite, #other, overflow, check
    const int parts = src.parts;
    const int lane = threadIdx.x & (kWave - 1);
    auto hdr = [&](int r) { return reinterpret_cast<const unsigned long long*>(src.slots + size_t(r) * src.sbytes); };
    const unsigned long long cap = static_cast<unsigned long long>(src.cap);
    // the summed histogram: buckets 2t, 2t + 1 -- every slot's load issued before the header work
    // (8 loads in flight per thread: one L2 round trip, not one per slot)
    unsigned n0 = 0u, n1 = 0u;
    {
        const uint2* hp = reinterpret_cast<const uint2*>(src.slots + src.hist_off) + threadIdx.x;
        const size_t sw = src.sbytes / sizeof(uint2);
        int r = 0;
        for (; r + 8 <= parts; r += 8) {
            uint2 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = hp[size_t(r + j) * sw];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                n0 += v[j].x;
                n1 += v[j].y;
            }
        }
        for (; r < parts; ++r) {
            const uint2 v = hp[size_t(r) * sw];
            n0 += v.x;
            n1 += v.y;
        }
    }
    if (threadIdx.x < kWave) {
        unsigned long long run = 0, P = 0, nf = 0, other = 0, mism = 0;
        bool over = false;
        for (int r0 = 0; r0 < parts; r0 += kWave) {
            const int r = r0 + lane;
            unsigned long long stored = 0;
            if (r < parts) {
                const unsigned long long* h = hdr(r);
                const unsigned long long pr = h[0];
                P += pr;
                nf += h[2];
                other += h[3];
                mism += h[4] != static_cast<unsigned long long>(src.n);
                over |= pr > cap;
                stored = pr < cap ? pr : cap;
            }
            unsigned long long inc = stored;
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const unsigned long long t = __shfl_up(inc, d, kWave);
                if (lane >= d) inc += t;
            }
            if (r < parts) off[r] = run + inc - stored;
            run += __shfl(inc, kWave - 1, kWave);
        }
        P = wave_sum(P);
        nf = wave_sum(nf);
        other = wave_sum(other);
        mism = wave_sum(mism);
        over = __ballot(over) != 0ull;
        if (lane == 0) {
            off[parts] = run;
            hs[0] = P;
            hs[1] = nf;
            hs[2] = other;
            hs[3] = over ? 1ull : 0ull;
            // the check word: the queried slot's P - the range length (low half, mod 2^32; the
            // query pass adds its queries), the slots built for another n (high half)
            const unsigned long long* q = hdr((src.part + 1) % parts);
            const unsigned lo = static_cast<unsigned>(q[0]) - static_cast<unsigned>(src.qlen);
            hs[4] = (mism << 32) | lo;
        }
    }
    __syncthreads();  // (an overflow adds past-capacity keys to bucket 0)
    // SLOT: this thread's first key is loaded now, so its latency overlaps the plan's three scans
    // (one key per thread: the grid covers the index's capacity)
    const int64_t i_first = int64_t(blockIdx.x) * kSlotCountThreads + threadIdx.x;
    float v_first = 0.0f;
    if constexpr (SLOT) {
        if (hs[3] == 0ull && i_first < static_cast<int64_t>(hs[0])) {
            int lo = 0, hi = parts;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (off[mid] <= static_cast<unsigned long long>(i_first)) lo = mid;
                else hi = mid;
            }
            v_first = reinterpret_cast<const float*>(src.slots + size_t(lo) * src.sbytes + src.data_off)
                [i_first - static_cast<int64_t>(off[lo])];
        }
    }
    const bool over = hs[3] != 0ull;
    if (threadIdx.x == 0 && over) n0 += static_cast<unsigned>(mcap) + 1u;
    // round 6: only the totals of the used buckets and of the keys are needed, not their scans: the
    // used buckets by two ballots per wave and one LDS sum, and the keys = the slots' P (every
    // positive is in its slot's histogram, stored or not; an overflow adds the past-capacity count,
    // as the overflow bucket did, so the plan refuses the table) -- two workgroup scans fewer
    {
        const int wid = threadIdx.x / kWave;
        const unsigned wu = static_cast<unsigned>(__popcll(__ballot(n0 != 0u)) + __popcll(__ballot(n1 != 0u)));
        if (lane == 0) wtot[wid] = wu;
    }
    __syncthreads();
    unsigned used_total = 0u;
#pragma unroll
    for (int w = 0; w < kSlotCountThreads / kWave; ++w) used_total += wtot[w];
    __syncthreads();  // (wtot is the next scan's)
    const int64_t M = static_cast<int64_t>(hs[0]) + (over ? mcap + 1 : 0);
    const int64_t avail = int64_t(kCiMaxCells) - int64_t(used_total);
    const int64_t num = avail < 2 * M ? avail : 2 * M;
    const unsigned C0 = n0 ? static_cast<unsigned>((int64_t(n0) * num + M - 1) / M) : 0u;
    const unsigned C1 = n1 ? static_cast<unsigned>((int64_t(n1) * num + M - 1) / M) : 0u;
    const unsigned incl = block_incl_scan1024<false>(C0 + C1, wtot);
    if (threadIdx.x == kSlotCountThreads - 1) totals[1] = incl;
    const unsigned run = incl - (C0 + C1);
    l1[2 * threadIdx.x] = uint2{run, C0};
    l1[2 * threadIdx.x + 1] = uint2{run + C0, C1};
    __syncthreads();
    const unsigned total = totals[1];
    const bool ok = num > 0 && 3 * num >= 2 * M && total <= static_cast<unsigned>(kCiMaxCells) && M <= mcap;
    const unsigned long long P = hs[0];
    if (blockIdx.x == 0) {
        l1g[2 * threadIdx.x] = l1[2 * threadIdx.x];
        l1g[2 * threadIdx.x + 1] = l1[2 * threadIdx.x + 1];
        // SLOT: `cell` holds the query pass's 8 group lines (query_ci_kernel's red8), zeroed here
        if (SLOT && cell != nullptr && threadIdx.x < 256)
            reinterpret_cast<unsigned long long*>(cell)[threadIdx.x] = 0ull;
        if (threadIdx.x == 0) {
            meta[kCiOk] = ok ? 1u : 0u;
            meta[kCiCells] = total;
            meta[kCiBlocks] = (total + 1 + kCiBlock - 1) / kCiBlock;
            if constexpr (!SLOT) meta[kCiSkew] = 0u;  // SLOT: zeroed by the compaction (see above)
            *src.m_eff = over ? static_cast<unsigned long long>(mcap) + 1ull : P;
        } else if (threadIdx.x < 4) {
            src.wt[threadIdx.x - 1] = 0ull;
        } else if (threadIdx.x == 4) {
            *src.verdict = 0ull;
        } else if (threadIdx.x < 9) {
            const int k = threadIdx.x - 5;  // stats: P, check, #non-finite, #other
            src.stats[k] = k == 0 ? P : k == 1 ? hs[4] : hs[k - 1];  // hs: P, #non-finite, #other, .., check
        }
    }
    if (!ok) return;
    const int64_t Mk = static_cast<int64_t>(P);  // no overflow here: every positive is stored
    if constexpr (SLOT) {
        // step 2 again on the same step-1 state: the counters and slots already hold the keys, so
        // inserting them twice would double every count -- refuse the index instead (verdict 2:
        // the caller's sorted path gives the exact integers)
        if (meta[kCiConsumed] != 0u) {
            if (threadIdx.x == 0) atomicOr(meta + kCiSkew, 1u);
            return;
        }
        bool skew = false;
        for (int64_t i0 = int64_t(blockIdx.x) * kSlotCountThreads; i0 < Mk;
             i0 += int64_t(gridDim.x) * kSlotCountThreads) {
            const int64_t i = i0 + threadIdx.x;
            const bool live = i < Mk;
            unsigned x = 0u, c = 0u;
            if (live) {
                float v = v_first;
                if (i != i_first) {  // past the first key (a grid smaller than the table)
                    int lo = 0, hi = parts;
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (off[mid] <= static_cast<unsigned long long>(i)) lo = mid;
                        else hi = mid;
                    }
                    v = reinterpret_cast<const float*>(src.slots + size_t(lo) * src.sbytes + src.data_off)
                        [i - static_cast<int64_t>(off[lo])];
                }
                x = key_fast(v);
                c = ci_cell(x, l1[x >> kCiLowBits]);
            }
            skew |= slot_insert(x, c, live, cnt, stab, slot_cells, lane);
        }
        if (__ballot(skew) != 0ull && lane == 0) atomicOr(meta + kCiSkew, 1u);
        return;
    }
    for (int64_t i0 = int64_t(blockIdx.x) * kSlotCountThreads; i0 < Mk;
         i0 += int64_t(gridDim.x) * kSlotCountThreads) {
        const int64_t i = i0 + threadIdx.x;
        const bool live = i < Mk;
        unsigned c = 0u;
        if (live) {
            // the slot holding key i: the last r with off[r] <= i (binary search over the prefix)
            int lo = 0, hi = parts;  // off[lo] <= i < off[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (off[mid] <= static_cast<unsigned long long>(i)) lo = mid;
                else hi = mid;
            }
            const float v = reinterpret_cast<const float*>(src.slots + size_t(lo) * src.sbytes + src.data_off)
                [i - static_cast<int64_t>(off[lo])];
            pos[i] = v;
            const unsigned x = key_fast(v);
            c = ci_cell(x, l1[x >> kCiLowBits]);
            cell[i] = c;
        }
        const unsigned long long act = __ballot(live);
        if (act == 0ull) continue;
        const int first = __ffsll(static_cast<long long>(act)) - 1;
        const unsigned cf = __shfl(c, first, kWave);
        if (__ballot(live && c == cf) == act) {
            if (lane == first) atomicAdd(cnt + cf, static_cast<unsigned>(__popcll(act)));
        } else if (live) {
            atomicAdd(cnt + c, 1u);
        }
    }
}

// ---- round 5's direct build: histogram, blocks, scatter (behind the <false> count passes) ------

// top-bucket histogram (LDS, then one global add per used bucket; `hist` zeroed by the caller);
// also zeroes the per-cell counters the count pass adds into
// The table size M is read from the device (the compaction's count), so the whole build and query
// are enqueued without the host knowing M: the grids are sized for the index's capacity and loop.
__global__ __launch_bounds__(256) void direct_hist_kernel(const float* __restrict__ pos,
                                                          const unsigned long long* __restrict__ Mp,
                                                          unsigned* __restrict__ hist, unsigned* __restrict__ cnt,
                                                          int64_t ncnt) {
    const int64_t M = static_cast<int64_t>(*Mp);
    __shared__ unsigned h[kCiTop];
    for (int i = threadIdx.x; i < kCiTop; i += 256) h[i] = 0u;
    __syncthreads();
    const int64_t gid = int64_t(blockIdx.x) * 256 + threadIdx.x, stride = int64_t(gridDim.x) * 256;
    for (int64_t i = gid; i < ncnt; i += stride) cnt[i] = 0u;
    for (int64_t i = gid; i < M; i += stride) atomicAdd(&h[key_fast(pos[i]) >> kCiLowBits], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < kCiTop; i += 256)
        if (h[i]) atomicAdd(hist + i, h[i]);
}

// One thread per block of 8 cells, one workgroup per group of 256 blocks: blk[b] = {the table
// keys before block b within its group, the 8 cells' counts as nibbles}, grp[g] = the group's
// keys; a count of 15 or more marks the table skewed. The consumers add the groups' prefix
// (group_prefix), so no one-workgroup scan launch sits between this pass and the scatter.
__global__ __launch_bounds__(kDirectGroup) void direct_blocks_kernel(const unsigned* __restrict__ cnt,
                                                                     unsigned* __restrict__ meta,
                                                                     uint2* __restrict__ blk,
                                                                     unsigned* __restrict__ grp) {
    if (meta[kCiOk] == 0u) return;
    __shared__ unsigned wtot[kDirectGroup / kWave];
    const int b = blockIdx.x * kDirectGroup + threadIdx.x;
    const bool live = b < static_cast<int>(meta[kCiBlocks]);
    bool skew = false;
    unsigned w = 0u, sum = 0u;
    if (live) {
        const uint4 lo = reinterpret_cast<const uint4*>(cnt)[2 * b], hi = reinterpret_cast<const uint4*>(cnt)[2 * b + 1];
        const unsigned c[kCiBlock] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int j = 0; j < kCiBlock; ++j) {
            skew |= c[j] >= 15u;
            w |= (c[j] < 15u ? c[j] : 15u) << (4 * j);
            sum += c[j];
        }
    }
    const unsigned incl = block_incl_scan1024<false>(sum, wtot);
    if (live) blk[b] = uint2{incl - sum, w};
    if (threadIdx.x == kDirectGroup - 1) grp[blockIdx.x] = incl;
    if (__ballot(skew) != 0ull && (threadIdx.x & (kWave - 1)) == 0) atomicOr(meta + kCiSkew, 1u);
}

// every key into its cell's range of the table (the counters are counted back down to zero);
// the table's tail is padded with +inf keys for the 16-byte windows
__global__ __launch_bounds__(kDirectThreads) void direct_scatter_kernel(const float* __restrict__ pos,
                                                                        const unsigned long long* __restrict__ Mp,
                                                                        const uint2* __restrict__ blk,
                                                                        const unsigned* __restrict__ grp,
                                                                        unsigned* __restrict__ meta,
                                                                        unsigned* __restrict__ cnt,
                                                                        const unsigned* __restrict__ cell,
                                                                        unsigned* __restrict__ table,
                                                                        int64_t ncnt) {
    if (meta[kCiOk] == 0u) return;  // nothing was counted: the counters are still zero
    if (meta[kCiSkew] != 0u) {
        // a skewed table: no scatter, but the counters go back to zero for the next build (the
        // scatter of a good build counts them down to zero itself)
        for (int64_t i = int64_t(blockIdx.x) * kDirectThreads + threadIdx.x; i < ncnt;
             i += int64_t(gridDim.x) * kDirectThreads)
            cnt[i] = 0u;
        return;
    }
    const int64_t M = static_cast<int64_t>(*Mp);
    __shared__ unsigned pre[kDirectMaxGroups];
    group_prefix(grp, (static_cast<int>(meta[kCiBlocks]) + kDirectGroup - 1) / kDirectGroup, pre);
    __syncthreads();
    const int64_t gid = int64_t(blockIdx.x) * kDirectThreads + threadIdx.x;
    if (gid < 16) table[M + gid] = kPadKey;
    // Every index is checked before it is used (a producer bug must become a verdict-2 fallback,
    // never an out-of-bounds store): the cell must be one of the plan's, and its counter must still
    // hold a slot (the count pass counted exactly this many keys into it). A failed check marks the
    // index skewed, so the query passes return at once and the caller takes the sorted path.
    const unsigned ncells = meta[kCiCells];
    bool bad = false;
    for (int64_t i = gid; i < M; i += int64_t(gridDim.x) * kDirectThreads) {
        const unsigned x = key_fast(pos[i]);
        const unsigned c = cell[i];
        if (c >= ncells) {
            bad = true;
            continue;
        }
        const unsigned bi = c / kCiBlock;
        unsigned rl, ccount;
        ci_decode(c, blk[bi], rl, ccount);
        const unsigned left = atomicSub(cnt + c, 1u);  // slots of the cell not yet taken, before this one
        if (left == 0u || left > ccount) {
            bad = true;
            continue;
        }
        const unsigned pos_in_table = pre[bi / kDirectGroup] + rl + (left - 1u);
        if (pos_in_table >= static_cast<unsigned>(M)) {
            bad = true;
            continue;
        }
        table[pos_in_table] = x;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & (kWave - 1)) == 0) atomicOr(meta + kCiSkew, 1u);
}

// The count and scatter passes loop over the keys (up to 1024 workgroups; 256 measured the same:
// profiles/r04/query_ablations/r04q_*)
constexpr int64_t kDirectGrid = 1024;

}  // namespace

int64_t direct_capacity(int64_t n) {
    // the plan's bound (2 M <= 3 cells), and the smaller class of n scores (the evaluation's
    // workspace holds a table of n / 2 + 1 keys)
    const int64_t cap = 3 * int64_t(kCiMaxCells) / 2, half = n / 2 + 1;
    return half < cap ? half : cap;
}

unsigned* direct_cnt_ptr(void* workspace, int64_t Mcap) { return sort_workspace(workspace, Mcap).count.cstart; }

int64_t direct_cnt_words() { return kCiCntWords; }

int64_t direct_hist_offset(int64_t Mcap) {  // the count index's `first`, relative to the workspace
    return static_cast<int64_t>(reinterpret_cast<uintptr_t>(sort_workspace(nullptr, Mcap).count.first));
}

#ifdef DAUC_TUNING
// Tuning builds: dauc_set_direct_fault corrupts the direct build between its count and scatter
// passes, so a test can check that the scatter's index checks turn a producer bug into a verdict-2
// fallback (include/dauc_tuning.h): 1 = one key's cell past the plan's last cell, 2 = one key moved
// to the next cell (that cell's counter runs out), 3 = one cell's counter one above its count.
int g_direct_fault = 0;

__global__ void direct_fault_kernel(int mode, const unsigned long long* __restrict__ Mp,
                                    const unsigned* __restrict__ meta, unsigned* __restrict__ cnt,
                                    unsigned* __restrict__ cell) {
    const int64_t M = static_cast<int64_t>(*Mp);
    if (threadIdx.x != 0 || meta[kCiOk] == 0u || M == 0) return;
    const int64_t i = M / 2;
    const unsigned ncells = meta[kCiCells], c = cell[i];
    if (mode == 1) cell[i] = ncells + 7u;
    if (mode == 2) cell[i] = c + 1u < ncells ? c + 1u : 0u;
    if (mode == 3) cnt[c] += 1u;
}
#endif

int build_direct_index(const float* pos, const unsigned long long* Mp, int64_t Mcap, void* workspace,
                       size_t workspace_bytes, hipStream_t st, DirectIndex* ix, const unsigned* ready_hist) {
    if (pos == nullptr || Mp == nullptr || Mcap < 1 || workspace == nullptr || ix == nullptr ||
        workspace_bytes < dauc_sort_workspace_size(Mcap))
        return DAUC_EINVAL;
    const SortWorkspace ws = sort_workspace(workspace, Mcap);
    const SortWs& w = ws.sort;
    const CountWs& nw = ws.count;
    unsigned* table = w.keys_a;  // Mcap + 64 words: room for the +inf tail
    // the histogram aggregates 8 keys per thread in LDS; the count and scatter passes are chains of
    // dependent loads per key, so they take one key per thread per step (every chain in flight)
    unsigned* grp = ws.grp;  // [kDirectMaxGroups]
    const auto blocks = [](int64_t keys, int64_t per, int64_t cap) {
        const int64_t b = (keys + per - 1) / per;
        return dim3(static_cast<unsigned>(b < cap ? b : cap));
    };
    if (ready_hist == nullptr)
        hipLaunchKernelGGL(direct_hist_kernel, blocks(Mcap, 256 * kDirectPerThread, 256), dim3(256), 0, st, pos, Mp,
                           nw.first, nw.cstart, kCiCntWords);
    hipLaunchKernelGGL(direct_count_kernel<false>, blocks(Mcap, kDirectThreads, kDirectGrid), dim3(kDirectThreads), 0,
                       st, pos, Mcap, ready_hist ? ready_hist : nw.first, nw.l1, nw.meta, nw.cstart, w.keys_b,
                       nullptr, 0u);
    hipLaunchKernelGGL(direct_blocks_kernel, dim3(kDirectMaxGroups), dim3(kDirectGroup), 0, st, nw.cstart, nw.meta,
                       nw.blk, grp);
#ifdef DAUC_TUNING
    if (g_direct_fault != 0)
        hipLaunchKernelGGL(direct_fault_kernel, dim3(1), dim3(64), 0, st, g_direct_fault, Mp, nw.meta, nw.cstart,
                           w.keys_b);
#endif
    hipLaunchKernelGGL(direct_scatter_kernel, blocks(Mcap, kDirectThreads, kDirectGrid), dim3(kDirectThreads), 0, st, pos,
                       Mp, nw.blk, grp, nw.meta, nw.cstart, w.keys_b, table, kCiCntWords);
    *ix = DirectIndex{table, nw.l1, nw.blk, grp, nw.meta};
    return launch_status();
}

int counts_labeled_direct_slots(const SlotSource& src, float* pos, int64_t Mcap, const LabeledQueries& q,
                                unsigned* verdict, void* workspace, size_t workspace_bytes, hipStream_t st,
                                unsigned* check) {
    if (!q.valid() || pos == nullptr || src.slots == nullptr || src.parts < 1 || src.parts > kMaxSlotParts ||
        workspace == nullptr || Mcap < 1 || workspace_bytes < dauc_sort_workspace_size(Mcap))
        return DAUC_EINVAL;
    const SortWorkspace ws = sort_workspace(workspace, Mcap);
    const SortWs& w = ws.sort;
    const CountWs& nw = ws.count;
    unsigned* table = w.keys_a;
    unsigned* grp = ws.grp;
    const int64_t gk = (Mcap + kSlotCountThreads - 1) / kSlotCountThreads;
    hipLaunchKernelGGL(direct_count_slots_kernel<false>, dim3(static_cast<unsigned>(gk)), dim3(kSlotCountThreads), 0,
                       st, src, Mcap, nw.l1, nw.meta, nw.cstart, w.keys_b, pos, nullptr, 0u);
    hipLaunchKernelGGL(direct_blocks_kernel, dim3(kDirectMaxGroups), dim3(kDirectGroup), 0, st, nw.cstart, nw.meta,
                       nw.blk, grp);
    const int64_t gs = (Mcap + kDirectThreads - 1) / kDirectThreads;
    hipLaunchKernelGGL(direct_scatter_kernel, dim3(static_cast<unsigned>(gs < kDirectGrid ? gs : kDirectGrid)),
                       dim3(kDirectThreads), 0, st, pos, src.m_eff, nw.blk, grp, nw.meta, nw.cstart, w.keys_b, table,
                       kCiCntWords);
    int rc = launch_status();
    if (rc || q.empty()) return rc;
    return launch_ci(q, nw, table, 0, st, CiForm::direct(verdict, grp, src.m_eff, check));
}

int64_t slotted_cells(int64_t Mcap) {
    // the plan uses at most min(kCiMaxCells, 2 M + one per used bucket) cells
    const int64_t c = 2 * Mcap + kCiTop;
    return c < kCiMaxCells ? c : kCiMaxCells;
}

size_t slotted_table_bytes(int64_t Mcap) {  // primary + secondary + tertiary
    return size_t(slotted_cells(Mcap) + 1) * 8 * 4 + size_t(slotted_cells(Mcap)) * 8 * 4;
}

size_t slotted_fill_bytes(int64_t Mcap) { return size_t(slotted_cells(Mcap) + 1) * 8 * 4; }  // the +inf part

int64_t slotted_cnt_words() { return (int64_t(kCiMaxBlocks) * kCiBlock) / 4; }

unsigned* slotted_meta_ptr(void* workspace, int64_t Mcap) { return sort_workspace(workspace, Mcap).count.meta; }

int counts_labeled_slotted(const SlotSource& src, unsigned* stab, int64_t Mcap, const LabeledQueries& q,
                           unsigned* verdict, void* workspace, size_t workspace_bytes, hipStream_t st,
                           unsigned* check) {
    if (!q.valid() || stab == nullptr || src.slots == nullptr || src.parts < 1 || src.parts > kMaxSlotParts ||
        workspace == nullptr || Mcap < 1 || workspace_bytes < dauc_sort_workspace_size(Mcap) || check == nullptr)
        return DAUC_EINVAL;
    const CountWs nw = sort_workspace(workspace, Mcap).count;
    const int64_t gk = (Mcap + kSlotCountThreads - 1) / kSlotCountThreads;
    const unsigned cells = static_cast<unsigned>(slotted_cells(Mcap));
    hipLaunchKernelGGL(direct_count_slots_kernel<true>, dim3(static_cast<unsigned>(gk)), dim3(kSlotCountThreads), 0,
                       st, src, Mcap, nw.l1, nw.meta, nw.cstart, nw.first, nullptr, stab, cells);  // (SLOT: see above)
    int rc = launch_status();
    if (rc || q.empty()) return rc;
    return launch_ci(q, nw, stab, 0, st,
                     CiForm::slotted_two_step(verdict, src.m_eff, check, reinterpret_cast<const uint2*>(nw.cstart),
                                              cells, reinterpret_cast<unsigned long long*>(nw.first)));
}

int counts_labeled_direct_slotted(const float* pos, const unsigned long long* Mp, int64_t Mcap, unsigned* stab,
                                  const LabeledQueries& q, unsigned* verdict, void* workspace, size_t workspace_bytes,
                                  hipStream_t st, const unsigned* ready_hist) {
    if (!q.valid() || pos == nullptr || Mp == nullptr || stab == nullptr || ready_hist == nullptr || Mcap < 1 ||
        workspace == nullptr || workspace_bytes < dauc_sort_workspace_size(Mcap))
        return DAUC_EINVAL;
    const CountWs nw = sort_workspace(workspace, Mcap).count;
    const unsigned cells = static_cast<unsigned>(slotted_cells(Mcap));
    const int64_t gb = (Mcap + kDirectThreads - 1) / kDirectThreads;
    hipLaunchKernelGGL(direct_count_kernel<true>, dim3(static_cast<unsigned>(gb < kDirectGrid ? gb : kDirectGrid)),
                       dim3(kDirectThreads), 0, st, pos, Mcap, ready_hist, nw.l1, nw.meta, nw.cstart, nullptr, stab,
                       cells, Mp);
    int rc = launch_status();
    if (rc || q.empty()) return rc;
    return launch_ci(q, nw, stab, 0, st,
                     CiForm::slotted_one_call(verdict, Mp, reinterpret_cast<const uint2*>(nw.cstart), cells));
}

int counts_labeled_direct(const float* pos, const unsigned long long* Mp, int64_t Mcap, const LabeledQueries& q,
                          unsigned* verdict, void* workspace, size_t workspace_bytes, hipStream_t st,
                          const unsigned* ready_hist, unsigned* check) {
    if (!q.valid()) return DAUC_EINVAL;
    DirectIndex ix{};
    int rc = build_direct_index(pos, Mp, Mcap, workspace, workspace_bytes, st, &ix, ready_hist);
    if (rc || q.empty()) return rc;
    return launch_ci(q, sort_workspace(workspace, Mcap).count, ix.table, 0, st,
                     CiForm::direct(verdict, ix.grp, Mp, check));
}

}  // namespace dauc

#ifdef DAUC_TUNING
extern "C" int dauc_set_direct_fault(int mode) {
    if (mode < 0 || mode > 3) return DAUC_EINVAL;
    dauc::g_direct_fault = mode;
    return DAUC_OK;
}
#endif
