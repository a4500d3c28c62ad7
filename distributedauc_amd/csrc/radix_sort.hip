// LSD radix sort of fp32 scores' order-preserving keys (count_index.h, key_of): the sorted path's
// table (auc_sort.hip, prepare_table, through radix_sort_keys) and dauc_sort_keys.
//
// Sort (per 8-bit digit, 4 passes, keys only; 2048-key tiles, one 256-thread workgroup each):
//   hist    : LDS histogram of the tile's digit -> hist[digit][tile] (digit-major)
//   scan    : small sorts (<= 256 tiles) have none — every scatter workgroup derives its own
//             offsets from the raw histogram; larger sorts scan it in 3 launches
//   scatter : wave w owns the tile's keys [512w, 512w + 512); a key's stable rank among its
//             wave's keys with the same digit = the wave's running count of that digit (a
//             wave-private LDS row) + the same-digit lanes below it (8 ballots); one barrier turns
//             the per-wave counts into offsets; writes to out[offset[digit][tile] + rank].

#include "sort_workspace.h"

namespace dauc {
namespace {

// ---- pass kernels -------------------------------------------------------------------

// FROM_FLOAT: the first pass reads fp32 scores and converts them to keys on the fly.
template <bool FROM_FLOAT>
__global__ __launch_bounds__(kSortThreads) void radix_hist_kernel(const void* __restrict__ in, int64_t n,
                                                                  int shift, unsigned* __restrict__ hist,
                                                                  int64_t ntiles) {
    __shared__ unsigned h[kRadix];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t0 = int64_t(blockIdx.x) * kTile;
    for (int k = 0; k < kPerThread; ++k) {
        const int64_t i = t0 + int64_t(k) * kSortThreads + threadIdx.x;
        if (i < n) {
            const unsigned key = FROM_FLOAT ? key_of(static_cast<const float*>(in)[i])
                                            : static_cast<const unsigned*>(in)[i];
            atomicAdd(&h[(key >> shift) & 0xffu], 1u);
        }
    }
    __syncthreads();
    hist[int64_t(threadIdx.x) * ntiles + blockIdx.x] = h[threadIdx.x];  // digit-major
}

// exclusive scan of m counts, in place: 3 steps (block sums, scan of block sums, add back)
__global__ __launch_bounds__(kScanBlock) void scan_blocks_kernel(unsigned* __restrict__ a, int64_t m,
                                                                 unsigned* __restrict__ block_sums) {
    __shared__ unsigned s[kScanBlock];
    const int64_t i = int64_t(blockIdx.x) * kScanBlock + threadIdx.x;
    const unsigned v = i < m ? a[i] : 0u;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < kScanBlock; d <<= 1) {
        const unsigned t = threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    if (i < m) a[i] = s[threadIdx.x] - v;  // exclusive within the block
    if (threadIdx.x == kScanBlock - 1) block_sums[blockIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(kScanBlock) void scan_sums_kernel(unsigned* __restrict__ sums, int64_t nb) {
    // one block: exclusive scan of nb block sums (nb <= kScanBlock * per-thread run)
    __shared__ unsigned s[kScanBlock];
    const int64_t per = scan_sums_run(nb);
    const int64_t b0 = int64_t(threadIdx.x) * per;
    const int64_t b1 = (b0 + per < nb) ? b0 + per : nb;
    unsigned local = 0;
    for (int64_t b = b0; b < b1; ++b) local += sums[b];
    s[threadIdx.x] = local;
    __syncthreads();
    for (int d = 1; d < kScanBlock; d <<= 1) {
        const unsigned t = threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    unsigned run = s[threadIdx.x] - local;
    for (int64_t b = b0; b < b1; ++b) {
        const unsigned v = sums[b];
        sums[b] = run;
        run += v;
    }
}

__global__ __launch_bounds__(kScanBlock) void scan_add_kernel(unsigned* __restrict__ a, int64_t m,
                                                              const unsigned* __restrict__ sums) {
    const int64_t i = int64_t(blockIdx.x) * kScanBlock + threadIdx.x;
    if (i < m) a[i] += sums[blockIdx.x];
}

// FUSED_SCAN: offs is the raw digit-major histogram; every workgroup derives its own output
// offsets from it (its digit's count in the tiles before it + the exclusive scan of the digit
// totals): a small sort (<= kFusedScanTiles tiles, sort_workspace.h) then needs no scan launches at all.

// exclusive scan of v over the block's 256 threads (thread t holds digit t): wave scans by
// shuffles, then the wave totals through LDS (one barrier); returns the exclusive prefix
__device__ __forceinline__ unsigned block_excl_scan256(unsigned v, unsigned* wtot) {
    static_assert(kSortThreads == 256, "4 waves");
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    unsigned incl = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned t = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += t;
    }
    if (lane == kWave - 1) wtot[wid] = incl;
    __syncthreads();
    unsigned before = 0;
#pragma unroll
    for (int w = 0; w < kSortThreads / kWave; ++w) before += w < wid ? wtot[w] : 0u;
    return before + incl - v;
}

// Stable scatter of one tile. Wave w owns the tile's contiguous keys [w * 512, (w + 1) * 512),
// read as 8 chunks of 64 (one per lane). A key's rank among its wave's keys with the same digit
// = the wave's running count of that digit (wave-private LDS row: a wave's LDS reads and writes
// are ordered, so no barrier) + the same-digit lanes below it in its chunk (8 ballots: wave
// multisplit). One barrier, then per digit the waves' counts become offsets, and every key goes
// to base[digit] + offset[wave][digit] + rank: 2 barriers per pass instead of 4 per chunk.
template <bool FROM_FLOAT, bool FUSED_SCAN>
__global__ __launch_bounds__(kSortThreads) void radix_scatter_kernel(const void* __restrict__ in, int64_t n,
                                                                     int shift,
                                                                     const unsigned* __restrict__ offs,
                                                                     int64_t ntiles,
                                                                     unsigned* __restrict__ out) {
    constexpr int kWaves = kSortThreads / kWave;
    constexpr int kChunks = kTile / kSortThreads;  // chunks of 64 keys per wave
    __shared__ unsigned base[kRadix];             // output start of each digit for this tile
    __shared__ unsigned wcnt[kWaves][kRadix];     // per-wave running digit counts, then offsets
    __shared__ unsigned wtot[kWaves];
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    const int64_t t0 = int64_t(blockIdx.x) * kTile + int64_t(wid) * (kChunks * kWave);
    unsigned key[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int64_t i = t0 + c * kWave + lane;
        key[c] = 0u;
        if (i < n)
            key[c] = FROM_FLOAT ? key_of(static_cast<const float*>(in)[i]) : static_cast<const unsigned*>(in)[i];
    }
    // this tile's digit bases (thread t = digit t)
    if constexpr (FUSED_SCAN) {
        static_assert(kSortThreads == kRadix, "one thread per digit");
        const unsigned* h = offs + int64_t(threadIdx.x) * ntiles;
        unsigned before = 0, total = 0;
        int64_t b = 0;
        for (; b + 4 <= ntiles; b += 4) {
            const unsigned c0 = h[b], c1 = h[b + 1], c2 = h[b + 2], c3 = h[b + 3];
            before += (b < blockIdx.x ? c0 : 0u) + (b + 1 < blockIdx.x ? c1 : 0u) + (b + 2 < blockIdx.x ? c2 : 0u) +
                      (b + 3 < blockIdx.x ? c3 : 0u);
            total += c0 + c1 + c2 + c3;
        }
        for (; b < ntiles; ++b) {
            const unsigned c = h[b];
            before += b < blockIdx.x ? c : 0u;
            total += c;
        }
        base[threadIdx.x] = block_excl_scan256(total, wtot) + before;
    } else {
        base[threadIdx.x] = offs[int64_t(threadIdx.x) * ntiles + blockIdx.x];
    }
#pragma unroll
    for (int q = 0; q < kRadix / kWave; ++q) wcnt[wid][q * kWave + lane] = 0u;
    unsigned rank[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const bool valid = t0 + c * kWave + lane < n;
        const unsigned d = (key[c] >> shift) & 0xffu;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long m = __ballot((d >> bit) & 1u);
            same &= ((d >> bit) & 1u) ? m : ~m;
        }
        const unsigned below = __popcll(same & lt);
        const unsigned run = valid ? wcnt[wid][d] : 0u;  // every same-digit lane reads before the leader writes
        rank[c] = run + below;
        if (valid && below == 0) wcnt[wid][d] = run + __popcll(same);
    }
    __syncthreads();
    {
        // offsets of the waves within each digit (thread t = digit t)
        unsigned run = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const unsigned c = wcnt[w][threadIdx.x];
            wcnt[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        if (t0 + c * kWave + lane < n) {
            const unsigned d = (key[c] >> shift) & 0xffu;
            out[base[d] + wcnt[wid][d] + rank[c]] = key[c];
        }
    }
}

}  // namespace

// Sorts the keys of neg[0..N) into the workspace; returns the sorted array.
int radix_sort_keys(const float* neg, int64_t N, const SortWs& w, hipStream_t st, const unsigned** sorted) {
    const unsigned* src = nullptr;
    unsigned* dst = w.keys_a;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 8 * pass;
        if (pass == 0)
            hipLaunchKernelGGL(radix_hist_kernel<true>, dim3(w.ntiles), dim3(kSortThreads), 0, st,
                               static_cast<const void*>(neg), N, shift, w.hist, w.ntiles);
        else
            hipLaunchKernelGGL(radix_hist_kernel<false>, dim3(w.ntiles), dim3(kSortThreads), 0, st,
                               static_cast<const void*>(src), N, shift, w.hist, w.ntiles);
        const void* in = pass == 0 ? static_cast<const void*>(neg) : static_cast<const void*>(src);
        if (w.fused_scan) {
            // small sorts are launch-bound: the scatter workgroups scan the histogram themselves
            if (pass == 0)
                hipLaunchKernelGGL((radix_scatter_kernel<true, true>), dim3(w.ntiles), dim3(kSortThreads), 0, st,
                                   in, N, shift, w.hist, w.ntiles, dst);
            else
                hipLaunchKernelGGL((radix_scatter_kernel<false, true>), dim3(w.ntiles), dim3(kSortThreads), 0, st,
                                   in, N, shift, w.hist, w.ntiles, dst);
        } else {
            hipLaunchKernelGGL(scan_blocks_kernel, dim3(w.nsum), dim3(kScanBlock), 0, st, w.hist, w.m, w.sums);
            hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kScanBlock), 0, st, w.sums, w.nsum);
            hipLaunchKernelGGL(scan_add_kernel, dim3(w.nsum), dim3(kScanBlock), 0, st, w.hist, w.m, w.sums);
            if (pass == 0)
                hipLaunchKernelGGL((radix_scatter_kernel<true, false>), dim3(w.ntiles), dim3(kSortThreads), 0, st,
                                   in, N, shift, w.hist, w.ntiles, dst);
            else
                hipLaunchKernelGGL((radix_scatter_kernel<false, false>), dim3(w.ntiles), dim3(kSortThreads), 0, st,
                                   in, N, shift, w.hist, w.ntiles, dst);
        }
        const int rc = launch_status();
        if (rc) return rc;
        src = dst;
        dst = (dst == w.keys_a) ? w.keys_b : w.keys_a;
    }
    *sorted = src;
    return DAUC_OK;
}

}  // namespace dauc

using namespace dauc;

extern "C" {

int dauc_sort_keys(const float* scores, int64_t n, unsigned* keys_out, void* workspace,
                   size_t workspace_bytes, dauc_stream_t stream) {
    if (n <= 0 || scores == nullptr || keys_out == nullptr || workspace == nullptr ||
        workspace_bytes < sort_ws_bytes(n) || n > 0xffffffffLL)
        return DAUC_EINVAL;
    const SortWs w = sort_ws(workspace, n);
    const unsigned* sorted = nullptr;
    hipStream_t st = as_hip(stream);
    int rc = radix_sort_keys(scores, n, w, st, &sorted);
    if (rc) return rc;
    return -static_cast<int>(hipMemcpyAsync(keys_out, sorted, size_t(n) * 4, hipMemcpyDeviceToDevice, st));
}

}  // extern "C"
