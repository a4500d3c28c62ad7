// Internal helpers shared by the libdauc.so translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dauc.h"

namespace dauc {

constexpr int kWave = 64;  // CDNA wavefront width

// native 16-byte vector (one dwordx4 per lane); usable with the nontemporal builtins
typedef float f32x4 __attribute__((ext_vector_type(4)));

inline hipStream_t as_hip(dauc_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Launch-status helper: a failed launch is reported as -(hipError_t).
inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? DAUC_OK : -static_cast<int>(e);
}

// ---- wavefront / block reductions (64-lane waves) ----------------------------

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// Sum K doubles across the block. Every thread gets the block totals in v[].
// `scratch` must hold K * (blockDim.x / 64) doubles. The order of additions is
// fixed by the thread layout, so the result is bitwise reproducible.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* scratch) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = threadIdx.x / kWave;
    const int nw = blockDim.x / kWave;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) scratch[k * nw + wid] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int w = 0; w < nw; ++w) s += scratch[k * nw + w];
        v[k] = s;
    }
    __syncthreads();
}

// ---- inter-workgroup "last arriver" ticket ------------------------------------
// The write-through form of the agent-scope hand-off (cdna_hip_programming §6
// Guideline 16, R1): the payload (one workgroup's fp64 partial row) is stored by
// thread 0 with sc1 (write-through, agent-scope atomic) stores, drained with
// s_waitcnt vmcnt(0), and signalled by a relaxed agent-scope ticket add. The last
// arriver reads every row with sc1 loads (load_sc1), so neither a release fence
// (an L2 write-back that every workgroup would pay behind its streamed stores) nor
// an acquire is needed. Tickets start at zero and the last arriver resets them.
typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned gu32;

__device__ __forceinline__ void store_sc1(double* p, double v) {
    __hip_atomic_store((gu64*)p, static_cast<unsigned long long>(__double_as_longlong(v)), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double load_sc1(const double* p) {
    return __longlong_as_double(static_cast<long long>(
        __hip_atomic_load((gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
}

// Called by every thread of the block after thread 0 stored its row with store_sc1.
// Returns true in every thread of the block that arrived last.
__device__ __forceinline__ bool arrive_last(unsigned* counter, unsigned nblocks, int* lds_flag) {
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add((gu32*)counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (t == nblocks - 1);
        // leave the workspace zeroed for the next call on this stream
        if (last) __hip_atomic_store((gu32*)counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *lds_flag = last;
    }
    __syncthreads();
    // no instruction: keeps the compiler from hoisting the sc1 row loads above the ticket
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return *lds_flag != 0;
}

// ---- label arrays ---------------------------------------------------------------------------
// The element types a label array may have (dauc.h, DAUC_LABEL_*). with_labels calls f with the
// typed pointer and returns its status, or DAUC_EINVAL for any other dtype.
inline bool label_dtype_ok(int label_dtype) {
    return label_dtype == DAUC_LABEL_I8 || label_dtype == DAUC_LABEL_I32 || label_dtype == DAUC_LABEL_I64;
}

template <typename F>
int with_labels(const void* labels, int label_dtype, F&& f) {
    switch (label_dtype) {
        case DAUC_LABEL_I8: return f(static_cast<const int8_t*>(labels));
        case DAUC_LABEL_I32: return f(static_cast<const int32_t*>(labels));
        case DAUC_LABEL_I64: return f(static_cast<const int64_t*>(labels));
        default: return DAUC_EINVAL;
    }
}

}  // namespace dauc
