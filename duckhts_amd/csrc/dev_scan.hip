// dev_scan.hip -- the scans the count functions and the record stage share: one inclusive scan over the threads of a workgroup, and one
// exclusive scan of an array in place in two levels (the carry).  DESIGN.md 4q says who instantiates what.
//
//   operator     Op::identity<T>() and Op::combine(a, b): ScanSum (uint32_t, uint64, and any T with operator+, such as bam_bedcov's CovVec)
//                ScanMin (uint64) and ScanMax (any T with operator< and a static T::lowest(), such as the interval index's (rank, end) pair,
//                whose maximum in lexicographic order is the running maximum end per chrom).  All are commutative; the carry relies on it
//                where it reduces a chunk.
//   block_scan   the inclusive scan over the NT threads of the workgroup, Hillis-Steele through LDS: log2 NT rounds of read / barrier /
//                combine / barrier.  It ends in a barrier and leaves sh[t] = the inclusive value of thread t, so a caller may read its
//                neighbour's value or the workgroup's total (sh[NT - 1]) behind it, and needs a barrier of its own before sh is written again.
//   carry        v[i] becomes the combination of the elements in front of i (REV: behind i), seeded.  Chunks of 256 x PER elements:
//                carry_reduce leaves every chunk's combination in part, carry_scan (one workgroup, a chunk of part a turn) turns part into
//                what lies in front of every chunk, carry_apply scans every chunk again behind its part.  REV visits element i of a chunk
//                as last - i, so the suffix scan runs through the same bodies.  The exclusive value of a thread is its neighbour's
//                inclusive one (sh[t - 1], the identity for thread 0), never incl - own: min has no inverse.  The forward form leaves the
//                total in part[np] and v[n] (the buffer has n + 1 elements); the reverse form writes no total.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ScanSum {
    template <typename T> static __device__ __forceinline__ T identity() { return T{}; }
    template <typename T> static __device__ __forceinline__ T combine(const T &a, const T &b) { return a + b; }
};
struct ScanMin {
    template <typename T> static __device__ __forceinline__ T identity() { return ~(T)0; }
    template <typename T> static __device__ __forceinline__ T combine(const T &a, const T &b) { return a < b ? a : b; }
};

struct ScanMax {
    template <typename T> static __device__ __forceinline__ T identity() { return T::lowest(); }
    template <typename T> static __device__ __forceinline__ T combine(const T &a, const T &b) { return a < b ? b : a; }
};

template <typename T, typename Op, uint32_t NT = 256u> __device__ __forceinline__ T block_scan(T v, T *sh) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < NT; d <<= 1) {
        const T y = t >= d ? sh[t - d] : Op::template identity<T>();
        __syncthreads();
        sh[t] = Op::combine(sh[t], y);
        __syncthreads();
    }
    const T r = sh[t];
    __syncthreads();
    return r;
}

// ---- the carry in two levels -----------------------------------------------------------------------------------------------------------------
// part[b] = the combination of chunk b of v[0 .. n) (in any order: the operators commute)
template <typename T, typename Op, uint32_t PER = 16u> __global__ void __launch_bounds__(256) carry_reduce(const T *__restrict__ v, uint64_t n, T *__restrict__ part) {
    __shared__ T sh[256];
    const uint64_t b = (uint64_t)blockIdx.x * (256u * PER) + threadIdx.x * PER;
    T m = Op::template identity<T>();
#pragma unroll
    for (uint32_t e = 0; e < PER; e++) m = Op::combine(m, b + e < n ? v[b + e] : Op::template identity<T>());
    const T incl = block_scan<T, Op>(m, sh);
    if (threadIdx.x == 255u) part[blockIdx.x] = incl;
}
// part[b] becomes seed combined with part[0 .. b) (REV: with part(b .. np)): one workgroup, 256 x PER elements a turn.  Forward: part[np] = the total
template <typename T, typename Op, bool REV, uint32_t PER = 16u> __global__ void __launch_bounds__(256) carry_scan(T *__restrict__ part, uint64_t np, T seed) {
    __shared__ T sh[256];
    T carry = seed;
    for (uint64_t r0 = 0; r0 < np; r0 += 256u * PER) {
        const uint64_t r = r0 + threadIdx.x * PER;                                                 // in scan order; REV: element np - 1 - r
        T own[PER], m = Op::template identity<T>();
#pragma unroll
        for (uint32_t e = 0; e < PER; e++) { own[e] = r + e < np ? part[REV ? np - 1u - (r + e) : r + e] : Op::template identity<T>(); m = Op::combine(m, own[e]); }
        block_scan<T, Op>(m, sh);
        T run = Op::combine(carry, threadIdx.x ? sh[threadIdx.x - 1u] : Op::template identity<T>());
        carry = Op::combine(carry, sh[255]);
        __syncthreads();
#pragma unroll
        for (uint32_t e = 0; e < PER; e++) if (r + e < np) { part[REV ? np - 1u - (r + e) : r + e] = run; run = Op::combine(run, own[e]); }
    }
    if (!REV && threadIdx.x == 0) part[np] = carry;
}
// v[i] becomes part[chunk of i] combined with the chunk's elements in front of i (REV: behind i).  Forward: v[n] = the total
template <typename T, typename Op, bool REV, uint32_t PER = 16u> __global__ void __launch_bounds__(256) carry_apply(T *__restrict__ v, uint64_t n, const T *__restrict__ part, uint64_t np) {
    __shared__ T sh[256];
    const uint64_t first = (uint64_t)blockIdx.x * (256u * PER), last = first + (256u * PER - 1u), r = threadIdx.x * PER;      // in scan order; REV: element last - r
    T own[PER], m = Op::template identity<T>();
#pragma unroll
    for (uint32_t e = 0; e < PER; e++) { const uint64_t i = REV ? last - (r + e) : first + (r + e); own[e] = i < n ? v[i] : Op::template identity<T>(); m = Op::combine(m, own[e]); }
    block_scan<T, Op>(m, sh);
    T run = Op::combine(part[blockIdx.x], threadIdx.x ? sh[threadIdx.x - 1u] : Op::template identity<T>());
#pragma unroll
    for (uint32_t e = 0; e < PER; e++) { const uint64_t i = REV ? last - (r + e) : first + (r + e); if (i < n) { v[i] = run; run = Op::combine(run, own[e]); } }
    if (!REV && blockIdx.x == 0 && threadIdx.x == 0) v[n] = part[np];
}
