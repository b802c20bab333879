// The fixed-order sums of the two conjugate-gradient stages (position
// averaging and the rotation refit): over a workgroup, over the partials of a
// whole grid, over the lanes that share a node.  No float atomic: the same
// bits on every run.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace sfm {

// v[0..NV) summed over the workgroup, the same value in every thread: the wave's
// shuffle tree, a word per wave and value, the words added in wave order.
// Every thread of the workgroup calls it; `words` holds NV * (threads / 64) doubles.
template <int NV> __device__ __forceinline__ void pa_block_sum(double (&v)[NV], double *words) {
    const int tid = threadIdx.x, nw = blockDim.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_xor(v[i], off, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) words[NV * (tid >> 6) + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double t = words[i];
        for (int w = 1; w < nw; ++w) t += words[NV * w + i];
        v[i] = t;
    }
    __syncthreads();  // the words may be written again
}

// part[0..n) added in a fixed order by the whole workgroup: thread t takes t, t + T, ..
template <int NV> __device__ __forceinline__ void pa_resum(double (&v)[NV], const double *const (&part)[NV], int n,
                                                           double *words) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double t = 0.0;
        for (int k = threadIdx.x; k < n; k += blockDim.x) t += part[i][k];
        v[i] = t;
    }
    pa_block_sum<NV>(v, words);
}

template <int NV> __device__ __forceinline__ void pa_group_sum(double (&v)[NV], int G) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
        for (int off = G >> 1; off > 0; off >>= 1) v[i] += __shfl_xor(v[i], off, 64);
}

}  // namespace sfm
