// Wavefront, lane-group and workgroup reductions shared by the kernels (gfx950: 64 lanes per wavefront).
// Every device function is force-inlined and every lane receives the result.  Not here: gda_ce.hip's and gda_mmd.hip's
// block_sum (another tree, a result valid on thread 0 only: moving them would change the summation order).
#pragma once
#include <hip/hip_runtime.h>

// xor butterfly over the 64 lanes of a wavefront
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// the same over aligned groups of G lanes (G a power of two, at most 64)
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, G);
    return v;
}

template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, G));
    return v;
}

// sum over the workgroup (blockDim.x a power of two) through red[blockDim.x] in LDS; red is free again on return
__device__ __forceinline__ float block_sum_f(float v, float* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double block_sum_d(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// thread t's share part[t], part[t + THREADS], ... of part[0 .. n), summed in double on top of a (THREADS = blockDim.x)
template <int THREADS>
__device__ __forceinline__ double stride_sum_d(const float* __restrict__ part, int n, double a = 0.0) {
    for (int k = threadIdx.x; k < n; k += THREADS) a += (double)part[k];
    return a;
}

// block-strided sum of part[0 .. n) in double, folded through red[THREADS]; every thread receives it
template <int THREADS>
__device__ __forceinline__ double fold_d(const float* __restrict__ part, int n, double* red) {
    return block_sum_d(stride_sum_d<THREADS>(part, n), red);
}

namespace {

// one workgroup of THREADS: out[0] = scale * sum(part[0 .. nparts)), the sum as fold_d forms it
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_fold_scalar(const float* __restrict__ part, int nparts, double scale,
                                                         float* __restrict__ out) {
    __shared__ double red[THREADS];
    const double tot = fold_d<THREADS>(part, nparts, red);
    if (threadIdx.x == 0) out[0] = (float)(scale * tot);
}

}  // namespace

// lane src_lane's value in every lane (v_readlane: src_lane is wave-uniform)
__device__ __forceinline__ float bcast(float v, int src_lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}
