// What the two gradient steps and their validation passes (csrc/valuenet_fit.hip, csrc/distnet_fit.hip) share: the register
// layout of v_mfma_f32_32x32x2_f32, a quad of K steps on NT tiles, the chunked accumulation, the wave / block sums of the second
// stages and the moments of the per-sample losses.  Device inline functions only: each file keeps its own kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tmcts_fit {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the row of D that register r of the lane half `half` holds (the column is lane & 31)
__device__ __forceinline__ int drow(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// one quad of K: four steps on each of the NT tiles
template <int NT>
__device__ __forceinline__ void vf_quad(f32x16 (&acc)[NT], const float4& a, const float4 (&b)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[t].x, acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[t].y, acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[t].z, acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[t].w, acc[t], 0, 0, 0);
}

constexpr int CHUNK_QUADS = 4;          // quads of K per chunk: 32 terms per sequential chain
template <int NT>
__device__ __forceinline__ void vf_zero(f32x16 (&acc)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
}
template <int NT>
__device__ __forceinline__ void vf_add(f32x16 (&tot)[NT], const f32x16 (&acc)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[t][r] += acc[t][r];
}

__device__ __forceinline__ size_t row_of(const int64_t* __restrict__ idx, int b) { return idx ? (size_t)idx[b] : (size_t)b; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// sum over a workgroup of 256 threads, in one fixed order (sm: 256 doubles of LDS)
__device__ __forceinline__ double block_sum(double v, double* sm) {
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) sm[threadIdx.x] += sm[threadIdx.x + d];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

// mean of the n per-sample losses per[0..n) and the sum of their squared deviations from it, by a workgroup of 256 threads in
// one fixed order (thread t takes the samples t, t + 256, ...).  The loss of a gradient step (k_vf_loss, k_df_loss) and a
// chunk of a validation pass (chunk_moments) are both this function: the same losses give the same bits.
__device__ __forceinline__ void block_moments(const double* __restrict__ per, int n, double* sm, double& mean, double& ssq) {
    double s = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) s += per[b];
    mean = block_sum(s, sm) / (double)n;
    double q = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) {
        const double d = per[b] - mean;
        q += d * d;
    }
    ssq = block_sum(q, sm);
}

// One chunk of a validation pass (workgroup blockIdx.x of 256 threads): rows[3 c] = {w, mean, std} of the per-sample losses
// of the slab's rows [c chunk, min(B, (c + 1) chunk)), in double.  w: the sum of the rows' weights (block_moments' order) when
// `weighted`, else their count.  std divides by count - DDOF (the value net: 0; the head: 1, NaN for one row as torch.std_mean).
template <int DDOF>
__device__ __forceinline__ void chunk_moments(const double* __restrict__ per, const float* __restrict__ weight, int B, int chunk,
                                              int weighted, double* __restrict__ rows, double* sm) {
    const int b0 = blockIdx.x * chunk, cnt = min(chunk, B - b0);
    if (cnt < 1) return;
    double mean, ssq, w = (double)cnt;
    block_moments(per + b0, cnt, sm, mean, ssq);
    if (weighted) {
        double s = 0.0;
        for (int b = threadIdx.x; b < cnt; b += 256) s += (double)weight[b0 + b];
        w = block_sum(s, sm);
    }
    if (threadIdx.x == 0) {
        double* dst = rows + 3 * (size_t)blockIdx.x;
        dst[0] = w;
        dst[1] = mean;
        dst[2] = sqrt(ssq / (double)(cnt - DDOF));
    }
}

}  // namespace tmcts_fit
