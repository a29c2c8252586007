// What the two gradient steps and their validation passes (csrc/valuenet_fit.hip, csrc/distnet_fit.hip) share.  Device inline
// functions: the register layout of v_mfma_f32_32x32x2_f32, a quad of K steps on NT tiles, the chunked accumulation, the wave /
// block sums of the second stages and the moments of the per-sample losses.  Kernels that are the same statements in both nets
// up to constants and the activation: fc1's forward and data gradient (k_fit_fc1_fwd, k_fit_fc1_bwd_data), the second stage of
// every batch sum (k_fit_reduce), the loss of a gradient step and the chunks of a validation pass (k_fit_loss,
// k_fit_val_moments).  The two sources of a training row's cells, int8 or a packed observation (DenseStates, PackedStates).  The
// host helpers of the launch shapes (up4, blocks_for_waves, tiles).  A template is instantiated in the
// object of each file that launches it.  The convolutions, the output layers and the two FC weight gradients stay in their files.
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

// ---- where a CIN == 1 kernel reads its input cells: the state of training row i as int8 [200] (DenseStates) or as the packed
// observation of ENGINE_SPEC section 7, twelve dwords (PackedStates).  row(): what a lane keeps per sample.  strip(row, r): what
// it keeps for the board rows r, r + 1, r + 2 (r may be negative or past the board: rows outside 0..19 are never asked for).
// cell(strip, r, c): the value of cell (r, c) as the float the matrix core is fed, 0 empty, 1 locked, -1 the falling piece.
// Both sources give the same float for the same board, so everything a kernel does with it is the same bits. ----
struct DenseStates {
    typedef int8_t elem;
    static constexpr int STRIDE = 200;      // elements per training row
    struct Row { const int8_t* p; };
    typedef Row Strip;
    static __device__ __forceinline__ Row row(const elem* __restrict__ s, size_t i) { return Row{s + i * STRIDE}; }
    static __device__ __forceinline__ Strip strip(const Row& w, int) { return w; }
    static __device__ __forceinline__ float cell(const Strip& s, int r, int c) { return (float)s.p[r * 10 + c]; }
};

// engine.h obs_cell's semantics: the locked bit of cell (r, c) is bit 16 (r & 1) + c of word r >> 1; the cell is -1 where one
// of the four cell codes of word 10 equals 10 r + c and the low byte of word 11 (ended) is 0; the piece wins over a locked bit.
// Nothing read out of an observation is used as an address or a shift: a code is only compared (codes >= 200 match no cell, an
// ended row's codes are replaced by 255), and a row's bits 10..15 are never looked at, so any 48 bytes are safe to read.
// A row keeps words 10 and 11, loaded once per (lane, sample); a strip the two words of the four rows from the even row at or
// below r, loaded once where it is built (the word index is clamped to the ten board words).
struct PackedStates {
    typedef uint32_t elem;
    static constexpr int STRIDE = 12;
    struct Row { const uint32_t* o; uint32_t codes; };
    struct Strip { uint64_t bits; uint32_t codes; int r0; };
    static __device__ __forceinline__ Row row(const elem* __restrict__ s, size_t i) {
        const uint32_t* o = s + i * STRIDE;
        return Row{o, (o[11] & 0xFFu) ? 0xFFFFFFFFu : o[10]};
    }
    static __device__ __forceinline__ Strip strip(const Row& w, int r) {
        const int a = r >> 1;       // (arithmetic: -1 for the two rows above the board)
        const uint32_t lo = (a >= 0 && a <= 9) ? w.o[a] : 0u, hi = (a >= -1 && a <= 8) ? w.o[a + 1] : 0u;
        return Strip{(uint64_t)lo | ((uint64_t)hi << 32), w.codes, 2 * a};
    }
    static __device__ __forceinline__ float cell(const Strip& s, int r, int c) {
        const uint32_t i = (uint32_t)(r * 10 + c), k = s.codes;
        const bool piece = ((k & 0xFFu) == i) | (((k >> 8) & 0xFFu) == i) | (((k >> 16) & 0xFFu) == i) | ((k >> 24) == i);
        const uint32_t locked = (uint32_t)(s.bits >> (16 * (r - s.r0) + c)) & 1u;
        return piece ? -1.0f : (float)locked;
    }
};

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
// one fixed order (thread t takes the samples t, t + 256, ...).  The loss of a gradient step (k_fit_loss) and a
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

// ---- the activations: fwd(v) of a pre-activation, bwd(a, g) the gradient g passed where the STORED activation a is > 0 ----
struct Relu {
    static __device__ __forceinline__ float fwd(float v) { return v > 0.0f ? v : 0.0f; }
    static __device__ __forceinline__ float bwd(float a, float g) { return a > 0.0f ? g : 0.0f; }
};
struct Leaky {      // LeakyReLU(0.01); torch's rule at 0
    static __device__ __forceinline__ float fwd(float v) { return v > 0.0f ? v : 0.01f * v; }
    static __device__ __forceinline__ float bwd(float a, float g) { return a > 0.0f ? g : 0.01f * g; }
};

// ---- fc1 forward: h[b][j] = Act(bias[j] + sum_k Wf[j][k] in[b][k]); M = UNITS, N = B, K = the length of a row of in ----
template <int UNITS, int K, typename Act, int NT>
__global__ __launch_bounds__(256) void k_fit_fc1_fwd(const float* __restrict__ Wf, const float* __restrict__ bias,
                                                     const float* __restrict__ in, int B, float* __restrict__ h) {
    constexpr int MT = UNITS / 32;
    static_assert((MT & (MT - 1)) == 0 && K % (8 * CHUNK_QUADS) == 0, "whole tiles of units, whole chunks of K");
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), mt = wave & (MT - 1), n0 = (wave >> __builtin_ctz(MT)) * NT * 32;
    if (n0 >= B) return;
    bool ok[NT];
    const float* brow[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = n0 + 32 * t + l31;
        ok[t] = n < B;
        brow[t] = in + (size_t)(ok[t] ? n : 0) * K + 4 * half;
    }
    const float* arow = Wf + (size_t)(32 * mt + l31) * K + 4 * half;
    // the running total as an unevaluated sum hi + lo: TwoSum keeps what the addition of a chunk rounds away
    f32x16 hi[NT], lo[NT], acc[NT];
    vf_zero<NT>(lo);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) hi[t][r] = bias[32 * mt + drow(r, half)];
#pragma unroll 1
    for (int qc = 0; qc < K / 8; qc += CHUNK_QUADS) {
        vf_zero<NT>(acc);
#pragma unroll
        for (int q = qc; q < qc + CHUNK_QUADS; ++q) {
            // (four dwords, not one float4: the value net's entry points do not ask for 16-byte aligned parameters)
            const float4 a = make_float4(arow[8 * q], arow[8 * q + 1], arow[8 * q + 2], arow[8 * q + 3]);
            float4 b4[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                b4[t] = *reinterpret_cast<const float4*>(brow[t] + 8 * q);
                if (!ok[t]) b4[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            vf_quad<NT>(acc, a, b4);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float x = hi[t][r], y = acc[t][r], sum = x + y, yy = sum - x;
                lo[t][r] += (x - (sum - yy)) + (y - yy);
                hi[t][r] = sum;
            }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (ok[t]) {
            float* dst = h + (size_t)(n0 + 32 * t + l31) * UNITS + 32 * mt;
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[drow(r, half)] = Act::fwd(hi[t][r] + lo[t][r]);
        }
}

// ---- fc1 data gradient: din[b][k] = Act::bwd(in[b][k], sum_j dh[b][j] Wf[j][k]); M = B, N = K (a row of in), K = UNITS ----
template <int UNITS, int K, typename Act, int NT>
__global__ __launch_bounds__(256) void k_fit_fc1_bwd_data(const float* __restrict__ Wf, const float* __restrict__ dh,
                                                          const float* __restrict__ in, int B, float* __restrict__ din) {
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    constexpr int NG = K / 32 / NT;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), ng = wave % NG, m0 = (wave / NG) * 32;
    if (m0 >= B) return;
    const bool mok = m0 + l31 < B;
    const float* arow = dh + (size_t)(mok ? m0 + l31 : 0) * UNITS + 4 * half;
    const float* bcol = Wf + (size_t)(4 * half) * K + ng * NT * 32 + l31;
    f32x16 tot[NT], acc[NT];
    vf_zero<NT>(tot);
#pragma unroll 1
    for (int qc = 0; qc < UNITS / 8; qc += CHUNK_QUADS) {
        vf_zero<NT>(acc);
#pragma unroll
        for (int q = qc; q < qc + CHUNK_QUADS; ++q) {
            float4 a = *reinterpret_cast<const float4*>(arow + 8 * q);
            if (!mok) a = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 b4[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float* c = bcol + (size_t)(8 * q) * K + 32 * t;
                b4[t] = make_float4(c[0], c[K], c[2 * K], c[3 * K]);
            }
            vf_quad<NT>(acc, a, b4);
        }
        vf_add<NT>(tot, acc);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int b = m0 + drow(r, half);
            if (b < B) {
                const size_t o = (size_t)b * K + (ng * NT + t) * 32 + l31;
                din[o] = Act::bwd(in[o], tot[t][r]);
            }
        }
}

// ---- second stage: out[i] = sum_s part[s * stride + i], the partials of group g = s mod G added in ascending s (in double),
// the G group sums added in ascending g ----
template <int G>
__global__ __launch_bounds__(256) void k_fit_reduce(const float* __restrict__ part, int S, long long stride, int n,
                                                    float* __restrict__ out) {
    constexpr int PER = 256 / G;
    __shared__ double sm[256];
    const int o = threadIdx.x % PER, g = threadIdx.x / PER, i = blockIdx.x * PER + o;
    double acc = 0.0;
    if (i < n)
        for (int s = g; s < S; s += G) acc += (double)part[(size_t)s * stride + i];
    sm[threadIdx.x] = acc;
    __syncthreads();
    if (g == 0 && i < n) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < G; ++k) t += sm[k * PER + o];
        out[i] = (float)t;
    }
}

// mean and standard deviation (the divisor B - DDOF: 0 the population's; 1 torch.std_mean's default, NaN for one sample as
// torch) of the per-sample losses of a gradient step (one workgroup, double, fixed order)
template <int DDOF>
__global__ __launch_bounds__(256) void k_fit_loss(const double* __restrict__ per, int B, float* __restrict__ loss) {
    __shared__ double sm[256];
    double mean, ssq;
    block_moments(per, B, sm, mean, ssq);
    const double var = ssq / (double)(B - DDOF);
    if (threadIdx.x == 0) {
        loss[0] = (float)mean;
        loss[1] = (float)sqrt(var);
    }
}

// a validation pass's chunks of one slab: {w, mean, std} per chunk (one workgroup each; chunk_moments)
template <int DDOF>
__global__ __launch_bounds__(256) void k_fit_val_moments(const double* __restrict__ per, const float* __restrict__ weight, int B,
                                                         int chunk, int weighted, double* __restrict__ rows) {
    __shared__ double sm[256];
    chunk_moments<DDOF>(per, weight, B, chunk, weighted, rows, sm);
}

// ---- host: the sizes of the workspaces and of the launches ----
__host__ __device__ constexpr long long up4(long long x) { return (x + 3) / 4 * 4; }
static inline int blocks_for_waves(long long waves) { return (int)((waves + 3) / 4); }
static inline long long tiles(long long n) { return (n + 31) / 32; }

}  // namespace tmcts_fit
