// The split-precision ("bf16x3") convolutions of the value net (included at the end of valuenet.hip): the opt-in evaluator
// backend TM_VALUENET_BF16X3.  Same inputs and the same output as k_vn_conv (a3 rows in the TM_VALUENET_SCRATCH_MFMA layout,
// the fc1 tiles' arrival counters cleared), so today's k_vn_fc1 consumes it unchanged.
//
// Numerics contract (DESIGN.md section 3.3; tests/test_split_precision.py keeps a numpy emulation of it):
//   * every fp32 operand x of conv2 and conv3 (weights and activations) is split exactly into three bf16 planes with the
//     plain round-to-nearest-even conversion: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (both differences
//     are exact in fp32);
//   * a product a*b is the sum of the six plane products with i + j <= 2: mid*mid, lo*hi, hi*lo, mid*hi, hi*mid, hi*hi (the
//     order they are accumulated in, smallest first, per MFMA step).  Each is exact in fp32; the matrix core accumulates in
//     fp32.  The three dropped terms are below 2^-24 of the product: the error is that of an fp32 sum, not bit-equal to the
//     fp32 fma chain of k_vn_conv (and not claimed to be);
//   * the reduction over k = tap * 32 + input channel runs in MFMA steps of 16 k (v_mfma_f32_32x32x16_bf16), ascending;
//   * conv1 (its input is the rendered board, {-1, 0, 1}) stays on k_vn_conv's fp32 code, fc1 and the output layer on
//     k_vn_fc1: the same bits as the fp32 backend for the same a3;
//   * one wave computes one state from its own inputs, with the same instructions whatever the batch: a state's outputs depend
//     on that state only, not on the batch size, its position in it or its neighbours, and are the same bits from launch to
//     launch.
#include "bf16x3.h"     // split3, bf16x8, bf16x4, X3_ROW, store_planes

constexpr int X3_WAVE_BYTES = 144 * X3_ROW * 2 + 200 * 4;    // a1 planes (a2 overlays them), the input board in fp32
static_assert((144 * X3_ROW * 2) % 16 == 0, "input board aligned");
// one workgroup of four waves per CU: 123 KB of the 160 KB
constexpr int X3_PLANES = 18 * 3 * 64 * 8;                   // bf16 per convolution in the prepared planes: [step][plane][lane][8]
static_assert(2 * X3_PLANES / 2 == TM_VALUENET_PREPARED_X3, "planes buffer");

// conv2 / conv3 weights as bf16 planes in the A-operand order of v_mfma_f32_32x32x16_bf16: for step s of the 18 (16 k each,
// k = tap * 32 + ci, so tap = s / 2 and ci = 16 (s % 2) + 8 (l >> 5) + j) lane l holds W[co = l & 31][ci][tap] in element
// j of plane p at planes[((conv * 18 + s) * 3 + p) * 64 + l][j].
__global__ void k_vn_prepare_x3(const float* __restrict__ P, __bf16* __restrict__ planes) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;      // (conv, s, lane, j)
    if (t >= 2 * 18 * 64 * 8) return;
    const int conv = t / (18 * 512), s = (t / 512) % 18, l = (t / 8) % 64, j = t % 8;
    const int co = l & 31, ci = 16 * (s & 1) + 8 * (l >> 5) + j, tap = s >> 1;
    const float x = P[(conv ? OFF_C3W : OFF_C2W) + co * 288 + ci * 9 + tap];
    __bf16 h, m, lo;
    split3(x, h, m, lo);
    __bf16* dst = planes + (size_t)conv * X3_PLANES + (size_t)(s * 3) * 512 + l * 8 + j;
    dst[0] = h;
    dst[512] = m;
    dst[1024] = lo;
}

// One 3x3 valid convolution 32 -> 32 channels over TILES tiles of 32 output positions: D[co][position] += sum over the 18
// steps of the six plane products.  in: the wave's activation rows; brow[t][tap]: this lane's bf16 offset of the row its
// column reads at that tap (+ 8 (l >> 5) channels); W: the convolution's planes (+ lane).
template <int TILES>
__device__ __forceinline__ void conv_x3_mfma(const __bf16* in, const int (&brow)[TILES][9], const bf16x8* W,
                                             f32x16 (&acc)[TILES]) {
#pragma unroll
    for (int s = 0; s < 18; ++s) {
        const bf16x8 ah = W[(s * 3 + 0) * 64], am = W[(s * 3 + 1) * 64], al = W[(s * 3 + 2) * 64];
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            const __bf16* b = in + brow[t][s >> 1] + 16 * (s & 1);
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(b);
            const bf16x8 bm = *reinterpret_cast<const bf16x8*>(b + 32);
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(b + 64);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t], 0, 0, 0);
        }
    }
}

// render + conv1 (fp32, k_vn_conv's) + conv2 + conv3 (bf16x3) of one state per wave, four waves per workgroup.  (The planes
// and a3out are not __restrict__: the stores to a3out inside the state loop keep the weight loads in it, instead of hoisted
// into ~430 registers.)
__global__ __launch_bounds__(256, 1) void k_vn_conv_x3(const float* __restrict__ P, const __bf16* planes,
                                                       const int8_t* __restrict__ states, const uint32_t* __restrict__ obs_key,
                                                       ReqList rq, int max_nodes, int n, float* a3out, int a3stride,
                                                       int32_t* tile_cnt, int tile_cnt_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_x3[];
    // k_vn_fc1's arrival counters start every evaluation at zero (k_vn_conv)
    if (blockIdx.x == 0)
        for (int t = threadIdx.x; t < (n + 31) / 32; t += 256) tile_cnt[(size_t)t * tile_cnt_stride] = 0;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    __bf16* a1 = reinterpret_cast<__bf16*>(smem_x3 + (size_t)w * X3_WAVE_BYTES);
    __bf16* a2 = a1;                  // (a2 overlays a1 once conv2's reads are complete)
    float* x0 = reinterpret_cast<float*>(smem_x3 + (size_t)w * X3_WAVE_BYTES + 144 * X3_ROW * 2);
    int brow2[3][9], brow3[2][9];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int p = 32 * t + l31, y = p / 6, x = p - 6 * y;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) brow2[t][tap] = ((y + tap / 3) * 8 + x + tap % 3) * X3_ROW + 8 * half;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int p = min(32 * t + l31, 55), y = p / 4, x = p - 4 * y;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) brow3[t][tap] = ((y + tap / 3) * 6 + x + tap % 3) * X3_ROW + 8 * half;
    }
    float bias2[16], bias3[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * half;
        bias2[r] = P[OFF_C2B + i];
        bias3[r] = P[OFF_C3B + i];
    }
    float w1[5];      // conv1 as in k_vn_conv: A operand of step st = W1[co = l31][k = 2 st + half], k = 9 is the zero pad
    int koff1[5];
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const int k = 2 * st + half;
        w1[st] = (k < 9) ? P[OFF_C1W + l31 * 9 + k] : 0.0f;
        koff1[st] = (k < 9) ? (k / 3) * 10 + (k % 3) : 0;
    }
    const bf16x8* W2 = reinterpret_cast<const bf16x8*>(planes) + lane;
    const bf16x8* W3 = reinterpret_cast<const bf16x8*>(planes + X3_PLANES) + lane;

    const int stride = gridDim.x * 4;
    int s = blockIdx.x * 4 + w;
    int incl = 0;
    if (!states) incl = req_prefix(rq, lane, n);
    if (!states && blockIdx.x == 0 && w == 0) req_publish_served(rq, incl, lane);      // (as k_vn_conv does)
    uint32_t kw_next = states ? 0u : req_obs_word(rq, incl, obs_key, max_nodes, n, s, lane);
    for (; s < n; s += stride) {
        const uint32_t kw = kw_next;
        // ---- input ----
        if (states) {
            for (int i = lane; i < 200; i += 64) x0[i] = (float)states[(size_t)s * 200 + i];
        } else {
            render_obs(kw, lane, x0);
            kw_next = req_obs_word(rq, incl, obs_key, max_nodes, n, s + stride, lane);   // (in flight under this state's work)
        }
        lds_fence();
        // ---- conv1: 144 positions = 5 tiles, fp32 matrix cores (k_vn_conv's arithmetic), stored as planes ----
#pragma unroll 1
        for (int t = 0; t < 5; ++t) {
            const int p = 32 * t + l31, pc = min(p, 143), base = (pc >> 3) * 10 + (pc & 7);
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = P[OFF_C1B + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
            for (int st = 0; st < 5; ++st)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[st], x0[base + koff1[st]], acc, 0, 0, 0);
            if (p < 144) store_planes<Relu>(a1 + p * X3_ROW, acc, half);
        }
        lds_fence();
        // ---- conv2: 96 positions = 3 tiles ----
        {
            f32x16 acc[3];
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = bias2[r];
            conv_x3_mfma<3>(a1, brow2, W2, acc);
            lds_fence();   // a2 overlays a1: every read of a1 is complete before the first write
#pragma unroll
            for (int t = 0; t < 3; ++t) store_planes<Relu>(a2 + (32 * t + l31) * X3_ROW, acc[t], half);
        }
        lds_fence();
        // ---- conv3: 56 positions = 2 tiles (the last 8 lanes of tile 1 are padding), fp32 out in k_vn_conv's layout ----
        {
            f32x16 acc[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = bias3[r];
            conv_x3_mfma<2>(a2, brow3, W3, acc);
            float* dst = a3out + (size_t)s * a3stride;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int p = 32 * t + l31;
                if (p < 56) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int i = (r & 3) + 8 * (r >> 2) + 4 * half;
                        const float v = acc[t][r];
                        dst[i * 56 + p] = v > 0.0f ? v : 0.0f;
                    }
                }
            }
        }
        lds_fence();
    }
}
