// The split-precision ("bf16x3") convolution kernel of the distributional head (included at the end of distnet.hip): the
// opt-in backend TM_VALUENET_BF16X3 of a TM_KIND_DIST search.  Same inputs and the same output as k_dn_conv (conv2's
// LeakyReLU'd output in the state's scratch row, flatten order co*64 + y*4 + x), so today's k_dn_fc consumes it unchanged.
//
// Numerics contract (DESIGN.md section 3.8; tests/test_dist_split_precision.py keeps a numpy emulation of it):
//   * every fp32 operand x of conv2 (its weights and the LeakyReLU'd conv1 activations) is split exactly into three bf16
//     planes with the plain round-to-nearest-even conversion: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)
//     (split3, bf16x3.h: the value net's);
//   * a product w*a is the sum of the six plane products with i + j <= 2, accumulated per MFMA step in the value net's
//     order: mid*mid, lo*hi, hi*lo, mid*hi, hi*mid, hi*hi (weight plane first).  Each is exact in fp32; the matrix core
//     accumulates in fp32.  Not bit-equal to k_dn_conv's fp32 fma chain (and not claimed to be);
//   * the reduction over k = tap * 32 + ci, tap = ky * 4 + kx, runs in 32 MFMA steps of 16 k (v_mfma_f32_32x32x16_bf16),
//     ascending; the accumulator starts at the bias;
//   * conv1 (its input is the rendered board, {-1, 0, 1}) stays on k_dn_conv's fp32 code, fc1, fc_v and the softmax on
//     k_dn_fc: the same bits as the fp32 backend for the same a2;
//   * one wave computes one state from its own inputs, with the same instructions whatever the batch: a state's outputs
//     depend on that state only, not on the batch size, its position in it or its neighbours, and are the same bits from
//     launch to launch.
#include "bf16x3.h"     // split3, bf16x8, bf16x4, X3_ROW, store_planes

// conv1's output in LDS: a row of X3_ROW bf16 (bf16x3.h) per position (133 = 19 x 7, row p = y * 7 + x).  Then the 22 x 10
// input board in fp32.
constexpr int X3_A1_BYTES = C1P * X3_ROW * 2;
constexpr int X3_WAVE_BYTES = X3_A1_BYTES + 220 * 4;          // 28 544: four waves = one workgroup per CU (111.5 of 160 KiB)
static_assert(X3_A1_BYTES % 16 == 0, "input board aligned");
constexpr int X3_STEPS = 16 * 32 / 16;                        // K = 16 taps x 32 channels, 16 per step
constexpr int X3_PLANES = X3_STEPS * 3 * 64 * 8;              // bf16 in the prepared planes: [step][plane][lane][8]
static_assert(X3_PLANES / 2 == TM_DISTNET_PREPARED_X3, "planes buffer");

// conv2's weights as bf16 planes in the A-operand order of v_mfma_f32_32x32x16_bf16: for step s (tap = s >> 1) lane l holds
// W[co = l & 31][ci = 16 (s & 1) + 8 (l >> 5) + j][tap] in element j of plane p at planes[(s * 3 + p) * 64 + l][j].
__global__ void k_dn_prepare_x3(const float* __restrict__ P, __bf16* __restrict__ planes) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;      // (s, lane, j)
    if (t >= X3_STEPS * 64 * 8) return;
    const int s = t / 512, l = (t / 8) % 64, j = t % 8;
    const int co = l & 31, ci = 16 * (s & 1) + 8 * (l >> 5) + j, tap = s >> 1;
    __bf16 h, m, lo;
    split3(P[OFF_C2W + co * 512 + ci * 16 + tap], h, m, lo);
    __bf16* dst = planes + (size_t)(s * 3) * 512 + l * 8 + j;
    dst[0] = h;
    dst[512] = m;
    dst[1024] = lo;
}

// conv2 over its two tiles of 32 output positions: D[co][position] += sum over the 32 steps of the six plane products, the
// tiles sharing each step's A planes.  in: the wave's conv1 rows; brow[t]: this lane's bf16 offset of the row its column reads
// at tap 0 (+ 8 (l >> 5) channels; a tap adds a constant); W: the planes (+ lane).
// Software pipeline (one wave per SIMD: nothing else hides a latency): the weight planes of step s + X3_AHEAD (global, L2) and
// the B operands of step s + 1 (LDS) are requested while the 12 MFMAs of step s issue; the ring's first X3_AHEAD steps are
// requested before conv1 (conv2_x3_prefetch).
constexpr int X3_AHEAD = 4;
__device__ __forceinline__ void x3_load_w(const bf16x8* W, int s, bf16x8 (&slot)[3]) {
#pragma unroll
    for (int p = 0; p < 3; ++p) slot[p] = W[(s * 3 + p) * 64];
}
__device__ __forceinline__ void conv2_x3_prefetch(const bf16x8* W, bf16x8 (&wr)[X3_AHEAD + 1][3]) {
#pragma unroll
    for (int s = 0; s < X3_AHEAD; ++s) x3_load_w(W, s, wr[s]);
}
__device__ __forceinline__ void x3_load_b(const __bf16* in, const int (&brow)[2], int s, bf16x8 (&b)[2][3]) {
    const int tap = s >> 1, off = ((tap >> 2) * 7 + (tap & 3)) * X3_ROW + 16 * (s & 1);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int p = 0; p < 3; ++p) b[t][p] = *reinterpret_cast<const bf16x8*>(in + brow[t] + off + 32 * p);
}
__device__ __forceinline__ void conv2_x3_mfma(const __bf16* in, const int (&brow)[2], const bf16x8* W,
                                              bf16x8 (&wr)[X3_AHEAD + 1][3], f32x16 (&acc)[2]) {
    bf16x8 bb[2][2][3];      // [buffer][tile][plane]
    x3_load_b(in, brow, 0, bb[0]);
#pragma unroll
    for (int s = 0; s < X3_STEPS; ++s) {
        if (s + X3_AHEAD < X3_STEPS) x3_load_w(W, s + X3_AHEAD, wr[(s + X3_AHEAD) % (X3_AHEAD + 1)]);
        if (s + 1 < X3_STEPS) x3_load_b(in, brow, s + 1, bb[(s + 1) & 1]);
        const bf16x8 (&a)[3] = wr[s % (X3_AHEAD + 1)];
        const bf16x8 (&b)[2][3] = bb[s & 1];
        // the six products of a tile in the contract's order (weight plane first; 0 hi, 1 mid, 2 lo), the two tiles
        // alternating (independent accumulators)
        constexpr int PW[6] = {1, 2, 0, 1, 0, 0}, PA[6] = {1, 0, 2, 0, 1, 0};
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int t = 0; t < 2; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PW[k]], b[t][PA[k]], acc[t], 0, 0, 0);
        // issue order inside the step: the weight loads up front, one LDS read behind each of the first six MFMAs
        if (s + X3_AHEAD < X3_STEPS) __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);
        if (s + 1 < X3_STEPS) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
        } else {
            __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// render + conv1 (fp32, k_dn_conv's) + conv2 (bf16x3) of one state per wave, four waves per workgroup, one workgroup per CU
// (the LDS), so one wave per SIMD: the next state's request and packed game are fetched one state ahead, as in k_dn_conv.
// (The planes and a2out are not __restrict__: the stores to a2out inside the state loop keep the weight loads in it,
// instead of hoisted out of it into hundreds of registers - valuenet_x3.inc's k_vn_conv_x3.)
__global__ __launch_bounds__(256, 1) void k_dn_conv_x3(const float* __restrict__ P, const __bf16* planes,
                                                       const int8_t* __restrict__ states, const uint32_t* __restrict__ node_game,
                                                       const int32_t* __restrict__ eval_obs, int max_nodes, int n, float* a2out,
                                                       int a2stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_x3[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    __bf16* a1 = reinterpret_cast<__bf16*>(smem_x3 + (size_t)w * X3_WAVE_BYTES);
    float* x0 = reinterpret_cast<float*>(smem_x3 + (size_t)w * X3_WAVE_BYTES + X3_A1_BYTES);
    int brow[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int p = 32 * t + l31, y = p >> 2, x = p & 3;
        brow[t] = (y * 7 + x) * X3_ROW + 8 * half;
    }
    float bias2[16], bias1[16], w1[8];
    int koff1[8];
#pragma unroll
    for (int r = 0; r < 16; ++r) bias2[r] = P[OFF_C2B + (r & 3) + 8 * (r >> 2) + 4 * half];
    conv1_setup(P, l31, half, bias1, w1, koff1);
    const bf16x8* W2 = reinterpret_cast<const bf16x8*>(planes) + lane;
    bf16x8 wr[X3_AHEAD + 1][3];      // conv2's weight ring

    const int stride = gridDim.x * 4;
    int s = blockIdx.x * 4 + w;
    int o_next = (!states && s < n) ? eval_obs[s] : 0;
    uint32_t gw_next = states ? 0u : game_word(node_game, max_nodes, n, s, o_next, lane);
    // the two hidden rows never change
    if (lane < 20) x0[lane] = 0.0f;
    for (; s < n; s += stride) {
        if (!load_input(states, node_game, eval_obs, max_nodes, n, s, s + stride, lane, o_next, gw_next, x0)) continue;
        conv2_x3_prefetch(W2, wr);       // (in flight under conv1)
        lds_fence();
        // ---- conv1: 133 positions = 5 tiles, fp32 matrix cores (k_dn_conv's arithmetic), stored as planes ----
#pragma unroll 1
        for (int t = 0; t < 5; ++t) {
            const f32x16 acc = conv1_tile(x0, t, l31, bias1, w1, koff1);
            const int p = 32 * t + l31;
            if (p < C1P) store_planes<Leaky>(a1 + p * X3_ROW, acc, half);
        }
        lds_fence();
        // ---- conv2: 64 positions = 2 tiles, straight to the scratch row of the state ----
        {
            f32x16 acc[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = bias2[r];
            conv2_x3_mfma(a1, brow, W2, wr, acc);
            store_a2(a2out + (size_t)s * a2stride, acc, half, l31);
        }
        lds_fence();
    }
}
