// Gradient step of the value net's online fit for gfx950: forward, loss and backward of model.Net + train.batch_loss in
// one C call (tm_valuenet_fit_grad), on the fp32 matrix cores.  DESIGN.md section 3.3 ("The gradient step of the fit") has the
// contract and the measurements.
//
// Every layer, forward and backward, is a matrix product D[M x N] = A[M x K] B[K x N] on v_mfma_f32_32x32x2_f32 (lane l
// supplies A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31], and holds D[i = (r&3) + 8 (r>>2) + 4 (l>>5)][j = l&31] in register
// r of 16).  A wave owns NT tiles of 32 x 32 that share their A operand and reads its operands straight from memory through
// the caches: an fp32 MFMA of this shape occupies the matrix core for 64 cycles, so one dword per lane and step is all the
// operand traffic there is, and no LDS staging is needed to feed it.  K is walked in QUADS of four steps; inside a quad the
// lane of half h = l>>5 takes k = 8 q + 4 h + r for step r (a permutation of K that both operands share), so that an operand
// that is contiguous along K is one 16-byte load per quad.
//
// Summation order: an MFMA accumulates its K terms as one sequential fp32 chain, and a chain of 288 or 1 792 terms is several
// times less accurate than the blocked sums of a CPU library (measured against torch: the loss at the trained checkpoints
// needed 21x torch's own fp32 error).  So K is summed in CHUNKS of four quads (32 terms) that start from zero, and the chunk
// sums are added to a running total on the vector ALU (fc1's 56 chunks with an error-free TwoSum).
//
// Activations are STORED by the forward (a1, a2, a3, h in the workspace) and read back by the backward, not recomputed.
// Gradients are kept with respect to the pre-activations (dz = da where the activation is > 0, else 0).
//
// Determinism: every output element, and every partial sum, is produced by one wave in one fixed order; batch reductions
// (weight and bias gradients, the loss) are partial sums in the workspace and a second stage that adds them in a fixed
// order.  There are no atomics.  All launch shapes follow from `batch` alone.
//
// The validation pass (tm_valuenet_fit_validate) is the same forward (forward(): the same kernels and instantiations, idx NULL)
// over the held-out rows, a slab at a time, k_vf_head<false> for the per-sample losses and k_fit_val_moments<0> for each chunk's
// {w, mean, population std}: what a row's loss is, and the order in which losses are added, are the gradient step's.
//
// The training rows' states come as int8 [rows][200] or as the packed observations of the engine, uint32 [rows][12]
// (tm_valuenet_fit_grad_packed, tm_valuenet_fit_validate_packed): the two kernels that read them (conv1's forward and weight
// gradient) take fit_mma.h's DenseStates or PackedStates as a template argument and get a cell's value from it; every statement
// after that is one text, so the packed calls write the bits of the int8 calls on the rendered rows.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/tetris_mcts_hip.h"
#include "fit_mma.h"      // what this file shares with distnet_fit.hip: the MFMA helpers, fc1, the second stages, the loss

namespace tmcts_vf {
using namespace tmcts_fit;

constexpr int A1 = 32 * 18 * 8, A2 = 32 * 16 * 6, A3 = 32 * 14 * 4, HID = 256;
constexpr int OFF_C1W = 0, OFF_C1B = 288, OFF_C2W = 320, OFF_C2B = 9536, OFF_C3W = 9568, OFF_C3B = 18784,
              OFF_F1W = 18816, OFF_F1B = 477568, OFF_FOW = 477824, OFF_FOB = 478336, NPARAM = 478338;
constexpr int MAX_BATCH = 1 << 20;      // N = B * 144 positions stay inside an int (element offsets are size_t)
constexpr int SPW = 4;                  // samples per wave of the convolutions' weight-gradient partials
constexpr int FC1_KC = 256;             // samples per split of fc1's weight gradient
constexpr int HEAD_CHUNK = 32;          // samples per partial of the small batch sums (fc_out, fc1 bias)
constexpr int HEAD_PART = 772;          // floats of such a partial: dW_out[2][256], db_fc1[256], db_out[2], pad

// The workspace, in floats (every segment starts at a multiple of four: 16-byte loads).
struct Layout {
    long long a1, a2, a3, dz1, dz2, dz3, h, dh, dzo, per, pf1, pw3, pw2, pw1, cb, hp, total;
    int s1, chunks, hchunks;
};
__host__ inline Layout layout(int B) {
    Layout L;
    long long o = 0, b = B;
    L.s1 = (B + FC1_KC - 1) / FC1_KC;
    L.chunks = (B + SPW - 1) / SPW;
    L.hchunks = (B + HEAD_CHUNK - 1) / HEAD_CHUNK;
    L.a1 = o; o += b * A1;
    L.a2 = o; o += b * A2;
    L.a3 = o; o += b * A3;
    L.dz1 = o; o += b * A1;
    L.dz2 = o; o += b * A2;
    L.dz3 = o; o += b * A3;
    L.h = o; o += b * HID;
    L.dh = o; o += b * HID;
    L.dzo = o; o += up4(b * 2);
    L.per = o; o += up4(b * 2);                       // doubles
    L.pf1 = o; o += (long long)L.s1 * HID * A3;
    L.pw3 = o; o += (long long)L.chunks * 9216;
    L.pw2 = o; o += (long long)L.chunks * 9216;
    L.pw1 = o; o += (long long)L.chunks * 288;
    L.cb = o; o += b * 96;
    L.hp = o; o += (long long)L.hchunks * HEAD_PART;
    L.total = o;
    return L;
}

// ---- forward convolution: z[co][b, p] = bias[co] + sum_k W[co][k] in[b][ci][(y + ky) IW + x + kx], ReLU ----
// M = 32 output channels, N = B * OP positions, K = CIN * 9.  CIN == 1: the input is the state of row idx[b], read through SRC
// (fit_mma.h: int8 cells or a packed observation); a lane keeps the strip of its position's three rows per tile.
template <int CIN, int IH, int IW, int NT, typename SRC = DenseStates>
__global__ __launch_bounds__(256) void k_vf_conv_fwd(const float* __restrict__ W, const float* __restrict__ bias,
                                                     const float* __restrict__ in, const typename SRC::elem* __restrict__ states,
                                                     const int64_t* __restrict__ idx, int B, float* __restrict__ out) {
    constexpr int OW = IW - 2, OP = (IH - 2) * OW, IP = IH * IW, K = CIN * 9, KQ = (K + 7) / 8;
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NT * 32, N = B * OP;
    if (n0 >= N) return;
    bool ok[NT];
    int nb[NT], np[NT], ny[NT], nx[NT];
    size_t base[NT];
    typename SRC::Strip cells[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = n0 + 32 * t + l31;
        ok[t] = n < N;
        const int nn = ok[t] ? n : 0, b = nn / OP, p = nn - b * OP, y = p / OW, x = p - y * OW;
        nb[t] = b;
        np[t] = p;
        ny[t] = y;
        nx[t] = x;
        base[t] = (size_t)b * (CIN * IP) + y * IW + x;
        if constexpr (CIN == 1) cells[t] = SRC::strip(SRC::row(states, row_of(idx, b)), y);
    }
    f32x16 tot[NT], acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[t][r] = bias[drow(r, half)];
#pragma unroll 1
    for (int qc = 0; qc < KQ; qc += CHUNK_QUADS) {
        vf_zero<NT>(acc);
#pragma unroll
        for (int q = qc; q < (qc + CHUNK_QUADS < KQ ? qc + CHUNK_QUADS : KQ); ++q) {
            const int k0 = 8 * q + 4 * half;
            float av[4], bv[NT][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = k0 + r;
                const bool kin = (K % 8 == 0) || k < K;
                const int kk = kin ? k : 0, ci = kk / 9, rr = kk - 9 * ci, ky = rr / 3, kx = rr - 3 * ky;
                const int koff = ci * IP + ky * IW + kx;
                av[r] = kin ? W[l31 * K + kk] : 0.0f;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    float v = 0.0f;
                    if (kin && ok[t]) v = (CIN == 1) ? SRC::cell(cells[t], ny[t] + ky, nx[t] + kx) : in[base[t] + koff];
                    bv[t][r] = v;
                }
            }
            float4 b4[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) b4[t] = make_float4(bv[t][0], bv[t][1], bv[t][2], bv[t][3]);
            vf_quad<NT>(acc, make_float4(av[0], av[1], av[2], av[3]), b4);
        }
        vf_add<NT>(tot, acc);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (ok[t]) {
            float* dst = out + (size_t)nb[t] * (32 * OP) + np[t];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = tot[t][r];
                dst[drow(r, half) * OP] = v > 0.0f ? v : 0.0f;
            }
        }
}

// ---- output layer, loss and their gradients: one wave per sample, in double ----
// per = log var_p + ((value - v_p)^2 + max(variance, clip)) / var_p - log max(variance, clip) - 1, times the weight;
// dzo[b][2] = d(mean of per) / d(fc_out pre-activation), dh[b][i] = (dzo . W_out[:, i]) where h > 0.
// GRAD = false (the validation pass): per alone, by the same statements; dzo and dh are not touched.
// div: what the per-sample weight is divided by in the gradients - the batch for the gradient of the MEAN (tm_valuenet_fit_grad),
// 1 for the per-sample gradients of the Fisher pass.
template <bool GRAD>
__global__ __launch_bounds__(256) void k_vf_head(const float* __restrict__ P, const float* __restrict__ bounds,
                                                 const float* __restrict__ h, const float* __restrict__ value,
                                                 const float* __restrict__ variance, const float* __restrict__ weight,
                                                 const int64_t* __restrict__ idx, int B, int weighted, float clip, double div,
                                                 float* __restrict__ dzo, double* __restrict__ per, float* __restrict__ dh) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float4 h4 = *reinterpret_cast<const float4*>(h + (size_t)b * HID + 4 * lane);
    const float* w0 = P + OFF_FOW + 4 * lane;
    const float* w1 = w0 + HID;
    const float hv[4] = {h4.x, h4.y, h4.z, h4.w};
    double z0 = 0.0, z1 = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        z0 += (double)hv[r] * (double)w0[r];
        z1 += (double)hv[r] * (double)w1[r];
    }
    const double z[2] = {wave_sum(z0) + (double)P[OFF_FOB], wave_sum(z1) + (double)P[OFF_FOB + 1]};
    double s[2], ds[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double e = exp(-fabs(z[j])), d = 1.0 + e;       // sigmoid and its derivative without overflow
        s[j] = z[j] >= 0.0 ? 1.0 / d : e / d;
        ds[j] = e / (d * d);
    }
    const double vp = s[0] * (double)bounds[0] + (double)bounds[2], varp = s[1] * (double)bounds[1] + (double)bounds[3];
    const size_t row = row_of(idx, b);
    const double val = (double)value[row], vt = (double)fmaxf(variance[row], clip), w = weighted ? (double)weight[row] : 1.0;
    const double diff = val - vp, num = diff * diff + vt;
    if (lane == 0) per[b] = w * (log(varp) + num / varp - log(vt) - 1.0);
    if (!GRAD) return;
    const double scale = w / div;
    const double dvp = -2.0 * diff / varp * scale, dvarp = (1.0 / varp - num / (varp * varp)) * scale;
    const double g0 = dvp * (double)bounds[0] * ds[0], g1 = dvarp * (double)bounds[1] * ds[1];
    if (lane == 0) {
        dzo[2 * b] = (float)g0;
        dzo[2 * b + 1] = (float)g1;
    }
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = hv[r] > 0.0f ? (float)(g0 * (double)w0[r] + g1 * (double)w1[r]) : 0.0f;
    *reinterpret_cast<float4*>(dh + (size_t)b * HID + 4 * lane) = make_float4(o[0], o[1], o[2], o[3]);
}

// partial sums over HEAD_CHUNK samples of dW_out = dzo^T h, db_fc1 = sum dh, db_out = sum dzo
// SQ (the Fisher pass): of the squares of the per-sample terms, dzo^2 h^2, dh^2, dzo^2
template <bool SQ>
__global__ __launch_bounds__(256) void k_vf_head_part(const float* __restrict__ dzo, const float* __restrict__ h,
                                                      const float* __restrict__ dh, int B, float* __restrict__ part) {
    const int i = threadIdx.x, b0 = blockIdx.x * HEAD_CHUNK, b1 = min(B, b0 + HEAD_CHUNK);
    float w0 = 0.f, w1 = 0.f, bf = 0.f, bo = 0.f;
    for (int b = b0; b < b1; ++b) {
        float g0 = dzo[2 * b], g1 = dzo[2 * b + 1], hv = h[(size_t)b * HID + i], d = dh[(size_t)b * HID + i];
        if constexpr (SQ) {
            g0 = g0 * g0;
            g1 = g1 * g1;
            hv = hv * hv;
            d = d * d;
        }
        w0 = fmaf(g0, hv, w0);
        w1 = fmaf(g1, hv, w1);
        bf += d;
        if (i < 2) bo += i == 0 ? g0 : g1;
    }
    float* dst = part + (size_t)blockIdx.x * HEAD_PART;
    dst[i] = w0;
    dst[HID + i] = w1;
    dst[2 * HID + i] = bf;
    if (i < 2) dst[3 * HID + i] = bo;
}

// ---- fc1 weight gradient: part[s][j][k] = sum over the samples of split s of dh[b][j] a3[b][k]; M = 256, N = 1792 ----
// (a split is ONE chain here and chunks of 32 in distnet_fit.hip's k_df_fc_dw: one kernel for both would change this one's bits)
// SQ (the Fisher pass): both operands are squared as they are loaded - the sum over the samples of the squared outer products
// (dh[b][j] a3[b][k])^2 is the matrix product of the squared operands.
template <int NT, bool SQ = false>
__global__ __launch_bounds__(256) void k_vf_fc1_dw(const float* __restrict__ dh, const float* __restrict__ a3, int B,
                                                   float* __restrict__ part) {
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    constexpr int NG = A3 / 32 / NT;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), ng = wave % NG, mt = (wave / NG) & 7, s = wave / (NG * 8);
    const int b0 = s * FC1_KC, b1 = min(B, b0 + FC1_KC);
    if (b0 >= B) return;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const float* acol = dh + 32 * mt + l31;
    const float* bcol = a3 + ng * NT * 32 + l31;
    for (int bq = b0; bq < b1; bq += 8) {
        float av[4];
        float bv[NT][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = bq + 4 * half + r;
            const bool in = b < b1;
            const size_t bb = in ? b : b0;
            av[r] = in ? acol[bb * HID] : 0.0f;
#pragma unroll
            for (int t = 0; t < NT; ++t) bv[t][r] = in ? bcol[bb * A3 + 32 * t] : 0.0f;
            if constexpr (SQ) {
                av[r] = av[r] * av[r];
#pragma unroll
                for (int t = 0; t < NT; ++t) bv[t][r] = bv[t][r] * bv[t][r];
            }
        }
        float4 b4[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) b4[t] = make_float4(bv[t][0], bv[t][1], bv[t][2], bv[t][3]);
        vf_quad<NT>(acc, make_float4(av[0], av[1], av[2], av[3]), b4);
    }
    float* dst = part + (size_t)s * (HID * A3) + (size_t)(32 * mt) * A3 + ng * NT * 32 + l31;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(size_t)drow(r, half) * A3 + 32 * t] = acc[t][r];
}

// ---- convolution data gradient: dzi[b][ci][u] = (sum_{co,ky,kx} dzo[b][co][(uy - ky, ux - kx)] W[co][ci][ky][kx]) where
// ain[b][ci][u] > 0; the output gradient counts as zero outside its OH x OW.  M = 32 input channels, N = B * IP, K = 288 ----
template <int IH, int IW, int NT>
__global__ __launch_bounds__(256) void k_vf_conv_bwd_data(const float* __restrict__ W, const float* __restrict__ dzo,
                                                          const float* __restrict__ ain, int B, float* __restrict__ dzi) {
    constexpr int OH = IH - 2, OW = IW - 2, OP = OH * OW, IP = IH * IW;
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NT * 32, N = B * IP;
    if (n0 >= N) return;
    bool ok[NT];
    int uy[NT], ux[NT];
    size_t ob[NT], ib[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = n0 + 32 * t + l31;
        ok[t] = n < N;
        const int nn = ok[t] ? n : 0, b = nn / IP, u = nn - b * IP;
        uy[t] = u / IW;
        ux[t] = u - uy[t] * IW;
        ob[t] = (size_t)b * (32 * OP);
        ib[t] = (size_t)b * (32 * IP) + u;
    }
    // (one chain of 288 terms per element: chunked sums cost this kernel a wave per SIMD in registers and its gradients
    //  are inside the accuracy rule without them)
    f32x16 tot[NT];
    vf_zero<NT>(tot);
#pragma unroll 2
    for (int q = 0; q < 36; ++q) {
        const int k0 = 8 * q + 4 * half;
        float av[4], bv[NT][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + r, co = k / 9, rr = k - 9 * co, ky = rr / 3, kx = rr - 3 * ky;
            av[r] = W[co * 288 + l31 * 9 + rr];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int oy = uy[t] - ky, ox = ux[t] - kx;
                const bool in = ok[t] && oy >= 0 && oy < OH && ox >= 0 && ox < OW;
                bv[t][r] = in ? dzo[ob[t] + co * OP + oy * OW + ox] : 0.0f;
            }
        }
        float4 b4[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) b4[t] = make_float4(bv[t][0], bv[t][1], bv[t][2], bv[t][3]);
        vf_quad<NT>(tot, make_float4(av[0], av[1], av[2], av[3]), b4);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (ok[t]) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const size_t o = ib[t] + (size_t)drow(r, half) * IP;
                dzi[o] = ain[o] > 0.0f ? tot[t][r] : 0.0f;
            }
        }
}

// ---- convolution weight gradient: part[chunk][co][n = (ci,ky,kx)] = sum over the chunk's SPW samples and the OP positions of
// dzo[b][co][p] ain[b][ci][(y + ky) IW + x + kx].  M = 32, N = CIN * 9 (NT tiles per wave), K = (sample, position) ----
// CIN == 1: ain is the state of row idx[b], read through SRC.  A lane's tap is fixed and the loop walks the positions, so the
// strip is built per quad of positions (with OW == 8 a quad lies in one row) from the row the lane keeps per sample.
// SQ (the Fisher pass): after each sample's positions acc holds that sample's gradient; its square is added to a second set of
// accumulators and acc starts the next sample from zero, so a partial is the sum over its samples of the squared per-sample gradients.
template <int CIN, int IH, int IW, int NT, typename SRC = DenseStates, bool SQ = false>
__global__ __launch_bounds__(256) void k_vf_conv_dw(const float* __restrict__ dzo, const float* __restrict__ ain,
                                                    const typename SRC::elem* __restrict__ states,
                                                    const int64_t* __restrict__ idx, int B, float* __restrict__ part) {
    constexpr int OW = IW - 2, OP = (IH - 2) * OW, IP = IH * IW, KW = CIN * 9, NG = (KW + 32 * NT - 1) / (32 * NT);
    static_assert(OP % 8 == 0, "a quad of K stays inside one sample");
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), ng = wave % NG, chunk = wave / NG;
    const int b0 = chunk * SPW, b1 = min(B, b0 + SPW);
    if (b0 >= B) return;
    bool nok[NT];
    int noff[NT], nky[NT], nkx[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = (ng * NT + t) * 32 + l31;
        nok[t] = n < KW;
        const int nn = nok[t] ? n : 0, ci = nn / 9, rr = nn - 9 * ci, ky = rr / 3, kx = rr - 3 * ky;
        noff[t] = ci * IP + ky * IW + kx;
        nky[t] = ky;
        nkx[t] = kx;
    }
    f32x16 acc[NT];
    [[maybe_unused]] f32x16 sq[SQ ? NT : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[t][r] = 0.0f;
            if constexpr (SQ) sq[t][r] = 0.0f;
        }
    for (int b = b0; b < b1; ++b) {
        const float* arow = dzo + (size_t)b * (32 * OP) + l31 * OP + 4 * half;
        const size_t ibase = (size_t)b * (CIN * IP);
        typename SRC::Row srow;
        if constexpr (CIN == 1) srow = SRC::row(states, row_of(idx, b));
#pragma unroll 2
        for (int q = 0; q < OP / 8; ++q) {
            const float4 a = *reinterpret_cast<const float4*>(arow + 8 * q);
            float bv[NT][4];
            typename SRC::Strip cells[NT];
            if constexpr (CIN == 1) {
                static_assert(CIN != 1 || OW == 8, "a quad of positions lies in one row of the output");
#pragma unroll
                for (int t = 0; t < NT; ++t) cells[t] = SRC::strip(srow, q + nky[t]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = 8 * q + 4 * half + r, y = p / OW, x = p - y * OW, poff = y * IW + x;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    float v = 0.0f;
                    if (nok[t]) v = (CIN == 1) ? SRC::cell(cells[t], y + nky[t], x + nkx[t]) : ain[ibase + noff[t] + poff];
                    bv[t][r] = v;
                }
            }
            float4 b4[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) b4[t] = make_float4(bv[t][0], bv[t][1], bv[t][2], bv[t][3]);
            vf_quad<NT>(acc, a, b4);
        }
        if constexpr (SQ) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    sq[t][r] += acc[t][r] * acc[t][r];
                    acc[t][r] = 0.0f;
                }
        }
    }
    float* dst = part + (size_t)chunk * (32 * KW);
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (nok[t]) {
            const int n = (ng * NT + t) * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if constexpr (SQ) dst[drow(r, half) * KW + n] = sq[t][r];
                else dst[drow(r, half) * KW + n] = acc[t][r];
            }
        }
}

// per sample, the sums over positions of dz1 / dz2 / dz3 per channel: cb[b][96] (conv1, conv2, conv3); SQ (the Fisher pass): their
// squares
template <bool SQ>
__global__ __launch_bounds__(128) void k_vf_conv_bias_part(const float* __restrict__ dz1, const float* __restrict__ dz2,
                                                           const float* __restrict__ dz3, int B, float* __restrict__ cb) {
    const int b = blockIdx.x, i = threadIdx.x;
    if (i >= 96 || b >= B) return;
    const int layer = i >> 5, c = i & 31, op = layer == 0 ? 144 : layer == 1 ? 96 : 56;
    const float* src = (layer == 0 ? dz1 + (size_t)b * A1 : layer == 1 ? dz2 + (size_t)b * A2 : dz3 + (size_t)b * A3) + c * op;
    float s = 0.0f;
    for (int p = 0; p < op; p += 4) {
        const float4 v = *reinterpret_cast<const float4*>(src + p);
        s += (v.x + v.y) + (v.z + v.w);
    }
    cb[(size_t)b * 96 + i] = SQ ? s * s : s;
}

// the forward of B rows (states: SRC's rows, int8 [.][200] or packed [.][12]; row idx[b], or row b when idx is NULL) into a1, a2,
// a3, h: the launches of the gradient step and of the validation pass
template <typename SRC>
static void forward(const float* P, const typename SRC::elem* states, const int64_t* idx, int B, float* a1, float* a2, float* a3,
                    float* h, hipStream_t st) {
    hipLaunchKernelGGL((k_vf_conv_fwd<1, 20, 10, 3, SRC>), dim3(blocks_for_waves((tiles((long long)B * 144) + 2) / 3)), dim3(256), 0, st,
                       P + OFF_C1W, P + OFF_C1B, (const float*)nullptr, states, idx, B, a1);
    hipLaunchKernelGGL((k_vf_conv_fwd<32, 18, 8, 3>), dim3(blocks_for_waves((tiles((long long)B * 96) + 2) / 3)), dim3(256), 0, st,
                       P + OFF_C2W, P + OFF_C2B, a1, (const int8_t*)nullptr, (const int64_t*)nullptr, B, a2);
    hipLaunchKernelGGL((k_vf_conv_fwd<32, 16, 6, 2>), dim3(blocks_for_waves((tiles((long long)B * 56) + 1) / 2)), dim3(256), 0, st,
                       P + OFF_C3W, P + OFF_C3B, a2, (const int8_t*)nullptr, (const int64_t*)nullptr, B, a3);
    hipLaunchKernelGGL((k_fit_fc1_fwd<HID, A3, Relu, 1>), dim3(blocks_for_waves(8 * tiles(B))), dim3(256), 0, st, P + OFF_F1W, P + OFF_F1B, a3, B, h);
}

// the validation pass's workspace, in floats: the forward's activations of one slab and its per-row losses (doubles)
struct ValLayout {
    long long a1, a2, a3, h, per, total;
};
__host__ inline ValLayout val_layout(int slab) {
    ValLayout L;
    long long o = 0, b = slab;
    L.a1 = o; o += b * A1;
    L.a2 = o; o += b * A2;
    L.a3 = o; o += b * A3;
    L.h = o; o += b * HID;
    L.per = o; o += up4(b * 2);
    L.total = o;
    return L;
}

// the gradient step on either kind of rows: tm_valuenet_fit_grad (DenseStates) and tm_valuenet_fit_grad_packed (PackedStates)
template <typename SRC>
static int fit_grad(const float* params, const float* out_bounds, const typename SRC::elem* states, const float* value,
                    const float* variance, const float* weight, const int64_t* idx, int batch, int weighted,
                    float variance_clip, float* grad, float* loss, float* workspace, void* stream_) {
    if (!params || !out_bounds || !states || !value || !variance || !weight || !grad || !loss || !workspace)
        return (int)hipErrorInvalidValue;
    if (batch < 1 || batch > MAX_BATCH || ((uintptr_t)workspace & 15)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream_;
    const int B = batch;
    const Layout L = layout(B);
    float* ws = workspace;
    float *a1 = ws + L.a1, *a2 = ws + L.a2, *a3 = ws + L.a3, *dz1 = ws + L.dz1, *dz2 = ws + L.dz2, *dz3 = ws + L.dz3;
    float *h = ws + L.h, *dh = ws + L.dh, *dzo = ws + L.dzo, *pf1 = ws + L.pf1, *pw3 = ws + L.pw3, *pw2 = ws + L.pw2;
    float *pw1 = ws + L.pw1, *cb = ws + L.cb, *hp = ws + L.hp;
    double* per = reinterpret_cast<double*>(ws + L.per);
    const float* P = params;
    // ---- forward ----
    forward<SRC>(P, states, idx, B, a1, a2, a3, h, st);
    // ---- output layer, loss, and the small batch sums ----
    hipLaunchKernelGGL(k_vf_head<true>, dim3((B + 3) / 4), dim3(256), 0, st, P, out_bounds, h, value, variance, weight, idx, B, weighted,
                       variance_clip, (double)B, dzo, per, dh);
    hipLaunchKernelGGL(k_fit_loss<0>, dim3(1), dim3(256), 0, st, per, B, loss);
    hipLaunchKernelGGL(k_vf_head_part<false>, dim3(L.hchunks), dim3(256), 0, st, dzo, h, dh, B, hp);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3((512 + 15) / 16), dim3(256), 0, st, hp, L.hchunks, (long long)HEAD_PART, 512, grad + OFF_FOW);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(256 / 16), dim3(256), 0, st, hp + 512, L.hchunks, (long long)HEAD_PART, 256, grad + OFF_F1B);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(1), dim3(256), 0, st, hp + 768, L.hchunks, (long long)HEAD_PART, 2, grad + OFF_FOB);
    // ---- fc1 backward ----
    hipLaunchKernelGGL((k_vf_fc1_dw<2>), dim3(blocks_for_waves((long long)L.s1 * 8 * 28)), dim3(256), 0, st, dh, a3, B, pf1);
    hipLaunchKernelGGL((k_fit_reduce<4>), dim3(HID * A3 / 64), dim3(256), 0, st, pf1, L.s1, (long long)HID * A3, HID * A3, grad + OFF_F1W);
    hipLaunchKernelGGL((k_fit_fc1_bwd_data<HID, A3, Relu, 2>), dim3(blocks_for_waves(tiles(B) * 28)), dim3(256), 0, st, P + OFF_F1W, dh, a3, B, dz3);
    // ---- convolutions backward ----
    hipLaunchKernelGGL((k_vf_conv_dw<32, 16, 6, 3>), dim3(blocks_for_waves((long long)L.chunks * 3)), dim3(256), 0, st, dz3, a2,
                       (const int8_t*)nullptr, (const int64_t*)nullptr, B, pw3);
    hipLaunchKernelGGL((k_vf_conv_bwd_data<16, 6, 3>), dim3(blocks_for_waves((tiles((long long)B * 96) + 2) / 3)), dim3(256), 0, st,
                       P + OFF_C3W, dz3, a2, B, dz2);
    hipLaunchKernelGGL((k_vf_conv_dw<32, 18, 8, 3>), dim3(blocks_for_waves((long long)L.chunks * 3)), dim3(256), 0, st, dz2, a1,
                       (const int8_t*)nullptr, (const int64_t*)nullptr, B, pw2);
    hipLaunchKernelGGL((k_vf_conv_bwd_data<18, 8, 3>), dim3(blocks_for_waves((tiles((long long)B * 144) + 2) / 3)), dim3(256), 0, st,
                       P + OFF_C2W, dz2, a1, B, dz1);
    hipLaunchKernelGGL((k_vf_conv_dw<1, 20, 10, 1, SRC>), dim3(blocks_for_waves(L.chunks)), dim3(256), 0, st, dz1, (const float*)nullptr,
                       states, idx, B, pw1);
    hipLaunchKernelGGL(k_vf_conv_bias_part<false>, dim3(B), dim3(128), 0, st, dz1, dz2, dz3, B, cb);
    // ---- second stages of the convolutions' sums ----
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(9216 / 16), dim3(256), 0, st, pw3, L.chunks, 9216LL, 9216, grad + OFF_C3W);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(9216 / 16), dim3(256), 0, st, pw2, L.chunks, 9216LL, 9216, grad + OFF_C2W);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(288 / 16), dim3(256), 0, st, pw1, L.chunks, 288LL, 288, grad + OFF_C1W);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(2), dim3(256), 0, st, cb, B, 96LL, 32, grad + OFF_C1B);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(2), dim3(256), 0, st, cb + 32, B, 96LL, 32, grad + OFF_C2B);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(2), dim3(256), 0, st, cb + 64, B, 96LL, 32, grad + OFF_C3B);
    return (int)hipGetLastError();
}

// the validation pass on either kind of rows
template <typename SRC>
static int fit_validate(const float* params, const float* out_bounds, const typename SRC::elem* states, const float* value,
                        const float* variance, const float* weight, long long n, int chunk, int slab, int weighted,
                        float variance_clip, double* rows_out, float* workspace, void* stream_) {
    if (!params || !out_bounds || !states || !value || !variance || !weight || !rows_out || !workspace)
        return (int)hipErrorInvalidValue;
    if (n < 1 || chunk < 1 || slab < chunk || slab > MAX_BATCH || slab % chunk) return (int)hipErrorInvalidValue;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)rows_out & 7)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream_;
    const ValLayout L = val_layout(slab);
    float *a1 = workspace + L.a1, *a2 = workspace + L.a2, *a3 = workspace + L.a3, *h = workspace + L.h;
    double* per = reinterpret_cast<double*>(workspace + L.per);
    // slab by slab on the one stream: a slab's kernels have read the workspace before the next slab's overwrite it
    for (long long r0 = 0; r0 < n; r0 += slab) {
        const int B = (int)(n - r0 < slab ? n - r0 : slab);
        forward<SRC>(params, states + r0 * SRC::STRIDE, (const int64_t*)nullptr, B, a1, a2, a3, h, st);
        hipLaunchKernelGGL(k_vf_head<false>, dim3((B + 3) / 4), dim3(256), 0, st, params, out_bounds, h, value + r0, variance + r0,
                           weight + r0, (const int64_t*)nullptr, B, weighted, variance_clip, 1.0, (float*)nullptr, per, (float*)nullptr);
        hipLaunchKernelGGL(k_fit_val_moments<0>, dim3((B + chunk - 1) / chunk), dim3(256), 0, st, per, weight + r0, B, chunk, weighted,
                           rows_out + 3 * (r0 / chunk));
    }
    return (int)hipGetLastError();
}

// ---- the Fisher pass: F[i] = (1/n) sum_b (d loss_b / d p_i)^2 over n rows, a slab at a time ----
// A slab is the gradient step's forward, k_vf_head with the divisor 1 (dzo and dh are then PER-SAMPLE gradients) and its data
// gradients as they are, and the SQ forms of the weight-gradient kernels, whose partials hold sums over samples of squared
// per-sample gradients; the unchanged second stages add them into a temporary [NPARAM], which k_vf_fisher_add adds to a double
// accumulator, slab after slab in stream order.  The workspace is the gradient step's of `slab` rows, then the temporary, then
// the accumulator.
constexpr long long FISHER_TMP = up4(NPARAM), FISHER_ACC = 2LL * NPARAM;      // floats (the accumulator: NPARAM doubles)
static_assert(FISHER_ACC % 4 == 0, "every segment starts at a multiple of four floats");

// acc[i] = (first ? 0 : acc[i]) + tmp[i]; after the last slab fisher[i] = (float)(acc[i] / n)
__global__ __launch_bounds__(256) void k_vf_fisher_add(const float* __restrict__ tmp, double* __restrict__ acc, int first, int last,
                                                       double n, float* __restrict__ fisher) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NPARAM) return;
    const double a = (first ? 0.0 : acc[i]) + (double)tmp[i];
    acc[i] = a;
    if (last) fisher[i] = (float)(a / n);
}

template <typename SRC>
static int fit_fisher(const float* params, const float* out_bounds, const typename SRC::elem* states, const float* value,
                      const float* variance, const float* weight, const int64_t* idx, long long n, int slab, int weighted,
                      float variance_clip, float* fisher, float* workspace, void* stream_) {
    if (!params || !out_bounds || !states || !value || !variance || !weight || !fisher || !workspace)
        return (int)hipErrorInvalidValue;
    if (n < 1 || slab < 1 || slab > MAX_BATCH || ((uintptr_t)workspace & 15)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream_;
    const Layout L = layout(slab);
    float* ws = workspace;
    float *a1 = ws + L.a1, *a2 = ws + L.a2, *a3 = ws + L.a3, *dz1 = ws + L.dz1, *dz2 = ws + L.dz2, *dz3 = ws + L.dz3;
    float *h = ws + L.h, *dh = ws + L.dh, *dzo = ws + L.dzo, *pf1 = ws + L.pf1, *pw3 = ws + L.pw3, *pw2 = ws + L.pw2;
    float *pw1 = ws + L.pw1, *cb = ws + L.cb, *hp = ws + L.hp, *tmp = ws + L.total;
    double *per = reinterpret_cast<double*>(ws + L.per), *acc = reinterpret_cast<double*>(ws + L.total + FISHER_TMP);
    const float* P = params;
    // slab by slab on the one stream: a slab's kernels have read the workspace before the next slab's overwrite it
    for (long long r0 = 0; r0 < n; r0 += slab) {
        const int B = (int)(n - r0 < slab ? n - r0 : slab);
        const int s1 = (B + FC1_KC - 1) / FC1_KC, chunks = (B + SPW - 1) / SPW, hchunks = (B + HEAD_CHUNK - 1) / HEAD_CHUNK;
        // rows idx[r0 + b]; without idx the rows r0 + b
        const int64_t* ix = idx ? idx + r0 : nullptr;
        const long long base = idx ? 0 : r0;
        const typename SRC::elem* S = states + base * SRC::STRIDE;
        forward<SRC>(P, S, ix, B, a1, a2, a3, h, st);
        hipLaunchKernelGGL(k_vf_head<true>, dim3((B + 3) / 4), dim3(256), 0, st, P, out_bounds, h, value + base, variance + base,
                           weight + base, ix, B, weighted, variance_clip, 1.0, dzo, per, dh);
        hipLaunchKernelGGL(k_vf_head_part<true>, dim3(hchunks), dim3(256), 0, st, dzo, h, dh, B, hp);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3((512 + 15) / 16), dim3(256), 0, st, hp, hchunks, (long long)HEAD_PART, 512, tmp + OFF_FOW);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(256 / 16), dim3(256), 0, st, hp + 512, hchunks, (long long)HEAD_PART, 256, tmp + OFF_F1B);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(1), dim3(256), 0, st, hp + 768, hchunks, (long long)HEAD_PART, 2, tmp + OFF_FOB);
        hipLaunchKernelGGL((k_vf_fc1_dw<2, true>), dim3(blocks_for_waves((long long)s1 * 8 * 28)), dim3(256), 0, st, dh, a3, B, pf1);
        hipLaunchKernelGGL((k_fit_reduce<4>), dim3(HID * A3 / 64), dim3(256), 0, st, pf1, s1, (long long)HID * A3, HID * A3, tmp + OFF_F1W);
        hipLaunchKernelGGL((k_fit_fc1_bwd_data<HID, A3, Relu, 2>), dim3(blocks_for_waves(tiles(B) * 28)), dim3(256), 0, st, P + OFF_F1W, dh, a3, B, dz3);
        hipLaunchKernelGGL((k_vf_conv_dw<32, 16, 6, 3, DenseStates, true>), dim3(blocks_for_waves((long long)chunks * 3)), dim3(256), 0, st, dz3, a2,
                           (const int8_t*)nullptr, (const int64_t*)nullptr, B, pw3);
        hipLaunchKernelGGL((k_vf_conv_bwd_data<16, 6, 3>), dim3(blocks_for_waves((tiles((long long)B * 96) + 2) / 3)), dim3(256), 0, st,
                           P + OFF_C3W, dz3, a2, B, dz2);
        hipLaunchKernelGGL((k_vf_conv_dw<32, 18, 8, 3, DenseStates, true>), dim3(blocks_for_waves((long long)chunks * 3)), dim3(256), 0, st, dz2, a1,
                           (const int8_t*)nullptr, (const int64_t*)nullptr, B, pw2);
        hipLaunchKernelGGL((k_vf_conv_bwd_data<18, 8, 3>), dim3(blocks_for_waves((tiles((long long)B * 144) + 2) / 3)), dim3(256), 0, st,
                           P + OFF_C2W, dz2, a1, B, dz1);
        hipLaunchKernelGGL((k_vf_conv_dw<1, 20, 10, 1, SRC, true>), dim3(blocks_for_waves(chunks)), dim3(256), 0, st, dz1, (const float*)nullptr,
                           S, ix, B, pw1);
        hipLaunchKernelGGL(k_vf_conv_bias_part<true>, dim3(B), dim3(128), 0, st, dz1, dz2, dz3, B, cb);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(9216 / 16), dim3(256), 0, st, pw3, chunks, 9216LL, 9216, tmp + OFF_C3W);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(9216 / 16), dim3(256), 0, st, pw2, chunks, 9216LL, 9216, tmp + OFF_C2W);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(288 / 16), dim3(256), 0, st, pw1, chunks, 288LL, 288, tmp + OFF_C1W);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(2), dim3(256), 0, st, cb, B, 96LL, 32, tmp + OFF_C1B);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(2), dim3(256), 0, st, cb + 32, B, 96LL, 32, tmp + OFF_C2B);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(2), dim3(256), 0, st, cb + 64, B, 96LL, 32, tmp + OFF_C3B);
        hipLaunchKernelGGL(k_vf_fisher_add, dim3((NPARAM + 255) / 256), dim3(256), 0, st, tmp, acc, (int)(r0 == 0), (int)(r0 + slab >= n),
                           (double)n, fisher);
    }
    return (int)hipGetLastError();
}

}  // namespace tmcts_vf

extern "C" {

long long tm_valuenet_fit_fisher_workspace(int slab) {
    if (slab < 1 || slab > tmcts_vf::MAX_BATCH) return -1;
    return tmcts_vf::layout(slab).total + tmcts_vf::FISHER_TMP + tmcts_vf::FISHER_ACC;
}

int tm_valuenet_fit_fisher(const float* params, const float* out_bounds, const int8_t* states, const float* value,
                           const float* variance, const float* weight, const int64_t* idx, long long n, int slab, int weighted,
                           float variance_clip, float* fisher, float* workspace, void* stream) {
    return tmcts_vf::fit_fisher<tmcts_fit::DenseStates>(params, out_bounds, states, value, variance, weight, idx, n, slab, weighted,
                                                        variance_clip, fisher, workspace, stream);
}

int tm_valuenet_fit_fisher_packed(const float* params, const float* out_bounds, const uint32_t* obs, const float* value,
                                  const float* variance, const float* weight, const int64_t* idx, long long n, int slab, int weighted,
                                  float variance_clip, float* fisher, float* workspace, void* stream) {
    if ((uintptr_t)obs & 3) return (int)hipErrorInvalidValue;
    return tmcts_vf::fit_fisher<tmcts_fit::PackedStates>(params, out_bounds, obs, value, variance, weight, idx, n, slab, weighted,
                                                         variance_clip, fisher, workspace, stream);
}

long long tm_valuenet_fit_workspace(int batch) {
    if (batch < 1 || batch > tmcts_vf::MAX_BATCH) return -1;
    return tmcts_vf::layout(batch).total;
}

int tm_valuenet_fit_grad(const float* params, const float* out_bounds, const int8_t* states, const float* value,
                         const float* variance, const float* weight, const int64_t* idx, int batch, int weighted,
                         float variance_clip, float* grad, float* loss, float* workspace, void* stream) {
    return tmcts_vf::fit_grad<tmcts_fit::DenseStates>(params, out_bounds, states, value, variance, weight, idx, batch, weighted,
                                                      variance_clip, grad, loss, workspace, stream);
}

int tm_valuenet_fit_grad_packed(const float* params, const float* out_bounds, const uint32_t* obs, const float* value,
                                const float* variance, const float* weight, const int64_t* idx, int batch, int weighted,
                                float variance_clip, float* grad, float* loss, float* workspace, void* stream) {
    if ((uintptr_t)obs & 3) return (int)hipErrorInvalidValue;
    return tmcts_vf::fit_grad<tmcts_fit::PackedStates>(params, out_bounds, obs, value, variance, weight, idx, batch, weighted,
                                                       variance_clip, grad, loss, workspace, stream);
}

long long tm_valuenet_fit_validate_workspace(int slab) {
    if (slab < 1 || slab > tmcts_vf::MAX_BATCH) return -1;
    return tmcts_vf::val_layout(slab).total;
}

int tm_valuenet_fit_validate(const float* params, const float* out_bounds, const int8_t* states, const float* value,
                             const float* variance, const float* weight, long long n, int chunk, int slab, int weighted,
                             float variance_clip, double* rows_out, float* workspace, void* stream) {
    return tmcts_vf::fit_validate<tmcts_fit::DenseStates>(params, out_bounds, states, value, variance, weight, n, chunk, slab,
                                                          weighted, variance_clip, rows_out, workspace, stream);
}

int tm_valuenet_fit_validate_packed(const float* params, const float* out_bounds, const uint32_t* obs, const float* value,
                                    const float* variance, const float* weight, long long n, int chunk, int slab, int weighted,
                                    float variance_clip, double* rows_out, float* workspace, void* stream) {
    if ((uintptr_t)obs & 3) return (int)hipErrorInvalidValue;
    return tmcts_vf::fit_validate<tmcts_fit::PackedStates>(params, out_bounds, obs, value, variance, weight, n, chunk, slab,
                                                           weighted, variance_clip, rows_out, workspace, stream);
}

}  // extern "C"
