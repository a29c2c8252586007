// Gradient step of the distributional head's online fit for gfx950: forward, loss and backward of model_distributional.Net +
// Model_Dist.loss in one C call (tm_distnet_fit_grad), on the fp32 matrix cores.  DESIGN.md section 3.9 has the contract and
// the measurements; csrc/valuenet_fit.hip is the value net's counterpart and csrc/fit_mma.h what the two share.
//
// The net: conv 4x4 (1 -> 32) on 22 x 10 -> 19 x 7 = 133 positions, LeakyReLU(0.01), conv 4x4 (32 -> 32) -> 16 x 4 = 64 positions,
// LeakyReLU, FC 2048 -> 128, LeakyReLU, FC 128 -> atoms, log-softmax.  The states hold the 20 visible rows; the two empty rows on
// top are supplied by the index arithmetic of the kernels that read them.
//
// Every layer, forward and backward, is a matrix product on v_mfma_f32_32x32x2_f32 laid out as in valuenet_fit.hip: a wave owns
// NT tiles of 32 x 32 that share their A operand, K is walked in quads (a lane of half h takes k = 8 q + 4 h + r) and summed in
// chunks of four quads (32 terms) that start from zero, the chunk sums added on the vector ALU (fc1's 64 chunks with an
// error-free TwoSum).  The output layer (atoms x 128, 0.4 % of the arithmetic), the softmax, the per-sample loss and the logit
// gradient are one wave per sample in double (k_df_head), as the value net's k_vf_head.
//
// conv1's activations and their gradients are stored with a channel stride of 136 (133 positions and three of padding), so that
// a quad of K along the positions is one aligned 16-byte load; the padding of the gradient is written as zero and the padding of
// the activations is never read.
//
// LeakyReLU: the forward stores a = z > 0 ? z : 0.01f z; the backward passes 1 where the stored a > 0 and 0.01 elsewhere (torch's
// rule at 0).  Gradients are kept with respect to the pre-activations.
//
// Determinism: every output element, and every partial sum, is produced by one wave in one fixed order; batch reductions are
// partial sums in the workspace and a second stage that adds them in a fixed order.  There are no atomics.  All launch shapes
// follow from `batch` and `atoms` alone.
//
// The validation pass (tm_distnet_fit_validate) is the same forward (forward(): the same kernels and instantiations, idx NULL) over
// the held-out rows, a slab at a time, k_df_head<false> for the per-sample losses and k_fit_val_moments<1> for each chunk's
// {w, mean, n - 1 std}: what a row's loss is, and the order in which losses are added, are the gradient step's.
//
// The states come as int8 [rows][200] or as packed observations, uint32 [rows][12] (tm_distnet_fit_grad_packed,
// tm_distnet_fit_validate_packed), through the template argument SRC of conv1's two kernels, as in valuenet_fit.hip.
//
// The Fisher pass (tm_distnet_fit_fisher) is the diagonal of the empirical Fisher matrix over n rows: the
// gradient step's forward and data gradients with the divisor 1, the SQ forms of the weight-gradient kernels and a double
// accumulator across slabs (fit_fisher below).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/tetris_mcts_hip.h"
#include "fit_mma.h"

namespace tmcts_df {
using namespace tmcts_fit;

constexpr int P1 = 133, S1 = 136, P2 = 64, A1 = 32 * S1, A2 = 32 * P2, HID = 128, ROW = 64;
constexpr int OFF_C1W = 0, OFF_C1B = 512, OFF_C2W = 544, OFF_C2B = 16928, OFF_F1W = 16960, OFF_F1B = 279104, OFF_FVW = 279232;
static_assert(OFF_FVW + 50 * HID + 50 == TM_DISTNET_PARAMS_50, "parameter blob size at 50 atoms");
constexpr int MAX_BATCH = 1 << 20;      // N = B * 136 positions stay inside an int (element offsets are size_t)
constexpr int SPW = 4;                  // samples per wave of the convolutions' weight-gradient partials
constexpr int FC_KC = 256;              // samples per split of the two FC weight gradients
constexpr int HEAD_CHUNK = 32;          // samples per partial of the bias sums of fc1 and fc_v
constexpr int HEAD_PART = HID + ROW;    // floats of such a partial: db_fc1[128], db_v[64]

// The workspace, in floats (every segment starts at a multiple of four: 16-byte loads).
struct Layout {
    long long a1, dz1, a2, dz2, h, dh, dzv, per, pf1, pfv, pw2, pw1, cb, hp, total;
    int s1, chunks, hchunks;
};
__host__ inline Layout layout(int B) {
    Layout L;
    long long o = 0, b = B;
    L.s1 = (B + FC_KC - 1) / FC_KC;
    L.chunks = (B + SPW - 1) / SPW;
    L.hchunks = (B + HEAD_CHUNK - 1) / HEAD_CHUNK;
    L.a1 = o; o += b * A1;
    L.dz1 = o; o += b * A1;
    L.a2 = o; o += b * A2;
    L.dz2 = o; o += b * A2;
    L.h = o; o += b * HID;
    L.dh = o; o += b * HID;
    L.dzv = o; o += b * ROW;
    L.per = o; o += up4(b * 2);                       // doubles
    L.pf1 = o; o += (long long)L.s1 * HID * A2;
    L.pfv = o; o += (long long)L.s1 * ROW * HID;
    L.pw2 = o; o += (long long)L.chunks * 16384;
    L.pw1 = o; o += (long long)L.chunks * 512;
    L.cb = o; o += b * 64;
    L.hp = o; o += (long long)L.hchunks * HEAD_PART;
    L.total = o;
    return L;
}

// ---- forward convolution 4 x 4: z[co][b, p] = bias[co] + sum_k W[co][k] in[b][ci][(y + ky) IW + x + kx], LeakyReLU ----
// M = 32 output channels, N = B * OP positions, K = CIN * 16.  CIN == 1: the input is the state of row idx[b] under two empty
// rows, read through SRC (fit_mma.h: int8 cells or a packed observation); a lane's two quads are the board rows ny + half - 2 and
// ny + half, one strip that it keeps per tile.  ISTR / OSTR: the channel strides of the input and the output.
template <int CIN, int IH, int IW, int ISTR, int OSTR, int NT, typename SRC = DenseStates>
__global__ __launch_bounds__(256) void k_df_conv_fwd(const float* __restrict__ W, const float* __restrict__ bias,
                                                     const float* __restrict__ in, const typename SRC::elem* __restrict__ states,
                                                     const int64_t* __restrict__ idx, int B, float* __restrict__ out) {
    constexpr int OW = IW - 3, OP = (IH - 3) * OW, K = CIN * 16, KQ = K / 8;
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NT * 32, N = B * OP;
    if (n0 >= N) return;
    bool ok[NT];
    int nb[NT], np[NT], ny[NT], nx[NT];
    size_t base[NT];
    typename SRC::Strip cells[NT];
    static_assert(CIN != 1 || K == 16, "CIN == 1: two quads, the rows ny + half - 2 and ny + half of one strip");
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = n0 + 32 * t + l31;
        ok[t] = n < N;
        const int nn = ok[t] ? n : 0, b = nn / OP, p = nn - b * OP;
        nb[t] = b;
        np[t] = p;
        ny[t] = p / OW;
        nx[t] = p - ny[t] * OW;
        base[t] = (size_t)b * (CIN * ISTR) + ny[t] * IW + nx[t];
        if constexpr (CIN == 1) cells[t] = SRC::strip(SRC::row(states, row_of(idx, b)), ny[t] + half - 2);
    }
    f32x16 tot[NT], acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[t][r] = bias[drow(r, half)];
    const float* arow = W + l31 * K + 4 * half;
#pragma unroll 1
    for (int qc = 0; qc < KQ; qc += CHUNK_QUADS) {
        vf_zero<NT>(acc);
#pragma unroll
        for (int q = qc; q < (qc + CHUNK_QUADS < KQ ? qc + CHUNK_QUADS : KQ); ++q) {
            const int k0 = 8 * q + 4 * half, ci = k0 >> 4, ky = (k0 & 15) >> 2;      // the quad's four taps: kx = 0..3 of one row
            const float4 a = *reinterpret_cast<const float4*>(arow + 8 * q);
            float4 b4[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (CIN == 1) {
                    const int yy = ny[t] + ky - 2;      // row of the 20 visible ones; the two above them are empty
                    if (ok[t] && yy >= 0) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = SRC::cell(cells[t], yy, nx[t] + r);
                    }
                } else if (ok[t]) {
                    const float* s = in + base[t] + ci * ISTR + ky * IW;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = s[r];
                }
                b4[t] = make_float4(v[0], v[1], v[2], v[3]);
            }
            vf_quad<NT>(acc, a, b4);
        }
        vf_add<NT>(tot, acc);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (ok[t]) {
            float* dst = out + (size_t)nb[t] * (32 * OSTR) + np[t];
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[drow(r, half) * OSTR] = Leaky::fwd(tot[t][r]);
        }
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

// ---- output layer, log-softmax, loss and their gradients: one wave per sample, lane a = atom a, in double ----
// per = w sum_a (t log t - t log p); dzv[b][a] = (w / div) (p_a sum_a t - t_a) (zero for a >= atoms), div = B in the gradient
// step (the mean's gradient) and 1 in the Fisher pass (per-sample gradients);
// dh[b][i] = (sum_a dzv[a] Wv[a][i]) times 1 where h > 0, 0.01 elsewhere.
// GRAD = false (the validation pass): per alone, by the same statements; dzv and dh are not touched.
template <bool GRAD>
__global__ __launch_bounds__(256) void k_df_head(const float* __restrict__ Wv, const float* __restrict__ bv,
                                                 const float* __restrict__ h, const float* __restrict__ target, int tstride,
                                                 const float* __restrict__ weight, const int64_t* __restrict__ idx, int B,
                                                 int atoms, int weighted, double div, float* __restrict__ dzv,
                                                 double* __restrict__ per, float* __restrict__ dh) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bool on = lane < atoms;
    const float* hb = h + (size_t)b * HID;
    const float* wr = Wv + (on ? lane : 0) * HID;
    double z = 0.0;
#pragma unroll 4
    for (int i = 0; i < HID; i += 4) {
        const float4 hv = *reinterpret_cast<const float4*>(hb + i);
        const float4 wv = *reinterpret_cast<const float4*>(wr + i);
        z += (double)hv.x * (double)wv.x;
        z += (double)hv.y * (double)wv.y;
        z += (double)hv.z * (double)wv.z;
        z += (double)hv.w * (double)wv.w;
    }
    z += (double)bv[on ? lane : 0];
    const double zmax = wave_max(on ? z : -INFINITY);
    const double e = on ? exp(z - zmax) : 0.0, S = wave_sum(e);
    const double logp = z - zmax - log(S), p = e / S;
    const size_t row = row_of(idx, b);
    const double t = on ? (double)target[row * (size_t)tstride + lane] : 0.0, T = wave_sum(t);
    const double w = weighted ? (double)weight[row] : 1.0;
    const double term = t > 0.0 ? t * log(t) - t * logp : 0.0;
    const double loss = w * wave_sum(term);
    if (lane == 0) per[b] = loss;
    if (!GRAD) return;
    const double dz = on ? (w / div) * (p * T - t) : 0.0;
    dzv[(size_t)b * ROW + lane] = (float)dz;
    double g0 = 0.0, g1 = 0.0;
    for (int a = 0; a < atoms; ++a) {
        const double da = __shfl(dz, a, 64);
        g0 += da * (double)Wv[a * HID + lane];
        g1 += da * (double)Wv[a * HID + 64 + lane];
    }
    const float h0 = hb[lane], h1 = hb[64 + lane];
    dh[(size_t)b * HID + lane] = (float)(h0 > 0.0f ? g0 : 0.01 * g0);
    dh[(size_t)b * HID + 64 + lane] = (float)(h1 > 0.0f ? g1 : 0.01 * g1);
}

// partial sums over HEAD_CHUNK samples of db_fc1 = sum dh and db_v = sum dzv; SQ (the Fisher pass): of dh^2 and dzv^2
template <bool SQ>
__global__ __launch_bounds__(192) void k_df_head_part(const float* __restrict__ dzv, const float* __restrict__ dh, int B,
                                                      float* __restrict__ part) {
    const int i = threadIdx.x, b0 = blockIdx.x * HEAD_CHUNK, b1 = min(B, b0 + HEAD_CHUNK);
    float s = 0.f;
    for (int b = b0; b < b1; ++b) {
        const float v = i < HID ? dh[(size_t)b * HID + i] : dzv[(size_t)b * ROW + (i - HID)];
        s += SQ ? v * v : v;
    }
    part[(size_t)blockIdx.x * HEAD_PART + i] = s;
}

// ---- FC weight gradient: part[s][m][n] = sum over the samples of split s of dA[b][m] act[b][n]; M = MS, N = NS, K = samples.
// fc1: dA = dh (MS = 128), act = a2 (NS = 2048); fc_v: dA = dzv (MS = 64, zero beyond the atoms), act = h (NS = 128) ----
// (chunks of 32 samples here and ONE chain a split in valuenet_fit.hip's k_vf_fc1_dw: one kernel for both would change that one's bits)
// SQ (the Fisher pass): both operands are squared as they are loaded - the sum over the samples of the squared outer products
// (dA[b][m] act[b][n])^2 is the matrix product of the squared operands.
template <int MS, int NS, int NT, bool SQ = false>
__global__ __launch_bounds__(256) void k_df_fc_dw(const float* __restrict__ dA, const float* __restrict__ act, int B,
                                                  float* __restrict__ part) {
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    constexpr int NG = NS / 32 / NT, MT = MS / 32;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), ng = wave % NG, mt = (wave / NG) % MT, s = wave / (NG * MT);
    const int b0 = s * FC_KC, b1 = min(B, b0 + FC_KC);
    if (b0 >= B) return;
    f32x16 tot[NT], acc[NT];
    vf_zero<NT>(tot);
    const float* acol = dA + 32 * mt + l31;
    const float* bcol = act + ng * NT * 32 + l31;
#pragma unroll 1
    for (int bc = b0; bc < b1; bc += 8 * CHUNK_QUADS) {
        vf_zero<NT>(acc);
#pragma unroll
        for (int qq = 0; qq < CHUNK_QUADS; ++qq) {
            const int bq = bc + 8 * qq;
            float av[4];
            float bv[NT][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = bq + 4 * half + r;
                const bool in = b < b1;
                const size_t bb = in ? b : b0;
                av[r] = in ? acol[bb * MS] : 0.0f;
#pragma unroll
                for (int t = 0; t < NT; ++t) bv[t][r] = in ? bcol[bb * NS + 32 * t] : 0.0f;
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
        vf_add<NT>(tot, acc);
    }
    float* dst = part + (size_t)s * (MS * NS) + (size_t)(32 * mt) * NS + ng * NT * 32 + l31;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(size_t)drow(r, half) * NS + 32 * t] = tot[t][r];
}

// ---- conv2's transposed convolution: dz1[b][ci][u] = (sum_{co,ky,kx} dz2[b][co][(uy - ky, ux - kx)] W2[co][ci][ky][kx]) times
// the slope of a1[b][ci][u]; dz2 counts as zero outside its 16 x 4.  M = 32 input channels, N = B * 136 (the three positions
// of padding per sample are written as zero), K = 512 ----
template <int NT>
__global__ __launch_bounds__(256) void k_df_conv_bwd_data(const float* __restrict__ W, const float* __restrict__ dzo,
                                                          const float* __restrict__ ain, int B, float* __restrict__ dzi) {
    constexpr int OH = 16, OW = 4, IW = 7;
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NT * 32, N = B * S1;
    if (n0 >= N) return;
    bool ok[NT], real[NT];
    int uy[NT], ux[NT];
    size_t ob[NT], ib[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = n0 + 32 * t + l31;
        ok[t] = n < N;
        const int nn = ok[t] ? n : 0, b = nn / S1, u = nn - b * S1;
        real[t] = ok[t] && u < P1;
        uy[t] = u / IW;
        ux[t] = u - uy[t] * IW;
        ob[t] = (size_t)b * A2;
        ib[t] = (size_t)b * A1 + u;
    }
    f32x16 tot[NT], acc[NT];
    vf_zero<NT>(tot);
    const float* arow = W + l31 * 16 + 4 * half;
#pragma unroll 1
    for (int qc = 0; qc < 64; qc += CHUNK_QUADS) {
        vf_zero<NT>(acc);
#pragma unroll
        for (int q = qc; q < qc + CHUNK_QUADS; ++q) {
            const int k0 = 8 * q + 4 * half, co = k0 >> 4, ky = (k0 & 15) >> 2;      // the quad's four taps: kx = 0..3
            const float4 a = *reinterpret_cast<const float4*>(arow + (size_t)co * 512 + (8 * q & 15));
            float4 b4[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                const int oy = uy[t] - ky;
                if (real[t] && oy >= 0 && oy < OH) {
                    const float* s = dzo + ob[t] + co * P2 + oy * OW;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ox = ux[t] - r;
                        if (ox >= 0 && ox < OW) v[r] = s[ox];
                    }
                }
                b4[t] = make_float4(v[0], v[1], v[2], v[3]);
            }
            vf_quad<NT>(acc, a, b4);
        }
        vf_add<NT>(tot, acc);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (ok[t]) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const size_t o = ib[t] + (size_t)drow(r, half) * S1;
                dzi[o] = real[t] ? Leaky::bwd(ain[o], tot[t][r]) : 0.0f;
            }
        }
}

// ---- convolution weight gradient: part[chunk][co][n = (ci,ky,kx)] = sum over the chunk's SPW samples and the OP positions of
// dzo[b][co][p] in[b][ci][(y + ky) IW + x + kx].  M = 32, N = CIN * 16 (NT tiles per wave), K = (sample, position); the
// gradient's channel stride OSTR is a multiple of 8 and holds zeros beyond OP ----
// CIN == 1: ain is the state of row idx[b] under two empty rows, read through SRC.  A lane's tap is fixed and the loop walks the
// positions, so the strip is built per quad of positions (four positions lie in two rows at most) from the row the lane keeps
// per sample.
// SQ (the Fisher pass): tot starts every sample from zero and holds that sample's gradient after its positions; its square is
// added to a second set of accumulators, which is what is stored, so a partial is the sum over its samples of the squared
// per-sample gradients.
template <int CIN, int IW, int ISTR, int OW, int OP, int OSTR, int NT, typename SRC = DenseStates, bool SQ = false>
__global__ __launch_bounds__(256) void k_df_conv_dw(const float* __restrict__ dzo, const float* __restrict__ ain,
                                                    const typename SRC::elem* __restrict__ states,
                                                    const int64_t* __restrict__ idx, int B, float* __restrict__ part) {
    constexpr int KW = CIN * 16, NG = (KW + 32 * NT - 1) / (32 * NT), KQ = OSTR / 8;
    static_assert(OSTR % 8 == 0, "a quad of K stays inside one sample");
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), ng = wave % NG, chunk = wave / NG;
    const int b0 = chunk * SPW, b1 = min(B, b0 + SPW);
    if (b0 >= B) return;
    bool nok[NT];
    int nci[NT], nky[NT], nkx[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = (ng * NT + t) * 32 + l31;
        nok[t] = n < KW;
        const int nn = nok[t] ? n : 0;
        nci[t] = nn >> 4;
        nky[t] = (nn & 15) >> 2;
        nkx[t] = nn & 3;
    }
    f32x16 tot[NT], acc[NT];
    [[maybe_unused]] f32x16 sq[SQ ? NT : 1];
    vf_zero<NT>(tot);
    if constexpr (SQ) vf_zero<NT>(sq);
    for (int b = b0; b < b1; ++b) {
        const float* arow = dzo + (size_t)b * (32 * OSTR) + l31 * OSTR + 4 * half;
        const size_t ibase = (size_t)b * (CIN * ISTR);
        typename SRC::Row srow;
        if constexpr (CIN == 1) srow = SRC::row(states, row_of(idx, b));
#pragma unroll 1
        for (int qc = 0; qc < KQ; qc += CHUNK_QUADS) {
            vf_zero<NT>(acc);
#pragma unroll
            for (int qq = 0; qq < CHUNK_QUADS; ++qq) {
                const int q = qc + qq;
                if (q < KQ) {
                    const float4 a = *reinterpret_cast<const float4*>(arow + 8 * q);
                    float bv[NT][4];
                    typename SRC::Strip cells[NT];
                    if constexpr (CIN == 1) {
                        static_assert(CIN != 1 || OW >= 4, "a quad of positions lies in two rows at most");
#pragma unroll
                        for (int t = 0; t < NT; ++t) cells[t] = SRC::strip(srow, (8 * q + 4 * half) / OW + nky[t] - 2);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int p = 8 * q + 4 * half + r, y = p / OW, x = p - y * OW;
                        const bool pin = OSTR == OP || p < OP;
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            float v = 0.0f;
                            if (nok[t] && pin) {
                                if (CIN == 1) {
                                    const int yy = y + nky[t] - 2;      // row of the 20 visible ones
                                    if (yy >= 0) v = SRC::cell(cells[t], yy, x + nkx[t]);
                                } else {
                                    v = ain[ibase + nci[t] * ISTR + (y + nky[t]) * IW + x + nkx[t]];
                                }
                            }
                            bv[t][r] = v;
                        }
                    }
                    float4 b4[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) b4[t] = make_float4(bv[t][0], bv[t][1], bv[t][2], bv[t][3]);
                    vf_quad<NT>(acc, a, b4);
                }
            }
            vf_add<NT>(tot, acc);
        }
        if constexpr (SQ) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    sq[t][r] += tot[t][r] * tot[t][r];
                    tot[t][r] = 0.0f;
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
                else dst[drow(r, half) * KW + n] = tot[t][r];
            }
        }
}

// per sample, the sums over positions of dz1 / dz2 per channel: cb[b][64] (conv1, conv2); dz1's padding holds zeros; SQ (the
// Fisher pass): their squares
template <bool SQ>
__global__ __launch_bounds__(64) void k_df_conv_bias_part(const float* __restrict__ dz1, const float* __restrict__ dz2, int B,
                                                          float* __restrict__ cb) {
    const int b = blockIdx.x, i = threadIdx.x;
    if (b >= B) return;
    const int c = i & 31, op = i < 32 ? S1 : P2;
    const float* src = i < 32 ? dz1 + (size_t)b * A1 + c * S1 : dz2 + (size_t)b * A2 + c * P2;
    float s = 0.0f;
    for (int p = 0; p < op; p += 4) {
        const float4 v = *reinterpret_cast<const float4*>(src + p);
        s += (v.x + v.y) + (v.z + v.w);
    }
    cb[(size_t)b * 64 + i] = SQ ? s * s : s;
}

// the forward of B rows (states: SRC's rows, int8 [.][200] or packed [.][12]; row idx[b], or row b when idx is NULL) into a1, a2,
// h: the launches of the gradient step and of the validation pass
template <typename SRC>
static void forward(const float* P, const typename SRC::elem* states, const int64_t* idx, int B, float* a1, float* a2, float* h,
                    hipStream_t st) {
    hipLaunchKernelGGL((k_df_conv_fwd<1, 22, 10, 0, S1, 3, SRC>), dim3(blocks_for_waves((tiles((long long)B * P1) + 2) / 3)), dim3(256), 0, st,
                       P + OFF_C1W, P + OFF_C1B, (const float*)nullptr, states, idx, B, a1);
    hipLaunchKernelGGL((k_df_conv_fwd<32, 19, 7, S1, P2, 2>), dim3(blocks_for_waves((tiles((long long)B * P2) + 1) / 2)), dim3(256), 0, st,
                       P + OFF_C2W, P + OFF_C2B, a1, (const int8_t*)nullptr, (const int64_t*)nullptr, B, a2);
    hipLaunchKernelGGL((k_fit_fc1_fwd<HID, A2, Leaky, 1>), dim3(blocks_for_waves(4 * tiles(B))), dim3(256), 0, st, P + OFF_F1W, P + OFF_F1B, a2, B, h);
}

// the validation pass's workspace, in floats: the forward's activations of one slab and its per-row losses (doubles)
struct ValLayout {
    long long a1, a2, h, per, total;
};
__host__ inline ValLayout val_layout(int slab) {
    ValLayout L;
    long long o = 0, b = slab;
    L.a1 = o; o += b * A1;
    L.a2 = o; o += b * A2;
    L.h = o; o += b * HID;
    L.per = o; o += up4(b * 2);
    L.total = o;
    return L;
}

// the gradient step on either kind of rows: tm_distnet_fit_grad (DenseStates) and tm_distnet_fit_grad_packed (PackedStates)
template <typename SRC>
static int fit_grad(const float* params, const typename SRC::elem* states, const float* target, int target_stride,
                    const float* weight, const int64_t* idx, int batch, int atoms, int weighted, float* grad, float* loss,
                    float* workspace, void* stream_) {
    if (!params || !states || !target || !weight || !grad || !loss || !workspace) return (int)hipErrorInvalidValue;
    if (batch < 1 || batch > MAX_BATCH || atoms < 1 || atoms > ROW || target_stride < atoms) return (int)hipErrorInvalidValue;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)params & 15)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream_;
    const int B = batch;
    const Layout L = layout(B);
    float* ws = workspace;
    float *a1 = ws + L.a1, *dz1 = ws + L.dz1, *a2 = ws + L.a2, *dz2 = ws + L.dz2, *h = ws + L.h, *dh = ws + L.dh, *dzv = ws + L.dzv;
    float *pf1 = ws + L.pf1, *pfv = ws + L.pfv, *pw2 = ws + L.pw2, *pw1 = ws + L.pw1, *cb = ws + L.cb, *hp = ws + L.hp;
    double* per = reinterpret_cast<double*>(ws + L.per);
    const float* P = params;
    const int OFF_FVB = OFF_FVW + atoms * HID;
    // ---- forward ----
    forward<SRC>(P, states, idx, B, a1, a2, h, st);
    // ---- output layer, loss, and the bias sums of the two FC layers ----
    hipLaunchKernelGGL(k_df_head<true>, dim3((B + 3) / 4), dim3(256), 0, st, P + OFF_FVW, P + OFF_FVB, h, target, target_stride, weight, idx,
                       B, atoms, weighted, (double)B, dzv, per, dh);
    hipLaunchKernelGGL(k_fit_loss<1>, dim3(1), dim3(256), 0, st, per, B, loss);
    hipLaunchKernelGGL(k_df_head_part<false>, dim3(L.hchunks), dim3(HEAD_PART), 0, st, dzv, dh, B, hp);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(HID / 16), dim3(256), 0, st, hp, L.hchunks, (long long)HEAD_PART, HID, grad + OFF_F1B);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3((atoms + 15) / 16), dim3(256), 0, st, hp + HID, L.hchunks, (long long)HEAD_PART, atoms,
                       grad + OFF_FVB);
    // ---- the FC layers backward ----
    hipLaunchKernelGGL((k_df_fc_dw<ROW, HID, 2>), dim3(blocks_for_waves((long long)L.s1 * 2 * 2)), dim3(256), 0, st, dzv, h, B, pfv);
    hipLaunchKernelGGL((k_fit_reduce<4>), dim3((atoms * HID + 63) / 64), dim3(256), 0, st, pfv, L.s1, (long long)ROW * HID, atoms * HID,
                       grad + OFF_FVW);
    hipLaunchKernelGGL((k_df_fc_dw<HID, A2, 2>), dim3(blocks_for_waves((long long)L.s1 * 4 * 32)), dim3(256), 0, st, dh, a2, B, pf1);
    hipLaunchKernelGGL((k_fit_reduce<4>), dim3(HID * A2 / 64), dim3(256), 0, st, pf1, L.s1, (long long)HID * A2, HID * A2, grad + OFF_F1W);
    hipLaunchKernelGGL((k_fit_fc1_bwd_data<HID, A2, Leaky, 2>), dim3(blocks_for_waves(tiles(B) * 32)), dim3(256), 0, st, P + OFF_F1W, dh, a2, B, dz2);
    // ---- convolutions backward ----
    hipLaunchKernelGGL((k_df_conv_dw<32, 7, S1, 4, P2, P2, 4>), dim3(blocks_for_waves((long long)L.chunks * 4)), dim3(256), 0, st, dz2, a1,
                       (const int8_t*)nullptr, (const int64_t*)nullptr, B, pw2);
    hipLaunchKernelGGL((k_df_conv_bwd_data<2>), dim3(blocks_for_waves((tiles((long long)B * S1) + 1) / 2)), dim3(256), 0, st, P + OFF_C2W,
                       dz2, a1, B, dz1);
    hipLaunchKernelGGL((k_df_conv_dw<1, 10, 0, 7, P1, S1, 1, SRC>), dim3(blocks_for_waves(L.chunks)), dim3(256), 0, st, dz1,
                       (const float*)nullptr, states, idx, B, pw1);
    hipLaunchKernelGGL(k_df_conv_bias_part<false>, dim3(B), dim3(64), 0, st, dz1, dz2, B, cb);
    // ---- second stages of the convolutions' sums ----
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(16384 / 16), dim3(256), 0, st, pw2, L.chunks, 16384LL, 16384, grad + OFF_C2W);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(512 / 16), dim3(256), 0, st, pw1, L.chunks, 512LL, 512, grad + OFF_C1W);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(2), dim3(256), 0, st, cb, B, 64LL, 32, grad + OFF_C1B);
    hipLaunchKernelGGL((k_fit_reduce<16>), dim3(2), dim3(256), 0, st, cb + 32, B, 64LL, 32, grad + OFF_C2B);
    return (int)hipGetLastError();
}

// the validation pass on either kind of rows
template <typename SRC>
static int fit_validate(const float* params, const typename SRC::elem* states, const float* target, int target_stride,
                        const float* weight, long long n, int chunk, int slab, int atoms, int weighted, double* rows_out,
                        float* workspace, void* stream_) {
    if (!params || !states || !target || !weight || !rows_out || !workspace) return (int)hipErrorInvalidValue;
    if (n < 1 || chunk < 1 || slab < chunk || slab > MAX_BATCH || slab % chunk) return (int)hipErrorInvalidValue;
    if (atoms < 1 || atoms > ROW || target_stride < atoms) return (int)hipErrorInvalidValue;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)params & 15) || ((uintptr_t)rows_out & 7)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream_;
    const ValLayout L = val_layout(slab);
    float *a1 = workspace + L.a1, *a2 = workspace + L.a2, *h = workspace + L.h;
    double* per = reinterpret_cast<double*>(workspace + L.per);
    const int OFF_FVB = OFF_FVW + atoms * HID;
    // slab by slab on the one stream: a slab's kernels have read the workspace before the next slab's overwrite it
    for (long long r0 = 0; r0 < n; r0 += slab) {
        const int B = (int)(n - r0 < slab ? n - r0 : slab);
        forward<SRC>(params, states + r0 * SRC::STRIDE, (const int64_t*)nullptr, B, a1, a2, h, st);
        hipLaunchKernelGGL(k_df_head<false>, dim3((B + 3) / 4), dim3(256), 0, st, params + OFF_FVW, params + OFF_FVB, h,
                           target + r0 * target_stride, target_stride, weight + r0, (const int64_t*)nullptr, B, atoms, weighted,
                           1.0, (float*)nullptr, per, (float*)nullptr);
        hipLaunchKernelGGL(k_fit_val_moments<1>, dim3((B + chunk - 1) / chunk), dim3(256), 0, st, per, weight + r0, B, chunk, weighted,
                           rows_out + 3 * (r0 / chunk));
    }
    return (int)hipGetLastError();
}

// ---- the Fisher pass: F[i] = (1/n) sum_b (d loss_b / d p_i)^2 over n rows, a slab at a time ----
// A slab is the gradient step's forward, k_df_head with the divisor 1 (dzv and dh are then PER-SAMPLE gradients) and its data
// gradients as they are, and the SQ forms of the weight-gradient kernels, whose partials hold sums over samples of squared
// per-sample gradients; the unchanged second stages add them into a temporary [P], which k_df_fisher_add adds to a double
// accumulator, slab after slab in stream order.  The workspace is the gradient step's of `slab` rows, then the temporary, then
// the accumulator.
__host__ inline int nparam(int atoms) { return OFF_FVW + atoms * HID + atoms; }

// acc[i] = (first ? 0 : acc[i]) + tmp[i]; after the last slab fisher[i] = (float)(acc[i] / n)
__global__ __launch_bounds__(256) void k_df_fisher_add(const float* __restrict__ tmp, double* __restrict__ acc, int np, int first,
                                                       int last, double n, float* __restrict__ fisher) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const double a = (first ? 0.0 : acc[i]) + (double)tmp[i];
    acc[i] = a;
    if (last) fisher[i] = (float)(a / n);
}

template <typename SRC>
static int fit_fisher(const float* params, const typename SRC::elem* states, const float* target, int target_stride,
                      const float* weight, const int64_t* idx, long long n, int slab, int atoms, int weighted, float* fisher,
                      float* workspace, void* stream_) {
    if (!params || !states || !target || !weight || !fisher || !workspace) return (int)hipErrorInvalidValue;
    if (n < 1 || slab < 1 || slab > MAX_BATCH || atoms < 1 || atoms > ROW || target_stride < atoms) return (int)hipErrorInvalidValue;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)params & 15)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream_;
    const Layout L = layout(slab);
    const int NP = nparam(atoms), OFF_FVB = OFF_FVW + atoms * HID;
    float* ws = workspace;
    float *a1 = ws + L.a1, *dz1 = ws + L.dz1, *a2 = ws + L.a2, *dz2 = ws + L.dz2, *h = ws + L.h, *dh = ws + L.dh, *dzv = ws + L.dzv;
    float *pf1 = ws + L.pf1, *pfv = ws + L.pfv, *pw2 = ws + L.pw2, *pw1 = ws + L.pw1, *cb = ws + L.cb, *hp = ws + L.hp;
    float* tmp = ws + L.total;
    double *per = reinterpret_cast<double*>(ws + L.per), *acc = reinterpret_cast<double*>(ws + L.total + up4(NP));
    const float* P = params;
    // slab by slab on the one stream: a slab's kernels have read the workspace before the next slab's overwrite it
    for (long long r0 = 0; r0 < n; r0 += slab) {
        const int B = (int)(n - r0 < slab ? n - r0 : slab);
        const int s1 = (B + FC_KC - 1) / FC_KC, chunks = (B + SPW - 1) / SPW, hchunks = (B + HEAD_CHUNK - 1) / HEAD_CHUNK;
        // rows idx[r0 + b]; without idx the rows r0 + b
        const int64_t* ix = idx ? idx + r0 : nullptr;
        const long long base = idx ? 0 : r0;
        const typename SRC::elem* S = states + base * SRC::STRIDE;
        forward<SRC>(P, S, ix, B, a1, a2, h, st);
        hipLaunchKernelGGL(k_df_head<true>, dim3((B + 3) / 4), dim3(256), 0, st, P + OFF_FVW, P + OFF_FVB, h, target + base * target_stride,
                           target_stride, weight + base, ix, B, atoms, weighted, 1.0, dzv, per, dh);
        hipLaunchKernelGGL(k_df_head_part<true>, dim3(hchunks), dim3(HEAD_PART), 0, st, dzv, dh, B, hp);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(HID / 16), dim3(256), 0, st, hp, hchunks, (long long)HEAD_PART, HID, tmp + OFF_F1B);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3((atoms + 15) / 16), dim3(256), 0, st, hp + HID, hchunks, (long long)HEAD_PART, atoms,
                           tmp + OFF_FVB);
        hipLaunchKernelGGL((k_df_fc_dw<ROW, HID, 2, true>), dim3(blocks_for_waves((long long)s1 * 2 * 2)), dim3(256), 0, st, dzv, h, B, pfv);
        hipLaunchKernelGGL((k_fit_reduce<4>), dim3((atoms * HID + 63) / 64), dim3(256), 0, st, pfv, s1, (long long)ROW * HID, atoms * HID,
                           tmp + OFF_FVW);
        hipLaunchKernelGGL((k_df_fc_dw<HID, A2, 2, true>), dim3(blocks_for_waves((long long)s1 * 4 * 32)), dim3(256), 0, st, dh, a2, B, pf1);
        hipLaunchKernelGGL((k_fit_reduce<4>), dim3(HID * A2 / 64), dim3(256), 0, st, pf1, s1, (long long)HID * A2, HID * A2, tmp + OFF_F1W);
        hipLaunchKernelGGL((k_fit_fc1_bwd_data<HID, A2, Leaky, 2>), dim3(blocks_for_waves(tiles(B) * 32)), dim3(256), 0, st, P + OFF_F1W, dh, a2, B, dz2);
        hipLaunchKernelGGL((k_df_conv_dw<32, 7, S1, 4, P2, P2, 4, DenseStates, true>), dim3(blocks_for_waves((long long)chunks * 4)), dim3(256),
                           0, st, dz2, a1, (const int8_t*)nullptr, (const int64_t*)nullptr, B, pw2);
        hipLaunchKernelGGL((k_df_conv_bwd_data<2>), dim3(blocks_for_waves((tiles((long long)B * S1) + 1) / 2)), dim3(256), 0, st, P + OFF_C2W,
                           dz2, a1, B, dz1);
        hipLaunchKernelGGL((k_df_conv_dw<1, 10, 0, 7, P1, S1, 1, SRC, true>), dim3(blocks_for_waves(chunks)), dim3(256), 0, st, dz1,
                           (const float*)nullptr, S, ix, B, pw1);
        hipLaunchKernelGGL(k_df_conv_bias_part<true>, dim3(B), dim3(64), 0, st, dz1, dz2, B, cb);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(16384 / 16), dim3(256), 0, st, pw2, chunks, 16384LL, 16384, tmp + OFF_C2W);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(512 / 16), dim3(256), 0, st, pw1, chunks, 512LL, 512, tmp + OFF_C1W);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(2), dim3(256), 0, st, cb, B, 64LL, 32, tmp + OFF_C1B);
        hipLaunchKernelGGL((k_fit_reduce<16>), dim3(2), dim3(256), 0, st, cb + 32, B, 64LL, 32, tmp + OFF_C2B);
        hipLaunchKernelGGL(k_df_fisher_add, dim3((NP + 255) / 256), dim3(256), 0, st, tmp, acc, NP, (int)(r0 == 0), (int)(r0 + slab >= n),
                           (double)n, fisher);
    }
    return (int)hipGetLastError();
}

}  // namespace tmcts_df

extern "C" {

long long tm_distnet_fit_workspace(int batch, int atoms) {
    if (batch < 1 || batch > tmcts_df::MAX_BATCH || atoms < 1 || atoms > tmcts_df::ROW) return -1;
    return tmcts_df::layout(batch).total;
}

int tm_distnet_fit_grad(const float* params, const int8_t* states, const float* target, int target_stride, const float* weight,
                        const int64_t* idx, int batch, int atoms, int weighted, float* grad, float* loss, float* workspace,
                        void* stream) {
    return tmcts_df::fit_grad<tmcts_fit::DenseStates>(params, states, target, target_stride, weight, idx, batch, atoms, weighted,
                                                      grad, loss, workspace, stream);
}

int tm_distnet_fit_grad_packed(const float* params, const uint32_t* obs, const float* target, int target_stride,
                               const float* weight, const int64_t* idx, int batch, int atoms, int weighted, float* grad,
                               float* loss, float* workspace, void* stream) {
    if ((uintptr_t)obs & 3) return (int)hipErrorInvalidValue;
    return tmcts_df::fit_grad<tmcts_fit::PackedStates>(params, obs, target, target_stride, weight, idx, batch, atoms, weighted,
                                                       grad, loss, workspace, stream);
}

long long tm_distnet_fit_fisher_workspace(int slab, int atoms) {
    if (slab < 1 || slab > tmcts_df::MAX_BATCH || atoms < 1 || atoms > tmcts_df::ROW) return -1;
    const long long np = tmcts_df::nparam(atoms);
    return tmcts_df::layout(slab).total + tmcts_fit::up4(np) + tmcts_fit::up4(2 * np);
}

int tm_distnet_fit_fisher(const float* params, const int8_t* states, const float* target, int target_stride, const float* weight,
                          const int64_t* idx, long long n, int slab, int atoms, int weighted, float* fisher, float* workspace,
                          void* stream) {
    return tmcts_df::fit_fisher<tmcts_fit::DenseStates>(params, states, target, target_stride, weight, idx, n, slab, atoms, weighted,
                                                        fisher, workspace, stream);
}

int tm_distnet_fit_fisher_packed(const float* params, const uint32_t* obs, const float* target, int target_stride,
                                 const float* weight, const int64_t* idx, long long n, int slab, int atoms, int weighted,
                                 float* fisher, float* workspace, void* stream) {
    if ((uintptr_t)obs & 3) return (int)hipErrorInvalidValue;
    return tmcts_df::fit_fisher<tmcts_fit::PackedStates>(params, obs, target, target_stride, weight, idx, n, slab, atoms, weighted,
                                                         fisher, workspace, stream);
}

long long tm_distnet_fit_validate_workspace(int slab, int atoms) {
    if (slab < 1 || slab > tmcts_df::MAX_BATCH || atoms < 1 || atoms > tmcts_df::ROW) return -1;
    return tmcts_df::val_layout(slab).total;
}

int tm_distnet_fit_validate(const float* params, const int8_t* states, const float* target, int target_stride, const float* weight,
                            long long n, int chunk, int slab, int atoms, int weighted, double* rows_out, float* workspace,
                            void* stream) {
    return tmcts_df::fit_validate<tmcts_fit::DenseStates>(params, states, target, target_stride, weight, n, chunk, slab, atoms,
                                                          weighted, rows_out, workspace, stream);
}

int tm_distnet_fit_validate_packed(const float* params, const uint32_t* obs, const float* target, int target_stride,
                                   const float* weight, long long n, int chunk, int slab, int atoms, int weighted,
                                   double* rows_out, float* workspace, void* stream) {
    if ((uintptr_t)obs & 3) return (int)hipErrorInvalidValue;
    return tmcts_df::fit_validate<tmcts_fit::PackedStates>(params, obs, target, target_stride, weight, n, chunk, slab, atoms,
                                                           weighted, rows_out, workspace, stream);
}

}  // extern "C"
