// Training targets from recorded episodes (the reference's train.py:81-131, the part between its DataLoader and its gen_batch):
// tm_episode_targets turns State rows that lie in FILE order (move-major, slot-minor: an episode's rows are n_games rows apart)
// into value / variance / weight per row, and tm_episode_gather_states turns the boards of chosen rows into the float32
// [n][200] that the fit takes.  The 368-byte rows are read where they are; nothing sorts or copies them.
//
// k_episode_targets: a wave per segment (episode), four segments per workgroup.  The wave walks its episode BACKWARDS in chunks
// of 64 positions, lane l holding the row order[seg[e] + 64 c + l]: its score, value, variance and, for the visit weights, the
// seven visits.  Mode 1 (the lambda-return) is the affine recurrence
//     N_i = v_i + lambda (N_{i+1} + B_{i+1} d_i),   B_i = 1 + lambda B_{i+1},   value_i = N_i / B_i,   d_i = s_{i+1} - s_i
// (the DIFFERENCE form: every term is non-negative when scores do not fall and values are not negative, and lambda = 0 leaves
// v_i itself).  Row i is the map (N, B) -> (v_i + a N + b B, 1 + a B) with a = lambda, b = lambda d_i; maps of the shape
// (a, b, oN, oB) are closed under composition, so a chunk is an inclusive suffix scan of 64 maps with __shfl_down in six steps,
// applied to the carry (N, B) of the chunk after it, which is wave-uniform and lives in registers.  All of it is fp64; the result
// is rounded to fp32 once.  A tail (an episode that ended: its FINAL score, value 0) is nothing but the first carry:
// (N, B, s) = (tail_value, 1, tail_score).  Long episodes run their chunks one after the other.
// A position whose order entry is not a row (outside [0, n_rows)) is never turned into an address: it gets zeros and weight 0,
// fault[0] = 1 (a plain store), and it is LEFT OUT of its episode's series - the identity map, and d_i of the row before it
// looks past it to the next row that exists.  seg entries are clamped to [0, n_rows] the same way.
//
// k_episode_gather: a thread per dword of a board - four cells - one float4 store each, so a wave stores 1 KiB contiguously.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tetris_mcts_hip.h"

namespace tmcts {

constexpr int ET_THREADS = 256, ET_WAVES = ET_THREADS / 64;
constexpr int ET_ROW_DW = TM_EPISODE_ROW_BYTES / 4;
// dword offsets of the row's fields (include/tetris_mcts_hip.h, the table at tm_episode_record)
constexpr int ET_SCORE = 6, ET_VALUE = 11, ET_VARIANCE = 12, ET_VISITS = 13, ET_BOARD = 41, ET_BOARD_DW = 50;
static_assert(ET_ROW_DW == 92 && ET_BOARD + ET_BOARD_DW == 91, "the row of the header's table");

struct TargetArgs {
    const uint32_t* rows;
    const int32_t* order;
    const int32_t* seg;
    const uint8_t* tail_kind;
    const int32_t* tail_score;
    const float* tail_value;
    float* value;
    float* variance;
    float* weight;
    int32_t* fault;
    double lambda;
    float eps;
    int n_rows, n_seg, mode, weight_mode;
};

// (N, B) -> (oN + a N + b B, oB + a B)
struct Map {
    double a, b, oN, oB;
};

// first g, then f
__device__ __forceinline__ Map compose(const Map& f, const Map& g) {
    Map h;
    h.a = f.a * g.a;
    h.b = f.a * g.b + f.b * g.a;
    h.oN = f.oN + (f.a * g.oN + f.b * g.oB);
    h.oB = f.oB + f.a * g.oB;
    return h;
}

__device__ __forceinline__ double shfl_down_f64(double x, int k) {
    const long long bits = __double_as_longlong(x);
    const int lo = __shfl_down((int)(bits & 0xFFFFFFFFll), k), hi = __shfl_down((int)(bits >> 32), k);
    return __longlong_as_double(((long long)hi << 32) | (long long)(uint32_t)lo);
}

__device__ __forceinline__ double lane0_f64(double x) {
    const long long bits = __double_as_longlong(x);
    const int lo = __shfl((int)(bits & 0xFFFFFFFFll), 0), hi = __shfl((int)(bits >> 32), 0);
    return __longlong_as_double(((long long)hi << 32) | (long long)(uint32_t)lo);
}

__global__ __launch_bounds__(ET_THREADS) void k_episode_targets(TargetArgs A) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * ET_WAVES + (threadIdx.x >> 6);
    if (e >= A.n_seg) return;                                   // (wave-uniform: no barrier follows)
    int first = A.seg[e], last = A.seg[e + 1];
    if (first < 0 || last > A.n_rows) {
        if (lane == 0) A.fault[0] = 1;
        first = first < 0 ? 0 : first;
        last = last > A.n_rows ? A.n_rows : last;
    }
    if (first >= last) return;
    const bool tail = A.tail_kind[e] == 1;
    // the carry: what lies behind the chunk in hand (wave-uniform)
    double cN = tail ? (double)A.tail_value[e] : 0.0, cB = tail ? 1.0 : 0.0;
    int cs = tail ? A.tail_score[e] : 0;                        // the score of the next element that exists ...
    bool c_has = tail;                                          // ... if there is one
    int s_end = cs;                                             // mode 0: the tail's score, or the last row's
    bool end_has = tail;

    for (int base = first + ((last - first - 1) / 64) * 64; base >= first; base -= 64) {
        const int j = base + lane;
        const bool in = j < last;
        const int r = in ? A.order[j] : -1;
        const bool ok = in && r >= 0 && r < A.n_rows;
        if (in && !ok) A.fault[0] = 1;
        const uint32_t* row = A.rows + (size_t)(ok ? r : 0) * ET_ROW_DW;
        const int s = ok ? (int)row[ET_SCORE] : 0;
        const uint32_t v_bits = ok ? row[ET_VALUE] : 0u, var_bits = ok ? row[ET_VARIANCE] : 0u;
        const float v = __uint_as_float(v_bits), var = __uint_as_float(var_bits);

        float out = 0.0f;
        if (A.mode == 2) {
            out = v;
        } else if (A.mode == 0) {
            if (!end_has) {
                const uint64_t have = __ballot(ok);
                if (have) {
                    s_end = __shfl(s, 63 - __builtin_clzll(have));
                    end_has = true;
                }
            }
            out = (float)((long long)s_end - (long long)s);
        } else {
            // the score of the next row that exists, looking past the ones that do not: first inside the chunk ...
            int s_here = s;
            bool has = ok;
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                const int t = __shfl_down(s_here, k);
                const int th = __shfl_down((int)has, k);
                if (!has && lane + k < 64 && th) { s_here = t; has = true; }
            }
            int s_next = __shfl_down(s_here, 1);
            int next_has = __shfl_down((int)has, 1);
            if (lane == 63 || !next_has) { s_next = cs; next_has = c_has; }       // ... then behind it
            const double d = next_has ? (double)((long long)s_next - (long long)s) : 0.0;
            Map m;
            if (ok) { m.a = A.lambda; m.b = A.lambda * d; m.oN = (double)v; m.oB = 1.0; }
            else { m.a = 1.0; m.b = 0.0; m.oN = 0.0; m.oB = 0.0; }
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                Map g;
                g.a = shfl_down_f64(m.a, k); g.b = shfl_down_f64(m.b, k);
                g.oN = shfl_down_f64(m.oN, k); g.oB = shfl_down_f64(m.oB, k);
                if (lane + k < 64) m = compose(m, g);
            }
            const double N = m.oN + (m.a * cN + m.b * cB), B = m.oB + m.a * cB;
            out = (float)(N / B);
            cN = lane0_f64(N);
            cB = lane0_f64(B);
            const int h0 = __shfl((int)has, 0), s0 = __shfl(s_here, 0);
            if (h0) { cs = s0; c_has = true; }
        }

        float w = 1.0f;
        if (A.weight_mode >= 2) {
            const float* st = reinterpret_cast<const float*>(row + ET_VISITS);
            float sum = ok ? st[0] : 0.0f;
#pragma unroll
            for (int a = 1; a < 7; ++a) sum = sum + (ok ? st[a] : 0.0f);
            w = sum;
        }
        if (A.weight_mode == 1 || A.weight_mode == 3) w = w / (var + A.eps);
        if (in) {
            A.value[j] = ok ? out : 0.0f;
            A.variance[j] = __uint_as_float(var_bits);
            A.weight[j] = ok ? w : 0.0f;
        }
    }
}

__global__ __launch_bounds__(ET_THREADS) void k_episode_gather(const uint32_t* __restrict__ rows, int n_rows,
                                                                const int32_t* __restrict__ idx, int n, float4* __restrict__ out,
                                                                int32_t* __restrict__ fault) {
    const long long q = (long long)blockIdx.x * ET_THREADS + threadIdx.x;
    if (q >= (long long)n * ET_BOARD_DW) return;
    const int k = (int)(q / ET_BOARD_DW), d = (int)(q % ET_BOARD_DW);
    const int r = idx[k];
    uint32_t cells = 0u;
    if (r >= 0 && r < n_rows) cells = rows[(size_t)r * ET_ROW_DW + ET_BOARD + d];
    else if (d == 0) fault[0] = 1;
    float4 f;
    f.x = (float)(int8_t)(cells & 0xFFu);
    f.y = (float)(int8_t)((cells >> 8) & 0xFFu);
    f.z = (float)(int8_t)((cells >> 16) & 0xFFu);
    f.w = (float)(int8_t)(cells >> 24);
    out[q] = f;
}

}  // namespace tmcts

using namespace tmcts;

extern "C" {

int tm_episode_targets(const void* rows, int n_rows, const int32_t* order, const int32_t* seg, int n_seg, const uint8_t* tail_kind,
                       const int32_t* tail_score, const float* tail_value, int mode, double lambda, int weight_mode, float eps,
                       float* value, float* variance, float* weight, int32_t* fault, void* stream) {
    if (n_rows < 0 || n_seg < 0 || mode < 0 || mode > 2 || weight_mode < 0 || weight_mode > 3) return (int)hipErrorInvalidValue;
    if (n_rows > 0x7FFFFFFF - 64) return (int)hipErrorInvalidValue;                            // a chunk's positions stay ints
    if (!(lambda >= 0.0 && lambda <= 1.0)) return (int)hipErrorInvalidValue;                   // (a NaN is refused too)
    if (n_rows == 0 || n_seg == 0) return 0;
    if (!rows || !order || !seg || !tail_kind || !tail_score || !tail_value || !value || !variance || !weight || !fault)
        return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(rows) & 3) != 0) return (int)hipErrorInvalidValue;         // rows are read as dwords
    TargetArgs A;
    A.rows = reinterpret_cast<const uint32_t*>(rows);
    A.order = order; A.seg = seg;
    A.tail_kind = tail_kind; A.tail_score = tail_score; A.tail_value = tail_value;
    A.value = value; A.variance = variance; A.weight = weight; A.fault = fault;
    A.lambda = lambda; A.eps = eps;
    A.n_rows = n_rows; A.n_seg = n_seg; A.mode = mode; A.weight_mode = weight_mode;
    hipLaunchKernelGGL(k_episode_targets, dim3((n_seg + ET_WAVES - 1) / ET_WAVES), dim3(ET_THREADS), 0, (hipStream_t)stream, A);
    return (int)hipGetLastError();
}

int tm_episode_gather_states(const void* rows, int n_rows, const int32_t* idx, int n, float* out, int32_t* fault, void* stream) {
    if (n_rows < 0 || n < 0) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!rows || !idx || !out || !fault) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(rows) & 3) != 0 || (reinterpret_cast<uintptr_t>(out) & 15) != 0)
        return (int)hipErrorInvalidValue;                                                       // dword loads, float4 stores
    const long long quads = (long long)n * ET_BOARD_DW;
    const long long blocks = (quads + ET_THREADS - 1) / ET_THREADS;
    if (blocks > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_episode_gather, dim3((unsigned)blocks), dim3(ET_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(rows), n_rows, idx, n, reinterpret_cast<float4*>(out), fault);
    return (int)hipGetLastError();
}

}  // extern "C"
