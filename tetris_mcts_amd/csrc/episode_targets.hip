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
// k_episode_targets_discounted (tm_episode_targets_discounted) is the same body with a discount gamma per move and, optionally,
// the values taken from an array by table row instead of the rows' value column.  Mode 1 becomes
//     N_i = v_i + lambda (gamma N_{i+1} + B_{i+1} r_i),   B_i = 1 + lambda B_{i+1},   r_i = s_{i+1} - s_i:
// row i is (N, B) -> (v_i + a N + b B, 1 + aB B) with a = lambda gamma, b = lambda r_i, aB = lambda.  The composed maps carry FIVE
// doubles (a, b, oN, oB, aB): a = (lambda gamma)^span and aB = lambda^span are different powers, and a span is not the lane
// distance where rows were left out.  At gamma = 1 a and aB hold the same bits at every step, so every statement is the old
// kernel's.  Mode 0 with gamma < 1 is D_i = r_i + gamma D_{i+1}: the maps D -> o + a D, two doubles, the same scan; with
// gamma = 1 it is the integer statement.  Both kernels include episode_targets_body.inc; k_episode_targets compiles to the
// instructions it had before that file existed (scripts/compare_device_code.py).
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

struct TargetArgsDiscounted : TargetArgs {
    double gamma;
    const float* v_rows;                                        // by TABLE row, or nullptr: the rows' value column
};

// (N, B) -> (oN + a N + b B, oB + aB B); without a discount aB is a
template <bool DISC>
struct Map {
    double a, b, oN, oB;
    __device__ __forceinline__ double aB() const { return a; }
    __device__ __forceinline__ void set_aB(double) {}
};
template <>
struct Map<true> {
    double a, b, oN, oB, aB_;
    __device__ __forceinline__ double aB() const { return aB_; }
    __device__ __forceinline__ void set_aB(double x) { aB_ = x; }
};

// first g, then f
template <bool DISC>
__device__ __forceinline__ Map<DISC> compose(const Map<DISC>& f, const Map<DISC>& g) {
    Map<DISC> h;
    h.a = f.a * g.a;
    h.b = f.a * g.b + f.b * g.aB();
    h.oN = f.oN + (f.a * g.oN + f.b * g.oB);
    h.oB = f.oB + f.aB() * g.oB;
    h.set_aB(f.aB() * g.aB());
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
#define ET_DISCOUNTED 0
#include "episode_targets_body.inc"
#undef ET_DISCOUNTED
}

__global__ __launch_bounds__(ET_THREADS) void k_episode_targets_discounted(TargetArgsDiscounted A) {
#define ET_DISCOUNTED 1
#include "episode_targets_body.inc"
#undef ET_DISCOUNTED
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

// what both target calls refuse (hipErrorInvalidValue); 0 with *work = false: nothing to do
static int check_targets(const void* rows, int n_rows, const int32_t* order, const int32_t* seg, int n_seg, const uint8_t* tail_kind,
                         const int32_t* tail_score, const float* tail_value, int mode, double lambda, int weight_mode,
                         const float* value, const float* variance, const float* weight, const int32_t* fault, bool* work) {
    *work = false;
    if (n_rows < 0 || n_seg < 0 || mode < 0 || mode > 2 || weight_mode < 0 || weight_mode > 3) return (int)hipErrorInvalidValue;
    if (n_rows > 0x7FFFFFFF - 64) return (int)hipErrorInvalidValue;                            // a chunk's positions stay ints
    if (!(lambda >= 0.0 && lambda <= 1.0)) return (int)hipErrorInvalidValue;                   // (a NaN is refused too)
    if (n_rows == 0 || n_seg == 0) return 0;
    if (!rows || !order || !seg || !tail_kind || !tail_score || !tail_value || !value || !variance || !weight || !fault)
        return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(rows) & 3) != 0) return (int)hipErrorInvalidValue;         // rows are read as dwords
    *work = true;
    return 0;
}

static void fill_targets(TargetArgs& A, const void* rows, int n_rows, const int32_t* order, const int32_t* seg, int n_seg,
                         const uint8_t* tail_kind, const int32_t* tail_score, const float* tail_value, int mode, double lambda,
                         int weight_mode, float eps, float* value, float* variance, float* weight, int32_t* fault) {
    A.rows = reinterpret_cast<const uint32_t*>(rows);
    A.order = order; A.seg = seg;
    A.tail_kind = tail_kind; A.tail_score = tail_score; A.tail_value = tail_value;
    A.value = value; A.variance = variance; A.weight = weight; A.fault = fault;
    A.lambda = lambda; A.eps = eps;
    A.n_rows = n_rows; A.n_seg = n_seg; A.mode = mode; A.weight_mode = weight_mode;
}

int tm_episode_targets(const void* rows, int n_rows, const int32_t* order, const int32_t* seg, int n_seg, const uint8_t* tail_kind,
                       const int32_t* tail_score, const float* tail_value, int mode, double lambda, int weight_mode, float eps,
                       float* value, float* variance, float* weight, int32_t* fault, void* stream) {
    bool work;
    const int rc = check_targets(rows, n_rows, order, seg, n_seg, tail_kind, tail_score, tail_value, mode, lambda, weight_mode, value,
                                 variance, weight, fault, &work);
    if (!work) return rc;
    TargetArgs A;
    fill_targets(A, rows, n_rows, order, seg, n_seg, tail_kind, tail_score, tail_value, mode, lambda, weight_mode, eps, value, variance,
                 weight, fault);
    hipLaunchKernelGGL(k_episode_targets, dim3((n_seg + ET_WAVES - 1) / ET_WAVES), dim3(ET_THREADS), 0, (hipStream_t)stream, A);
    return (int)hipGetLastError();
}

int tm_episode_targets_discounted(const void* rows, int n_rows, const int32_t* order, const int32_t* seg, int n_seg,
                                  const uint8_t* tail_kind, const int32_t* tail_score, const float* tail_value, const float* v_rows,
                                  int mode, double lambda, double gamma, int weight_mode, float eps, float* value, float* variance,
                                  float* weight, int32_t* fault, void* stream) {
    if (!(gamma > 0.0 && gamma <= 1.0)) return (int)hipErrorInvalidValue;                      // (a NaN is refused too)
    if (v_rows && mode == 0) return (int)hipErrorInvalidValue;                                 // mode 0 reads no value
    if ((reinterpret_cast<uintptr_t>(v_rows) & 3) != 0) return (int)hipErrorInvalidValue;
    bool work;
    const int rc = check_targets(rows, n_rows, order, seg, n_seg, tail_kind, tail_score, tail_value, mode, lambda, weight_mode, value,
                                 variance, weight, fault, &work);
    if (!work) return rc;
    TargetArgsDiscounted A;
    fill_targets(A, rows, n_rows, order, seg, n_seg, tail_kind, tail_score, tail_value, mode, lambda, weight_mode, eps, value, variance,
                 weight, fault);
    A.gamma = gamma; A.v_rows = v_rows;
    hipLaunchKernelGGL(k_episode_targets_discounted, dim3((n_seg + ET_WAVES - 1) / ET_WAVES), dim3(ET_THREADS), 0,
                       (hipStream_t)stream, A);
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
