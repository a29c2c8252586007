// Categorical training targets from recorded episodes (tm_episode_dist_targets): what the distributional search's backup does
// along a trace - shift a distribution by the score gained, mix it into the node above (tree.hip wave_dist_back; the reference's
// backup_trace_distributional / shift_distribution) - done along the moves actually PLAYED.  The rows, order / seg and the tails
// are tm_episode_targets' (episode_targets.hip); the result is a row of `atoms` float32 per sorted position.
//
// The shift S_c(p) by an integer score difference c >= 0 over K atoms of width delta = (vmax - vmin) / K:
//     bs = (double)c / delta, n = floor(bs), f = bs - n;  source atom a gives p[a] (1 - f) to lb = min(a + n, K-1) and p[a] f to
//     min(lb + 1, K-1).
// In GATHER form, which is what a lane per atom wants (n is taken as min(n, K): from K-1 on everything is in the top atom):
//     b < K-1:   out[b] = p[b-n] (1 - f) + p[b-n-1] f                   (a source below atom 0 is 0)
//     b = K-1:   out[b] = suf[max(K-1-n, 0)] + p[K-2-n] f,   suf[a] = p[a] + p[a+1] + .. + p[K-1]
// (the sources that land on the top atom give it (1 - f) + f of their mass: all of it, which is why suf carries no factor).
// suf is a SEQUENTIAL fp64 sum from the top atom down - the numpy statement's cumsum - so both sides add in one order.
//
// mode 0: target_i = S_{s_end - s_i}(e_0), e_0 = all mass in atom 0: at most two atoms, no distribution read
//         (k_dist_targets_mc: a wave per position).
// mode 1: target_i = sum_{k=0..m} lambda^k S_{s_{i+k} - s_i}(P_{i+k}) / sum_{k=0..m} lambda^k over the series of the rows that
//         exist and the tail (e_0 at tail_score), m = min(horizon, elements after i); per atom in fp64, ascending k, the weight by
//         repeated multiplication, one division and one rounding to fp32 at the end (k_dist_targets_lambda).
// Two shifts composed are not the shift by the sum (each interpolates), so there is no recurrence to scan: every term is one
// exact shift of a recorded row's distribution, and a target depends on no other target.
//
// k_dist_targets_lambda: a workgroup of four waves owns 64 consecutive sorted positions (its TARGETS; a block may span several
// short episodes - a position finds its episode by bisection of seg, so long episodes are split over workgroups by position
// and nothing is carried).  It walks the positions from its first target on in CHUNKS of 64: the chunk's distributions are
// staged once in LDS ([64][65] float, the pad for the pass below), wave 0 adds the suffix sums (a lane per row, 64 sequential
// adds) and counts the rows that exist (ballot), then each wave takes its 16 targets in turn, a lane per atom: lane l first
// computes (n, f) of element l against the target - one fp64 division for the 64 elements - and the elements are then taken in
// order, (n, f) broadcast by __shfl, two LDS reads, the accumulator of (target, atom) in a register.  k is a difference of the
// running count of rows that exist, so a position whose order entry is not a row is simply not an element.  The walk ends when
// every target has met its horizon or its episode's end (__syncthreads_and).
//
// k_dist_targets_rows goes first (a thread per position): weight[j] by tm_episode_targets' four rules, and for an order entry
// that is not a row zeros, weight 0 and bit 0 of *fault.  Bit 1 (a score that fell) is set by the target kernels, which run
// AFTER it on the stream: they store (the word as it stands) | 2, the same value from every thread that stores, so no atomic is
// needed and no bit is lost.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/tetris_mcts_hip.h"

namespace tmcts {

constexpr int DT_THREADS = 256, DT_WAVES = DT_THREADS / 64;
constexpr int DT_RUN = 64;                                      // targets of a workgroup = positions of a chunk
constexpr int DT_PER_WAVE = DT_RUN / DT_WAVES;
constexpr int DT_PAD = DT_RUN + 1;
constexpr int DT_ROW_DW = TM_EPISODE_ROW_BYTES / 4;
constexpr int DT_SCORE = 6, DT_VARIANCE = 12, DT_VISITS = 13;   // dword offsets (include/tetris_mcts_hip.h, tm_episode_record)
static_assert(DT_ROW_DW == 92 && DT_RUN == 64 && TM_DIST_ROW == 64, "a lane per atom, a lane per row of a chunk");

struct DistTargetArgs {
    const uint32_t* rows;
    const int32_t* order;
    const int32_t* seg;
    const uint8_t* tail_kind;
    const int32_t* tail_score;
    const float* p_rows;
    float* target;
    float* weight;
    int32_t* fault;
    double delta, lambda;
    float eps;
    int n_rows, n_seg, p_stride, target_stride, atoms, horizon, weight_mode;
};

// the segment of sorted position p: the last e with seg[e] <= p, if p < seg[e + 1]; -1: no segment holds p.  (seg does not
// fall; in a table that does, p gets the segment the bisection meets - every address formed from it is checked all the same.)
__device__ __forceinline__ int segment_of(const int32_t* __restrict__ seg, int n_seg, int p) {
    if (seg[0] > p) return -1;
    int lo = 0, hi = n_seg;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (seg[mid] <= p) lo = mid; else hi = mid;
    }
    return p < seg[lo + 1] ? lo : -1;
}

__device__ __forceinline__ double dt_shfl_f64(double x, int src) {
    const long long bits = __double_as_longlong(x);
    const int lo = __shfl((int)(bits & 0xFFFFFFFFll), src), hi = __shfl((int)(bits >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (long long)(uint32_t)lo);
}

// (n, f) of a score difference; a negative one is taken as 0 and reported
__device__ __forceinline__ void shift_of(long long c, double delta, int K, int& n, double& f, bool& fell) {
    fell = c < 0;
    if (fell) c = 0;
    const double bs = (double)c / delta, fl = floor(bs);
    f = bs - fl;
    n = fl >= (double)K ? K : (int)fl;
}

// atom `lane` of S(e_0): the gather form with p = (1, 0, 0, ..)
__device__ __forceinline__ double shifted_unit(int lane, int K, int n, double f) {
    if (lane < K - 1) {
        const int src = lane - n;
        const double u = src == 0 ? 1.0 * (1.0 - f) : 0.0, v = src == 1 ? 1.0 * f : 0.0;
        return u + v;
    }
    const int top = K - 1 - n;
    return (top <= 0 ? 1.0 : 0.0) + (top == 1 ? 1.0 * f : 0.0);
}

__global__ __launch_bounds__(DT_THREADS) void k_dist_targets_rows(DistTargetArgs A) {
    const long long ql = (long long)blockIdx.x * DT_THREADS + threadIdx.x;
    if (ql <= A.n_seg) {
        const int v = A.seg[ql];
        if (v < 0 || v > A.n_rows) A.fault[0] = 1;
    }
    if (ql >= A.n_rows) return;
    const int q = (int)ql;
    if (segment_of(A.seg, A.n_seg, q) < 0) return;
    const int r = A.order[q];
    if (r < 0 || r >= A.n_rows) {
        A.fault[0] = 1;
        A.weight[q] = 0.0f;
        for (int b = 0; b < A.atoms; ++b) A.target[(size_t)q * A.target_stride + b] = 0.0f;
        return;
    }
    const uint32_t* row = A.rows + (size_t)r * DT_ROW_DW;
    const float var = __uint_as_float(row[DT_VARIANCE]);
    float w = 1.0f;
    if (A.weight_mode >= 2) {
        const float* st = reinterpret_cast<const float*>(row + DT_VISITS);
        float sum = st[0];
#pragma unroll
        for (int a = 1; a < 7; ++a) sum = sum + st[a];
        w = sum;
    }
    if (A.weight_mode == 1 || A.weight_mode == 3) w = w / (var + A.eps);
    A.weight[q] = w;
}

__global__ __launch_bounds__(DT_THREADS) void k_dist_targets_mc(DistTargetArgs A) {
    const int lane = threadIdx.x & 63;
    const long long pl = (long long)blockIdx.x * DT_WAVES + (threadIdx.x >> 6);
    if (pl >= A.n_rows) return;                                 // (wave-uniform, as everything below but the store)
    const int p = (int)pl, K = A.atoms;
    const int e = segment_of(A.seg, A.n_seg, p);
    if (e < 0) return;
    const int r = A.order[p];
    if (r < 0 || r >= A.n_rows) return;                         // (k_dist_targets_rows wrote its zeros)
    const int s = (int)A.rows[(size_t)r * DT_ROW_DW + DT_SCORE];
    int s_end = s;
    if (A.tail_kind[e] == 1) {
        s_end = A.tail_score[e];
    } else {                                                    // the last row of the episode that exists (p itself at the latest)
        const int end = min(A.seg[e + 1], A.n_rows);
        for (int j = end - 1; j > p; --j) {
            const int rj = A.order[j];
            if (rj >= 0 && rj < A.n_rows) { s_end = (int)A.rows[(size_t)rj * DT_ROW_DW + DT_SCORE]; break; }
        }
    }
    int n;
    double f;
    bool fell;
    shift_of((long long)s_end - (long long)s, A.delta, K, n, f, fell);
    if (fell && lane == 0) A.fault[0] = A.fault[0] | 2;
    if (lane < K) A.target[(size_t)p * A.target_stride + lane] = (float)shifted_unit(lane, K, n, f);
}

__global__ __launch_bounds__(DT_THREADS) void k_dist_targets_lambda(DistTargetArgs A) {
    __shared__ double sSuf[DT_RUN][DT_PAD];                     // [row of the chunk][atom]: p[atom] + .. + p[K-1]
    __shared__ float sP[DT_RUN][DT_PAD];                        // [row of the chunk][atom]
    __shared__ int tS[DT_RUN], tEnd[DT_RUN], tOk[DT_RUN], tTail[DT_RUN], tTailS[DT_RUN], tV[DT_RUN];      // by target
    __shared__ double tW[DT_RUN], tWk[DT_RUN];                  // by target: sum of the weights so far, the next weight
    __shared__ int cS[DT_RUN], cOk[DT_RUN], cV[DT_RUN];         // by row of the chunk; cV: rows that exist up to and with it
    __shared__ unsigned long long cMask;
    __shared__ int sMaxEnd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = A.atoms, H = A.lambda == 0.0 ? 0 : A.horizon;
    const int p0 = (int)((long long)blockIdx.x * DT_RUN);       // (< n_rows <= 2^31 - 65: p0 + 64 stays an int)

    if (tid < DT_RUN) {                                         // wave 0, all of its lanes
        const int p = p0 + tid;
        int ok = 0, s = 0, end = 0, tail = 0, ts = 0;
        if (p < A.n_rows) {
            const int e = segment_of(A.seg, A.n_seg, p);
            if (e >= 0) {
                const int r = A.order[p];
                if (r >= 0 && r < A.n_rows) {
                    ok = 1;
                    s = (int)A.rows[(size_t)r * DT_ROW_DW + DT_SCORE];
                    end = min(A.seg[e + 1], A.n_rows);
                    tail = A.tail_kind[e] == 1;
                    ts = A.tail_score[e];
                }
            }
        }
        tOk[tid] = ok; tS[tid] = s; tEnd[tid] = end; tTail[tid] = tail; tTailS[tid] = ts;
        int m = end;                                            // (0 where there is no target)
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) m = max(m, __shfl_xor(m, k));
        if (tid == 0) sMaxEnd = m;
    }
    __syncthreads();
    const int max_end = sMaxEnd;
    if (max_end == 0) return;                                   // (block-uniform) no target here

    // the accumulators of the wave's 16 targets stay in registers (a lane per atom); the loop over the targets is NOT unrolled -
    // its body exists once and picks its accumulator with a chain of selects - and the two wave-uniform doubles of a target
    // live in LDS, touched by its own wave alone
    double acc[DT_PER_WAVE];
    unsigned done = 0;                                          // bit tt: target wave * 16 + tt needs nothing more (wave-uniform)
#pragma unroll
    for (int tt = 0; tt < DT_PER_WAVE; ++tt) {
        acc[tt] = 0.0;
        if (!tOk[wave * DT_PER_WAVE + tt]) done |= 1u << tt;
    }
    if (lane < DT_PER_WAVE) { tW[wave * DT_PER_WAVE + lane] = 0.0; tWk[wave * DT_PER_WAVE + lane] = 1.0; }
    bool fell = false;
    int base = 0;                                               // wave 0: the rows that exist before this chunk

    for (int cs = p0; cs < max_end; cs += DT_RUN) {
        // ---- stage the chunk: wave w loads rows w, w + 4, ..; a lane per atom, 256 contiguous bytes a row
        for (int it = 0; it < DT_PER_WAVE; ++it) {
            const int row = it * DT_WAVES + wave, p = cs + row;
            int r = -1;
            if (p < max_end) r = A.order[p];
            const bool ok = r >= 0 && r < A.n_rows;
            float v = 0.0f;
            if (ok && lane < K) v = A.p_rows[(size_t)r * A.p_stride + lane];        // (the padding atoms are never read)
            sP[row][lane] = v;
            if (lane == 0) {
                cOk[row] = ok;
                cS[row] = ok ? (int)A.rows[(size_t)r * DT_ROW_DW + DT_SCORE] : 0;
            }
        }
        __syncthreads();
        if (tid < DT_RUN) {
            const unsigned long long mask = __ballot(cOk[tid] != 0);
            const int v = base + __popcll(mask & ((2ull << tid) - 1ull));
            cV[tid] = v;
            if (cs == p0) tV[tid] = v;
            base += __popcll(mask);
            if (tid == 0) cMask = mask;
            double s = (double)sP[tid][K - 1];
            sSuf[tid][K - 1] = s;
            for (int a = K - 2; a >= 0; --a) {
                s = s + (double)sP[tid][a];
                sSuf[tid][a] = s;
            }
        }
        __syncthreads();
        const unsigned long long mask = cMask;

        // ---- the terms of this chunk, target by target
#pragma unroll 1
        for (int tt = 0; tt < DT_PER_WAVE; ++tt) {
            if ((done >> tt) & 1u) continue;
            const int i = wave * DT_PER_WAVE + tt;
            const int s_i = tS[i], end_i = tEnd[i], v_i = tV[i];
            double a = 0.0, wsum = tW[i], wk = tWk[i];
#pragma unroll
            for (int u = 0; u < DT_PER_WAVE; ++u) a = u == tt ? acc[u] : a;
            int n_l;
            double f_l;
            bool fell_l;
            shift_of((long long)cS[lane] - (long long)s_i, A.delta, K, n_l, f_l, fell_l);
            const unsigned long long fell_mask = __ballot(fell_l);
            const int jlo = cs == p0 ? i : 0, jhi = min(DT_RUN, end_i - cs);
            for (int j = jlo; j < jhi; ++j) {
                if (!((mask >> j) & 1ull)) continue;            // not a row: not an element of the series
                if (cV[j] - v_i > H) { done |= 1u << tt; break; }
                if ((fell_mask >> j) & 1ull) fell = true;
                const int n = __shfl(n_l, j);
                const double f = dt_shfl_f64(f_l, j);
                double t;
                if (lane < K - 1) {
                    const int src = lane - n;
                    const double u = src >= 0 ? (double)sP[j][src] * (1.0 - f) : 0.0;
                    const double v = src >= 1 ? (double)sP[j][src - 1] * f : 0.0;
                    t = u + v;
                } else {                                        // the top atom (lanes past it compute it too and store nothing)
                    const int top = K - 1 - n;
                    const double v = top >= 1 ? (double)sP[j][top - 1] * f : 0.0;
                    t = sSuf[j][top > 0 ? top : 0] + v;
                }
                a = a + wk * t;
                wsum = wsum + wk;
                wk = wk * A.lambda;
            }
            if (!((done >> tt) & 1u) && end_i - cs <= DT_RUN) {  // the episode's last row is in this chunk: the tail, and done
                if (tTail[i] && cV[end_i - 1 - cs] - v_i + 1 <= H) {
                    int n;
                    double f;
                    bool fell_t;
                    shift_of((long long)tTailS[i] - (long long)s_i, A.delta, K, n, f, fell_t);
                    if (fell_t) fell = true;
                    const double t = shifted_unit(lane, K, n, f);
                    a = a + wk * t;
                    wsum = wsum + wk;
                }
                done |= 1u << tt;
            }
            // (the horizon is used up with this chunk: no later chunk is staged only to find that out)
            if (jhi == DT_RUN && cV[DT_RUN - 1] - v_i >= H) done |= 1u << tt;
#pragma unroll
            for (int u = 0; u < DT_PER_WAVE; ++u) acc[u] = u == tt ? a : acc[u];
            if (lane == 0) { tW[i] = wsum; tWk[i] = wk; }
        }
        // (also the barrier between this chunk's reads and the next one's stores)
        if (__syncthreads_and(done == (1u << DT_PER_WAVE) - 1u)) break;
    }

#pragma unroll
    for (int tt = 0; tt < DT_PER_WAVE; ++tt) {
        const int i = wave * DT_PER_WAVE + tt;
        if (tOk[i] && lane < K) A.target[(size_t)(p0 + i) * A.target_stride + lane] = (float)(acc[tt] / tW[i]);
    }
    if (fell && lane == 0) A.fault[0] = A.fault[0] | 2;
}

}  // namespace tmcts

using namespace tmcts;

extern "C" {

int tm_episode_dist_targets(const void* rows, int n_rows, const int32_t* order, const int32_t* seg, int n_seg, const uint8_t* tail_kind,
                            const int32_t* tail_score, const float* p_rows, int p_stride, int atoms, double vmin, double vmax, int mode,
                            double lambda, int horizon, int weight_mode, float eps, float* target, int target_stride, float* weight,
                            int32_t* fault, void* stream) {
    if (n_rows < 0 || n_seg < 0 || mode < 0 || mode > 1 || weight_mode < 0 || weight_mode > 3) return (int)hipErrorInvalidValue;
    if (n_rows > 0x7FFFFFFF - 64) return (int)hipErrorInvalidValue;                            // a chunk's positions stay ints
    if (!(lambda >= 0.0 && lambda <= 1.0)) return (int)hipErrorInvalidValue;                   // (a NaN is refused too)
    if (atoms < 1 || atoms > TM_DIST_ROW || target_stride < atoms || horizon < 0) return (int)hipErrorInvalidValue;
    if (mode == 1 && p_stride < atoms) return (int)hipErrorInvalidValue;
    if (!isfinite(vmin) || !isfinite(vmax) || !(vmax > vmin) || !isfinite(vmax - vmin)) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(p_rows) & 3) != 0 || (reinterpret_cast<uintptr_t>(target) & 3) != 0)
        return (int)hipErrorInvalidValue;
    if (n_rows == 0 || n_seg == 0) return 0;
    if (!rows || !order || !seg || !tail_kind || !tail_score || !target || !weight || !fault) return (int)hipErrorInvalidValue;
    if (mode == 1 && !p_rows) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(rows) & 3) != 0) return (int)hipErrorInvalidValue;         // rows are read as dwords
    const double delta = (vmax - vmin) / atoms;
    if (!(delta > 0.0)) return (int)hipErrorInvalidValue;                                      // (a range that underflows)
    DistTargetArgs A;
    A.rows = reinterpret_cast<const uint32_t*>(rows);
    A.order = order; A.seg = seg; A.tail_kind = tail_kind; A.tail_score = tail_score; A.p_rows = p_rows;
    A.target = target; A.weight = weight; A.fault = fault;
    A.delta = delta; A.lambda = lambda; A.eps = eps;
    A.n_rows = n_rows; A.n_seg = n_seg; A.p_stride = p_stride; A.target_stride = target_stride; A.atoms = atoms;
    A.horizon = horizon; A.weight_mode = weight_mode;
    const long long per_thread = (long long)(n_rows > n_seg + 1 ? n_rows : n_seg + 1);
    hipLaunchKernelGGL(k_dist_targets_rows, dim3((unsigned)((per_thread + DT_THREADS - 1) / DT_THREADS)), dim3(DT_THREADS), 0,
                       (hipStream_t)stream, A);
    if (mode == 0)
        hipLaunchKernelGGL(k_dist_targets_mc, dim3((unsigned)(((long long)n_rows + DT_WAVES - 1) / DT_WAVES)), dim3(DT_THREADS), 0,
                           (hipStream_t)stream, A);
    else
        hipLaunchKernelGGL(k_dist_targets_lambda, dim3((unsigned)(((long long)n_rows + DT_RUN - 1) / DT_RUN)), dim3(DT_THREADS), 0,
                           (hipStream_t)stream, A);
    return (int)hipGetLastError();
}

}  // extern "C"
