// Dense evaluation requests for evaluators the engine does not own (a Python callable, the torch back ends, a caller of the C
// protocol with a network of their own): tm_eval_gather compacts the request slots a tm_sim_step launch posted (eval_obs[j] != 0)
// into a dense batch of rendered observations, tm_eval_scatter / tm_eval_scatter_dist put the evaluator's rows back into the
// slots the backup reads.  The built-in nets draw the same economy from eval_list inside their own kernels (valuenet.hip,
// distnet.hip); what is here hands it to everybody else.
//
// The order of the batch is the ascending slot index, so it is the same from run to run (eval_list's order depends on which
// game's atomic came first) and the call does not depend on eval_parity.
//
// k_eval_gather: workgroup b owns the GATHER_SHARE slots from b * GATHER_SHARE.  It finds the dense position of its first request
// by counting the non-zero slots before its share itself (all its threads, 16-byte loads: the slots of 32 768 leaf-parallel games
// are 0.9 MB, read from L2), so no workgroup waits for another one and no atomic decides the order.  Its own share is ranked with
// wave ballots, listed in LDS, and rendered a request per wave: the packed observation in lanes 0..11 (TM_KIND_DIST: packed from
// the node's game, as k_eval_render does), 50 lanes storing four cells each as one dword.  The last workgroup knows the total:
// it writes `count` and the padding rows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tetris_mcts_hip.h"
#include "engine.h"

namespace tmcts {

constexpr int GATHER_THREADS = 256, GATHER_WAVES = GATHER_THREADS / 64;
constexpr int GATHER_PER = TM_EVAL_GATHER_SHARE / GATHER_THREADS;     // slots of the share per thread
static_assert(TM_EVAL_GATHER_SHARE % GATHER_THREADS == 0 && TM_EVAL_GATHER_SHARE % 4 == 0, "whole rounds of the workgroup, whole 16-byte loads");
constexpr int ROW_DW = 50;      // a rendered observation: 200 int8 cells

struct GatherArgs {
    const int32_t* eval_obs;
    const uint32_t* obs_key;     // [G][N][12]
    const uint32_t* node_game;   // [G][N][16] (TM_KIND_DIST: the request names a node)
    int total, eval_slots, max_nodes, dist;
};

// how many of eo[0 .. end) are non-zero, end a multiple of four: this thread's part (every thread of the workgroup calls it)
__device__ __forceinline__ int nonzero_before(const int32_t* __restrict__ eo, int end, int tid) {
    int c = 0;
    if ((reinterpret_cast<uintptr_t>(eo) & 15) == 0) {
        const int4* p = reinterpret_cast<const int4*>(eo);
#pragma unroll 4
        for (int i = tid; i < end / 4; i += GATHER_THREADS) {
            const int4 v = p[i];
            c += (v.x != 0) + (v.y != 0) + (v.z != 0) + (v.w != 0);
        }
    } else {
#pragma unroll 4
        for (int i = tid; i < end; i += GATHER_THREADS) c += eo[i] != 0;
    }
    return c;
}

// the words a request's rendering starts from, one per lane: the packed observation (lanes 0..11) or, TM_KIND_DIST, the node's
// packed game (lanes 0..15).  An index outside the pool reads nothing (the row is then written as zeros).
__device__ __forceinline__ uint32_t request_words(const GatherArgs& A, int2 e, int lane) {
    if ((unsigned)e.y >= (unsigned)A.max_nodes) return 0u;
    const size_t at = (size_t)(e.x / A.eval_slots) * A.max_nodes + e.y;
    if (A.dist) return lane < GAME_DW ? A.node_game[at * GAME_DW + lane] : 0u;
    return lane < OBS_DW ? A.obs_key[at * OBS_DW + lane] : 0u;
}

// TM_KIND_DIST: the packed game in lanes 0..15 -> its packed observation in lanes 0..11 (pack_obs: the rows are the game's, the
// cells and the end word follow from words 10 and 11)
__device__ __forceinline__ uint32_t game_to_obs(uint32_t gw, int lane) {
    uint32_t gm[GAME_DW] = {}, ob[OBS_DW];
    gm[10] = (uint32_t)__shfl((int)gw, 10, 64);
    gm[11] = (uint32_t)__shfl((int)gw, 11, 64);
    if ((gm[10] & 0xFFu) >= 7u || ((gm[10] >> 8) & 0xFFu) >= 4u) gm[10] &= ~0xFFFFu;   // (no piece of the game: keep the table lookup inside)
    pack_obs(gm, ob);
    return lane < 10 ? gw : lane == 10 ? ob[10] : lane == 11 ? ob[11] : 0u;
}

// cells 4 * lane .. 4 * lane + 3 of the packed observation held in lanes 0..11 of kw, one int8 each (obs_cell's values: 0 empty,
// 1 locked, -1 falling piece); every lane of the wave calls it (the shuffles need them all), lanes 0..49 hold a dword of the row
__device__ __forceinline__ uint32_t render_dword(uint32_t kw, int lane) {
    const uint32_t cells = (uint32_t)__shfl((int)kw, 10, 64), endw = (uint32_t)__shfl((int)kw, 11, 64);
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = min(4 * lane + k, 199), r = i / 10, c = i - 10 * r;
        const uint32_t w = (uint32_t)__shfl((int)kw, r >> 1, 64);
        uint32_t v = (w >> (16 * (r & 1) + c)) & 1u;
        const bool pc = ((cells & 0xFF) == (uint32_t)i) | (((cells >> 8) & 0xFF) == (uint32_t)i) |
                        (((cells >> 16) & 0xFF) == (uint32_t)i) | ((cells >> 24) == (uint32_t)i);
        if (!(endw & 0xFFu) && pc) v = 0xFFu;
        out |= v << (8 * k);
    }
    return out;
}

__global__ __launch_bounds__(GATHER_THREADS) void k_eval_gather(GatherArgs A, int cap, int pad, int8_t* __restrict__ states,
                                                                int32_t* __restrict__ slots, int32_t* __restrict__ count) {
    __shared__ int s_before[GATHER_WAVES];
    __shared__ int s_cnt[GATHER_PER * GATHER_WAVES];
    __shared__ int2 s_list[TM_EVAL_GATHER_SHARE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int start = blockIdx.x * TM_EVAL_GATHER_SHARE;

    // the requests before this share
    int c = nonzero_before(A.eval_obs, start, tid);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if (lane == 0) s_before[wave] = c;

    // this share: round h of the workgroup takes slots start + 256 h .., ranked by (round, wave, lane) = ascending slot
    int o[GATHER_PER];
    uint64_t bal[GATHER_PER];
#pragma unroll
    for (int h = 0; h < GATHER_PER; ++h) {
        const int j = start + h * GATHER_THREADS + tid;
        o[h] = j < A.total ? A.eval_obs[j] : 0;
        bal[h] = __ballot(o[h] != 0);
        if (lane == 0) s_cnt[h * GATHER_WAVES + wave] = __popcll(bal[h]);
    }
    __syncthreads();
    int base = 0, n_own = 0;
#pragma unroll
    for (int w = 0; w < GATHER_WAVES; ++w) base += s_before[w];
#pragma unroll
    for (int i = 0; i < GATHER_PER * GATHER_WAVES; ++i) n_own += s_cnt[i];
#pragma unroll
    for (int h = 0; h < GATHER_PER; ++h) {
        if (o[h] == 0) continue;
        int lp = __popcll(bal[h] & ((1ull << lane) - 1ull));
        for (int i = 0; i < h * GATHER_WAVES + wave; ++i) lp += s_cnt[i];
        const int j = start + h * GATHER_THREADS + tid;
        s_list[lp] = make_int2(j, o[h]);
        if (base + lp < cap) slots[base + lp] = j;
    }
    __syncthreads();

    // a request per wave, the next one's words requested before this one is rendered
    const int n_render = min(n_own, cap - min(base, cap));
    uint32_t next = wave < n_render ? request_words(A, s_list[wave], lane) : 0u;
    for (int q = wave; q < n_render; q += GATHER_WAVES) {
        const int2 e = s_list[q];
        uint32_t kw = next;
        if (q + GATHER_WAVES < n_render) next = request_words(A, s_list[q + GATHER_WAVES], lane);
        if (A.dist) kw = game_to_obs(kw, lane);
        const uint32_t dw = render_dword(kw, lane);
        if (lane < ROW_DW)
            reinterpret_cast<uint32_t*>(states + (size_t)(base + q) * 200)[lane] = (unsigned)e.y < (unsigned)A.max_nodes ? dw : 0u;
    }

    // the workgroup of the last share knows the total: the counts and the padding rows [n, m)
    if (blockIdx.x == gridDim.x - 1) {
        const int R = base + n_own, n = min(R, cap);
        const int m = (int)min((long long)cap, ((long long)n + pad - 1) / pad * pad);
        if (tid == 0) { count[0] = R; count[1] = n; }
        uint32_t* z = reinterpret_cast<uint32_t*>(states + (size_t)n * 200);
        for (size_t i = tid; i < (size_t)(m - n) * ROW_DW; i += GATHER_THREADS) z[i] = 0u;
        for (int i = tid; i < m - n; i += GATHER_THREADS) slots[n + i] = -1;
    }
}

// one thread per dense row: the evaluator's outputs back into the request slots
__global__ void k_eval_scatter(int total, const int32_t* __restrict__ slots, const int32_t* __restrict__ count,
                               const float* __restrict__ v, const float* __restrict__ var, float* __restrict__ eval_v,
                               float* __restrict__ eval_var) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total || p >= count[1]) return;
    const int j = slots[p];
    if ((unsigned)j >= (unsigned)total) return;
    eval_v[j] = v[p];
    eval_var[j] = var[p];
}

__global__ void k_eval_scatter_dist(int total, int bins, const int32_t* __restrict__ slots, const int32_t* __restrict__ count,
                                    const float* __restrict__ dist, int dist_stride, float* __restrict__ eval_dist) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total || p >= count[1]) return;
    const int j = slots[p];
    if ((unsigned)j >= (unsigned)total) return;
    const float* src = dist + (size_t)p * dist_stride;
    float* dst = eval_dist + (size_t)j * TM_DIST_ROW;
    for (int b = 0; b < bins; ++b) dst[b] = src[b];
}

}  // namespace tmcts

using namespace tmcts;

extern "C" {

int tm_eval_gather(const tm_store* s, int cap, int pad, int8_t* states, int32_t* slots, int32_t* count, void* stream) {
    if (!s || !states || !slots || !count || cap < 1 || pad < 1) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(states) & 3) != 0) return (int)hipErrorInvalidValue;      // rows are stored as dwords
    const bool dist = s->kind == TM_KIND_DIST;
    if (!s->eval_obs || !(dist ? s->node_game : s->obs_key) || s->n_games < 0 || s->eval_slots < 1 || s->max_nodes < 1)
        return (int)hipErrorInvalidValue;
    GatherArgs A;
    A.eval_obs = s->eval_obs;
    A.obs_key = s->obs_key;
    A.node_game = s->node_game;
    A.total = s->n_games * s->eval_slots;
    A.eval_slots = s->eval_slots;
    A.max_nodes = s->max_nodes;
    A.dist = dist ? 1 : 0;
    const int blocks = A.total > 0 ? (A.total + TM_EVAL_GATHER_SHARE - 1) / TM_EVAL_GATHER_SHARE : 1;
    hipLaunchKernelGGL(k_eval_gather, dim3(blocks), dim3(GATHER_THREADS), 0, (hipStream_t)stream, A, cap, pad, states, slots, count);
    return (int)hipGetLastError();
}

int tm_eval_scatter(const tm_store* s, const int32_t* slots, const int32_t* count, const float* v, const float* var, void* stream) {
    if (!s || !slots || !count || !v || !var || !s->eval_v || !s->eval_var) return (int)hipErrorInvalidValue;
    const int total = s->n_games * s->eval_slots;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(k_eval_scatter, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, total, slots, count, v, var,
                       s->eval_v, s->eval_var);
    return (int)hipGetLastError();
}

int tm_eval_scatter_dist(const tm_store* s, const int32_t* slots, const int32_t* count, const float* dist, int dist_stride,
                         void* stream) {
    if (!s || !slots || !count || !dist || s->kind != TM_KIND_DIST || !s->eval_dist) return (int)hipErrorInvalidValue;
    if (s->dist_bins < 1 || s->dist_bins > TM_DIST_ROW || dist_stride < s->dist_bins) return (int)hipErrorInvalidValue;
    const int total = s->n_games * s->eval_slots;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(k_eval_scatter_dist, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, total, s->dist_bins,
                       slots, count, dist, dist_stride, s->eval_dist);
    return (int)hipGetLastError();
}

}  // extern "C"
