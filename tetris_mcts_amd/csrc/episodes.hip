// Self-play records on the device (the reference's util/Data.py State rows, play.py:131-132): tm_episode_record writes one
// 368-byte row per game and move straight from what is already on the device - the packed game, the caller's tm_root_stats
// buffer, the action, the root observation's statistics - and tm_episode_advance numbers the episodes and logs the ones that
// end with their FINAL score and lines.  The device row is the file's row: a flush is a plain copy.
//
// k_episode_record: a wave per game, four games per workgroup.  Lane 0 of the wave packs the game's observation (pack_obs) into
// LDS as k_env_render does; after that every lane builds whole dwords of the row - dword d of pass 0 in lane d, dword 64 + d of
// pass 1 in lanes 0..27 - and stores them, so a row leaves as two coalesced stores.  Lanes 41..90 of the row are the board, four
// cells (obs_cell) a dword.  A game that has ended gets episode = -1 and zeros.
//
// k_episode_advance: ONE workgroup walks the slots in chunks of 256 in ascending order; a wave ballot and the waves' counts in
// LDS give a finishing slot its rank among the slots that finish in this call.  The order is the loop's: no atomics, no
// workgroup waits for another one.
//
// k_episode_record_positions writes, beside every State row, the packed game the row was made from (a position row), and
// k_episode_rerecord makes State rows again from such positions after another search (reanalyse.py): both are described where
// they stand.  k_episode_record_root_dists writes, beside the State rows of a TM_KIND_DIST tree, the root's backed-up distribution
// (a root-distribution row): what the distributional head is fitted to.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tetris_mcts_hip.h"
#include "engine.h"

namespace tmcts {

constexpr int EP_THREADS = 256, EP_WAVES = EP_THREADS / 64;
constexpr int EP_ROW_DW = TM_EPISODE_ROW_BYTES / 4, EP_DONE_DW = TM_EPISODE_DONE_BYTES / 4, EP_SLOT_DW = TM_EPISODE_SLOT_DW;
// dword offsets of the row's fields (include/tetris_mcts_hip.h, the table at tm_episode_record)
constexpr int EP_LS = 7, EP_VALUE = 11, EP_STATS = 13, EP_POLICY = 34, EP_BOARD = 41, EP_ACTION = 91;
static_assert(EP_ROW_DW == 92 && EP_DONE_DW == 10 && EP_BOARD + 50 == EP_ACTION, "the row of the header's table");
// the position row (the table at tm_episode_record_positions)
constexpr int POS_ROW_DW = TM_POSITION_ROW_BYTES / 4, POS_GAME = 4, POS_LS = POS_GAME + GAME_DW;
static_assert(POS_ROW_DW == 24 && POS_LS + 4 == POS_ROW_DW, "the position row of the header's table");
// the root-distribution row (the table at tm_episode_record_root_dists)
constexpr int RD_ROW_DW = TM_ROOT_DIST_ROW_BYTES / 4, RD_DIST = 4;
static_assert(RD_ROW_DW == 68 && RD_DIST + TM_DIST_ROW == RD_ROW_DW, "the root-distribution row of the header's table");

struct RecordArgs {
    const uint32_t* env_game;        // [G][16]
    const int32_t* env_line_stats;   // [G][4]
    const int32_t* gs;               // the tree's control blocks, NULL: value = variance = 0
    const uint32_t* node_rec;
    const uint32_t* obs_stat;
    int n_games, max_nodes, cycle;
};

// the root observation's (value, variance) bits: TreeAgent.get_value_and_variance - gs[ROOT] -> node_rec[.., TM_REC_OBS] ->
// obs_stat[.., 1:3]; an index outside the pool reads nothing
__device__ __forceinline__ uint32_t root_stat(const RecordArgs& A, int g, int which) {
    if (!A.gs) return 0u;
    const uint32_t root = (uint32_t)A.gs[(size_t)g * TM_GS_DW + TM_GS_ROOT];
    if (root >= (uint32_t)A.max_nodes) return 0u;
    const uint32_t o = A.node_rec[((size_t)g * A.max_nodes + root) * TM_REC_DW + TM_REC_OBS];
    if (o >= (uint32_t)A.max_nodes) return 0u;
    return A.obs_stat[((size_t)g * A.max_nodes + o) * 4 + 1 + which];
}

__device__ __forceinline__ uint32_t row_dword(const RecordArgs& A, int g, int d, const uint32_t* gm, const uint32_t* key,
                                              const int32_t* ss, const float* __restrict__ st, int action) {
    if (d >= EP_BOARD && d < EP_ACTION) {
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) out |= ((uint32_t)obs_cell(key, 4 * (d - EP_BOARD) + k) & 0xFFu) << (8 * k);
        return out;
    }
    if (d >= EP_POLICY && d < EP_BOARD) {
        float sum = st[0];
#pragma unroll
        for (int a = 1; a < 7; ++a) sum = sum + st[a];
        return __float_as_uint(st[d - EP_POLICY] / sum);
    }
    if (d >= EP_STATS && d < EP_POLICY) return __float_as_uint(st[d - EP_STATS]);
    if (d >= EP_LS && d < EP_VALUE) return (uint32_t)A.env_line_stats[(size_t)g * 4 + d - EP_LS];
    switch (d) {
        case 0: return (uint32_t)ss[0];
        case 1: return (uint32_t)A.cycle;
        case 2: return (uint32_t)g;
        case 3: return (uint32_t)ss[1];
        case 4: return (uint32_t)(int)(int16_t)(gm[11] >> 16);
        case 5: return gm[15];
        case 6: return gm[14];
        case EP_VALUE: return root_stat(A, g, 0);
        case EP_VALUE + 1: return root_stat(A, g, 1);
        default: return (uint32_t)action & 0xFFu;      // EP_ACTION: the action's byte, three pad bytes of zero
    }
}

__global__ __launch_bounds__(EP_THREADS) void k_episode_record(RecordArgs A, const float* __restrict__ stats,
                                                               const int32_t* __restrict__ action, int32_t* __restrict__ slot_state,
                                                               uint32_t* __restrict__ rows) {
    __shared__ uint32_t s_gm[EP_WAVES][GAME_DW];
    __shared__ uint32_t s_key[EP_WAVES][OBS_DW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * EP_WAVES + wave;
    const bool have = g < A.n_games;
    if (have && lane < GAME_DW) {
        uint32_t w = A.env_game[(size_t)g * GAME_DW + lane];
        if (lane == 10 && ((w & 0xFFu) >= 7u || ((w >> 8) & 0xFFu) >= 4u)) w &= ~0xFFFFu;    // (no piece of the game: keep the table lookup inside)
        s_gm[wave][lane] = w;
    }
    __syncthreads();
    if (have && lane == 0) pack_obs(s_gm[wave], s_key[wave]);
    __syncthreads();
    if (!have) return;
    const uint32_t* gm = s_gm[wave];
    const bool ended = ((gm[11] >> 8) & 1u) != 0;
    int32_t* ss = slot_state + (size_t)g * EP_SLOT_DW;
    uint32_t* row = rows + (size_t)g * EP_ROW_DW;
    if (ended) {
        row[lane] = lane == 0 ? 0xFFFFFFFFu : 0u;
        if (lane < EP_ROW_DW - 64) row[64 + lane] = 0u;
        return;
    }
    const float* st = stats + (size_t)g * 21;
    const int act = action[g];
    row[lane] = row_dword(A, g, lane, gm, s_key[wave], ss, st, act);
    if (lane < EP_ROW_DW - 64) row[64 + lane] = row_dword(A, g, 64 + lane, gm, s_key[wave], ss, st, act);
    if (lane == 0) ss[2] = 1;
}

// Position rows (TM_POSITION_ROW_BYTES): a thread per dword of the G x 24 the call writes, so a wave stores 256 contiguous bytes.
// Dwords 0..3 the State row's identity, 4..19 the packed game, 20..23 its line statistics; an ended game: -1, then zeros.
__global__ __launch_bounds__(EP_THREADS) void k_episode_record_positions(const uint32_t* __restrict__ env_game,
                                                                         const int32_t* __restrict__ env_line_stats, int n_games,
                                                                         int cycle, const int32_t* __restrict__ slot_state,
                                                                         uint32_t* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * EP_THREADS + threadIdx.x;
    if (i >= (long long)n_games * POS_ROW_DW) return;
    const int g = (int)(i / POS_ROW_DW), d = (int)(i % POS_ROW_DW);
    const uint32_t* gm = env_game + (size_t)g * GAME_DW;
    uint32_t out;
    if (((gm[11] >> 8) & 1u) != 0) out = d == 0 ? 0xFFFFFFFFu : 0u;
    else if (d >= POS_LS) out = (uint32_t)env_line_stats[(size_t)g * 4 + d - POS_LS];
    else if (d >= POS_GAME) out = gm[d - POS_GAME];
    else if (d == 0) out = (uint32_t)slot_state[(size_t)g * EP_SLOT_DW];
    else if (d == 1) out = (uint32_t)cycle;
    else if (d == 2) out = (uint32_t)g;
    else out = (uint32_t)slot_state[(size_t)g * EP_SLOT_DW + 1];
    rows[i] = out;
}

// Root-distribution rows (TM_ROOT_DIST_ROW_BYTES): a thread per dword of the n x 68 the call writes, so a wave stores 256 contiguous
// bytes (and, 68 being no multiple of 64, always parts of two rows).  Dwords 0..3 are the State row's identity, copied from the
// row tm_episode_record / tm_episode_rerecord has just written for that slot; 4..67 the bits of node_dist[g][gs[ROOT]][0..63], atoms
// at or beyond dist_bins as 0.  A State row with episode -1: -1, then zeros.  A root outside the pool: zeros for the distribution.
__global__ __launch_bounds__(EP_THREADS) void k_episode_record_root_dists(const uint32_t* __restrict__ state_rows,
                                                                          const int32_t* __restrict__ gs,
                                                                          const uint32_t* __restrict__ node_dist, int n, int max_nodes,
                                                                          int dist_bins, uint32_t* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * EP_THREADS + threadIdx.x;
    if (i >= (long long)n * RD_ROW_DW) return;
    const int g = (int)(i / RD_ROW_DW), d = (int)(i % RD_ROW_DW);
    const uint32_t* st = state_rows + (size_t)g * EP_ROW_DW;
    uint32_t out;
    if (st[0] == 0xFFFFFFFFu) out = d == 0 ? 0xFFFFFFFFu : 0u;
    else if (d < RD_DIST) out = st[d];
    else if (d - RD_DIST >= dist_bins) out = 0u;
    else {
        const uint32_t root = (uint32_t)gs[(size_t)g * TM_GS_DW + TM_GS_ROOT];
        out = root < (uint32_t)max_nodes ? node_dist[((size_t)g * max_nodes + root) * TM_DIST_ROW + d - RD_DIST] : 0u;
    }
    rows[i] = out;
}

// Re-recording (tm_episode_rerecord): k_episode_record's wave per row over the first n games of an environment into which the
// rows' positions were loaded.  Dwords 0..3 and the action's dword are the old row's; every other dword is row_dword's, from the
// loaded game, the searched tree and its statistics buffer.  The dwords row_dword takes from the game alone must be the old
// row's: where they are not (or the loaded game has ended: such a game has no row) the row's first differing column group goes
// into fault[0] by atomicMin as 4 x row + group, and fault[1] counts the row.
__device__ __forceinline__ int guard_group(int d) {
    if (d >= 4 && d < EP_LS) return TM_REREC_SCALARS;
    if (d >= EP_LS && d < EP_VALUE) return TM_REREC_LINE_STATS;
    if (d >= EP_BOARD && d < EP_ACTION) return TM_REREC_BOARD;
    return -1;
}

__global__ __launch_bounds__(EP_THREADS) void k_episode_rerecord(RecordArgs A, const float* __restrict__ stats,
                                                                 const uint32_t* __restrict__ old_rows, int n,
                                                                 uint32_t* __restrict__ rows, int32_t* __restrict__ fault) {
    __shared__ uint32_t s_gm[EP_WAVES][GAME_DW];
    __shared__ uint32_t s_key[EP_WAVES][OBS_DW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * EP_WAVES + wave;
    const bool have = g < n;
    if (have && lane < GAME_DW) {
        uint32_t w = A.env_game[(size_t)g * GAME_DW + lane];
        if (lane == 10 && ((w & 0xFFu) >= 7u || ((w >> 8) & 0xFFu) >= 4u)) w &= ~0xFFFFu;    // (as k_episode_record)
        s_gm[wave][lane] = w;
    }
    __syncthreads();
    if (have && lane == 0) pack_obs(s_gm[wave], s_key[wave]);
    __syncthreads();
    if (!have) return;
    const uint32_t* gm = s_gm[wave];
    const uint32_t* old = old_rows + (size_t)g * EP_ROW_DW;
    uint32_t* row = rows + (size_t)g * EP_ROW_DW;
    const float* st = stats + (size_t)g * 21;
    const int32_t none[2] = {0, 0};       // (episode and move are the old row's: row_dword is not asked for them)
    int group = ((gm[11] >> 8) & 1u) != 0 ? TM_REREC_ENDED : 4;       // this lane's first differing group, 4: none
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int d = 64 * pass + lane;
        if (d >= EP_ROW_DW) break;
        const uint32_t was = old[d];
        const bool copied = d < 4 || d == EP_ACTION;
        const uint32_t now = copied ? was : row_dword(A, g, d, gm, s_key[wave], none, st, 0);
        const int gg = guard_group(d);
        if (gg >= 0 && now != was && gg < group) group = gg;
        row[d] = now;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int other = __shfl_xor(group, o, 64);
        group = other < group ? other : group;
    }
    if (lane == 0 && group < 4) {
        atomicMin(&fault[0], 4 * g + group);
        atomicAdd(&fault[1], 1);
    }
}

__global__ __launch_bounds__(EP_THREADS) void k_episode_advance(const uint32_t* __restrict__ env_game,
                                                                const int32_t* __restrict__ env_line_stats, int n_games, int cycle,
                                                                int32_t* __restrict__ slot_state, int32_t* __restrict__ counters,
                                                                int32_t* __restrict__ done, int cap) {
    __shared__ int s_cnt[EP_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int next_id = counters[0], n_done = counters[1];
    int finished = 0;                     // in the chunks before this one (the same value in every thread)
    for (int base = 0; base < n_games; base += EP_THREADS) {
        const int g = base + tid;
        const bool have = g < n_games;
        int32_t* ss = slot_state + (size_t)(have ? g : 0) * EP_SLOT_DW;
        const uint32_t* e = env_game + (size_t)(have ? g : 0) * GAME_DW;
        const bool live = have && ss[2] != 0;
        const bool fin = live && ((e[11] >> 8) & 1u) != 0;
        const uint64_t bal = __ballot(fin);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int r = finished + __popcll(bal & ((1ull << lane) - 1ull)), chunk = 0;
#pragma unroll
        for (int w = 0; w < EP_WAVES; ++w) {
            if (w < wave) r += s_cnt[w];
            chunk += s_cnt[w];
        }
        if (fin) {
            const long long p = (long long)n_done + r;
            if (p < (long long)cap) {
                int32_t* d = done + (size_t)p * EP_DONE_DW;
                d[0] = ss[0]; d[1] = cycle; d[2] = g; d[3] = ss[1] + 1; d[4] = (int)e[14]; d[5] = (int)e[15];
#pragma unroll
                for (int i = 0; i < 4; ++i) d[6 + i] = env_line_stats[(size_t)g * 4 + i];
            }
            ss[0] = next_id + r;
            ss[1] = 0;
        } else if (live) {
            ss[1] += 1;
        }
        if (have) ss[2] = 0;
        finished += chunk;
        __syncthreads();                  // s_cnt is the next chunk's
    }
    if (tid == 0) { counters[0] = next_id + finished; counters[1] = n_done + finished; }
}

__global__ void k_episode_init(int n_games, int first_id, int32_t* __restrict__ slot_state, int32_t* __restrict__ counters) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0) { counters[0] = first_id + n_games; counters[1] = 0; }
    if (g >= n_games) return;
    int32_t* ss = slot_state + (size_t)g * EP_SLOT_DW;
    ss[0] = first_id + g; ss[1] = 0; ss[2] = 0; ss[3] = 0;
}

}  // namespace tmcts

using namespace tmcts;

extern "C" {

int tm_episode_init(int n_games, int first_id, int32_t* slot_state, int32_t* counters, void* stream) {
    if (!slot_state || !counters || n_games < 1 || first_id < 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_episode_init, dim3((n_games + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_games, first_id, slot_state,
                       counters);
    return (int)hipGetLastError();
}

int tm_episode_record(const tm_store* env, const tm_store* tree, const float* stats, const int32_t* action, int cycle,
                      int32_t* slot_state, void* rows, void* stream) {
    if (!env || !stats || !action || !slot_state || !rows) return (int)hipErrorInvalidValue;
    if (env->n_games < 1 || !env->env_game || !env->env_line_stats) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(rows) & 3) != 0) return (int)hipErrorInvalidValue;        // rows are stored as dwords
    if (tree && (tree->n_games != env->n_games || tree->max_nodes < 1 || !tree->gs || !tree->node_rec || !tree->obs_stat))
        return (int)hipErrorInvalidValue;
    RecordArgs A;
    A.env_game = env->env_game;
    A.env_line_stats = env->env_line_stats;
    A.gs = tree ? tree->gs : nullptr;
    A.node_rec = tree ? tree->node_rec : nullptr;
    A.obs_stat = tree ? tree->obs_stat : nullptr;
    A.n_games = env->n_games;
    A.max_nodes = tree ? tree->max_nodes : 0;
    A.cycle = cycle;
    hipLaunchKernelGGL(k_episode_record, dim3((A.n_games + EP_WAVES - 1) / EP_WAVES), dim3(EP_THREADS), 0, (hipStream_t)stream, A,
                       stats, action, slot_state, reinterpret_cast<uint32_t*>(rows));
    return (int)hipGetLastError();
}

int tm_episode_record_positions(const tm_store* env, const int32_t* slot_state, int cycle, void* rows, void* stream) {
    if (!env || !slot_state || !rows) return (int)hipErrorInvalidValue;
    if (env->n_games < 1 || !env->env_game || !env->env_line_stats) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(rows) & 3) != 0) return (int)hipErrorInvalidValue;
    const long long dwords = (long long)env->n_games * POS_ROW_DW;
    hipLaunchKernelGGL(k_episode_record_positions, dim3((unsigned)((dwords + EP_THREADS - 1) / EP_THREADS)), dim3(EP_THREADS), 0,
                       (hipStream_t)stream, (const uint32_t*)env->env_game, (const int32_t*)env->env_line_stats, env->n_games, cycle,
                       slot_state, reinterpret_cast<uint32_t*>(rows));
    return (int)hipGetLastError();
}

int tm_episode_rerecord(const tm_store* env, const tm_store* tree, const float* stats, const void* old_rows, int n, void* rows,
                        int32_t* fault, void* stream) {
    if (!env || !tree || !stats || !old_rows || !rows || !fault) return (int)hipErrorInvalidValue;
    if (env->n_games < 1 || !env->env_game || !env->env_line_stats || n < 0 || n > env->n_games) return (int)hipErrorInvalidValue;
    if (tree->n_games != env->n_games || tree->max_nodes < 1 || !tree->gs || !tree->node_rec || !tree->obs_stat)
        return (int)hipErrorInvalidValue;
    if (((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(old_rows) | reinterpret_cast<uintptr_t>(fault)) & 3) != 0)
        return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    RecordArgs A;
    A.env_game = env->env_game;
    A.env_line_stats = env->env_line_stats;
    A.gs = tree->gs;
    A.node_rec = tree->node_rec;
    A.obs_stat = tree->obs_stat;
    A.n_games = env->n_games;
    A.max_nodes = tree->max_nodes;
    A.cycle = 0;
    hipLaunchKernelGGL(k_episode_rerecord, dim3((n + EP_WAVES - 1) / EP_WAVES), dim3(EP_THREADS), 0, (hipStream_t)stream, A, stats,
                       reinterpret_cast<const uint32_t*>(old_rows), n, reinterpret_cast<uint32_t*>(rows), fault);
    return (int)hipGetLastError();
}

int tm_episode_record_root_dists(const tm_store* tree, const void* state_rows, int n, void* rows, void* stream) {
    if (!tree || !state_rows || !rows) return (int)hipErrorInvalidValue;
    if (tree->kind != TM_KIND_DIST || !tree->node_dist || !tree->gs) return (int)hipErrorInvalidValue;
    if (n < 0 || n > tree->n_games || tree->max_nodes < 1 || tree->dist_bins < 1 || tree->dist_bins > TM_DIST_ROW)
        return (int)hipErrorInvalidValue;
    if (((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(state_rows)) & 3) != 0) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const long long dwords = (long long)n * RD_ROW_DW;
    hipLaunchKernelGGL(k_episode_record_root_dists, dim3((unsigned)((dwords + EP_THREADS - 1) / EP_THREADS)), dim3(EP_THREADS), 0,
                       (hipStream_t)stream, reinterpret_cast<const uint32_t*>(state_rows), (const int32_t*)tree->gs,
                       reinterpret_cast<const uint32_t*>(tree->node_dist), n, tree->max_nodes, tree->dist_bins,
                       reinterpret_cast<uint32_t*>(rows));
    return (int)hipGetLastError();
}

int tm_episode_advance(const tm_store* env, int cycle, int32_t* slot_state, int32_t* counters, void* done, int cap, void* stream) {
    if (!env || !slot_state || !counters || !done || cap < 1) return (int)hipErrorInvalidValue;
    if (env->n_games < 1 || !env->env_game || !env->env_line_stats) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(done) & 3) != 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_episode_advance, dim3(1), dim3(EP_THREADS), 0, (hipStream_t)stream, env->env_game, env->env_line_stats,
                       env->n_games, cycle, slot_state, counters, reinterpret_cast<int32_t*>(done), cap);
    return (int)hipGetLastError();
}

}  // extern "C"
