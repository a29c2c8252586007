// Game snapshots: the games of an environment copied out (tm_env_save) and, after a check ON THE DEVICE, back in (tm_env_load),
// so that a batch of games goes on in the next self-play run; tm_episode_resume starts the episode recorder in the middle of
// those games.  A game is its 64-byte packed record (ENGINE_SPEC.md section 2) and its four line statistics: nothing else of a
// game lives outside tm_store::env_game / env_line_stats, and the randomizer is a function of (seed, piece_count), both in it.
//
// Why a check: the engine trusts a packed game.  `piece` and `rot` index PIECE_MASK[7][4] and PIECE_CELLS[7][4], lock_piece
// writes rows[y + i] for the box rows of a piece that "does not collide".  Bytes that did not come from the engine would make
// k_env_step and the tree kernels read and write out of bounds.  The rule (the TM_GAME_BAD_* bits of the header) admits every
// state the engine produces and refuses every state whose falling piece is not wholly inside the well.
//
// k_env_check: a lane per game, 64 games a workgroup, the game in a 64-byte LDS slot as k_env_step holds it, so that the
// placement test is the engine's own collides() on the engine's own row layout.  NO value read from a game is an index or a shift
// count before it has passed its test: the mask table is read only for piece <= 6 and rot <= 3 (the indices are clamped as well,
// so that no form of the select can leave the table), collides() is called only for -3 <= x <= 9 and -3 <= y <= 19 (its shift
// count x + 3 is then 0..12, and prow() bounds the rows by itself).
// k_env_count: ONE workgroup adds the games with a fault in a fixed order (a strided pass, then a tree in LDS): no atomics.
// k_env_copy: a thread per dword of the 20 a game has; with a gate it copies only where gate[0] == 0, which is how tm_env_load
// stays all or nothing without the host looking at anything.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tetris_mcts_hip.h"
#include "engine.h"

namespace tmcts {

constexpr int GS_THREADS = 256;

// the fault bits of one game; sl: the game's 16 dwords in LDS, ls: its four line statistics in memory or NULL
__device__ __forceinline__ int game_faults(const uint32_t* sl, const int32_t* ls, int app) {
    int f = 0;
    bool bad_row = false;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t w = sl[i];
        bad_row |= (w & 0xFC00FC00u) != 0u || (w & 0xFFFFu) == 0x3FFu || (w >> 16) == 0x3FFu;
    }
    const uint32_t a = sl[10], b = sl[11];
    const int piece = (int)(a & 0xFFu), rot = (int)((a >> 8) & 0xFFu);
    const int x = (int)(int8_t)((a >> 16) & 0xFFu), y = (int)(int8_t)((a >> 24) & 0xFFu);
    const int drop_ctr = (int)(b & 0xFFu), flags = (int)((b >> 8) & 0xFFu), combo = (int)(int16_t)(b >> 16);
    if (piece > 6) f |= TM_GAME_BAD_PIECE;
    if (rot > 3) f |= TM_GAME_BAD_ROT;
    if (bad_row) f |= TM_GAME_BAD_ROWS;
    bool place;
    if (flags & 1) {
        place = !(rot == 0 && x == 3 && y == 0);       // where spawn() leaves the piece of a game it ends
    } else {
        place = x < -3 || x > 9 || y < -3 || y > 19;
        if (!place && piece <= 6 && rot <= 3) {
            const uint32_t mask = PIECE_MASK[piece <= 6 ? piece : 0][rot <= 3 ? rot : 0];
            place = collides(reinterpret_cast<const uint16_t*>(sl), mask, x, y);
        }
    }
    if (place) f |= TM_GAME_BAD_PLACE;
    if (drop_ctr >= app || (flags & ~3) != 0 || combo < -1 || sl[12] == 0u) f |= TM_GAME_BAD_FIELDS;
    if (ls) {
        bool neg = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) neg |= ls[i] < 0;
        if (neg) f |= TM_GAME_BAD_LINE_STATS;
    }
    return f;
}

__global__ __launch_bounds__(64) void k_env_check(const uint32_t* __restrict__ games, const int32_t* __restrict__ line_stats, int n,
                                                  int app, int32_t* __restrict__ fault) {
    __shared__ uint32_t slots[64][GAME_DW];
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= n) return;
    uint32_t* sl = slots[threadIdx.x];
#pragma unroll
    for (int i = 0; i < GAME_DW; ++i) sl[i] = games[(size_t)g * GAME_DW + i];
    fault[g] = game_faults(sl, line_stats ? line_stats + (size_t)g * 4 : nullptr, app);
}

__global__ __launch_bounds__(GS_THREADS) void k_env_count(const int32_t* __restrict__ fault, int n, int32_t* __restrict__ n_bad) {
    __shared__ int s_cnt[GS_THREADS];
    int mine = 0;
    for (int g = threadIdx.x; g < n; g += GS_THREADS) mine += fault[g] != 0;
    s_cnt[threadIdx.x] = mine;
    __syncthreads();
    for (int half = GS_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s_cnt[threadIdx.x] += s_cnt[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) n_bad[0] = s_cnt[0];
}

// dst_* <- src_* for n games; gate: NULL, or copy only if gate[0] == 0
__global__ __launch_bounds__(GS_THREADS) void k_env_copy(const uint32_t* __restrict__ src_games, const int32_t* __restrict__ src_ls,
                                                         uint32_t* __restrict__ dst_games, int32_t* __restrict__ dst_ls, int n,
                                                         const int32_t* __restrict__ gate) {
    if (gate && gate[0] != 0) return;
    const long long i = (long long)blockIdx.x * GS_THREADS + threadIdx.x;
    const long long n_game_dw = (long long)n * GAME_DW;
    if (i < n_game_dw) dst_games[i] = src_games[i];
    else if (i < n_game_dw + (long long)n * 4) dst_ls[i - n_game_dw] = src_ls[i - n_game_dw];
}

__global__ void k_episode_resume(int n_games, int first_id, const int32_t* __restrict__ move_idx, int32_t* __restrict__ slot_state,
                                 int32_t* __restrict__ counters) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0) { counters[0] = first_id + n_games; counters[1] = 0; }
    if (g >= n_games) return;
    const int m = move_idx[g];
    int32_t* ss = slot_state + (size_t)g * TM_EPISODE_SLOT_DW;
    ss[0] = first_id + g; ss[1] = m > 0 ? m : 0; ss[2] = 0; ss[3] = 0;
}

static inline bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

static int launch_check(const uint32_t* games, const int32_t* line_stats, int n, int app, int32_t* fault, int32_t* n_bad,
                        hipStream_t stream) {
    hipLaunchKernelGGL(k_env_check, dim3((n + 63) / 64), dim3(64), 0, stream, games, line_stats, n, app, fault);
    hipLaunchKernelGGL(k_env_count, dim3(1), dim3(GS_THREADS), 0, stream, fault, n, n_bad);
    return (int)hipGetLastError();
}

static unsigned copy_blocks(int n) { return (unsigned)(((long long)n * (GAME_DW + 4) + GS_THREADS - 1) / GS_THREADS); }

}  // namespace tmcts

using namespace tmcts;

extern "C" {

int tm_env_check(const uint32_t* games, const int32_t* line_stats, int n, int app, int32_t* fault, int32_t* n_bad, void* stream) {
    if (!games || !fault || !n_bad || n < 1 || app < 1) return (int)hipErrorInvalidValue;
    if (misaligned4(games) || misaligned4(line_stats) || misaligned4(fault) || misaligned4(n_bad)) return (int)hipErrorInvalidValue;
    return launch_check(games, line_stats, n, app, fault, n_bad, (hipStream_t)stream);
}

int tm_env_save(const tm_store* s, uint32_t* games, int32_t* line_stats, void* stream) {
    if (!s || !games || !line_stats) return (int)hipErrorInvalidValue;
    if (s->n_games < 1 || !s->env_game || !s->env_line_stats) return (int)hipErrorInvalidValue;
    if (misaligned4(games) || misaligned4(line_stats)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_env_copy, dim3(copy_blocks(s->n_games)), dim3(GS_THREADS), 0, (hipStream_t)stream,
                       (const uint32_t*)s->env_game, (const int32_t*)s->env_line_stats, games, line_stats, s->n_games,
                       (const int32_t*)nullptr);
    return (int)hipGetLastError();
}

int tm_env_load(const tm_store* s, const uint32_t* games, const int32_t* line_stats, int32_t* fault, int32_t* n_bad, void* stream) {
    if (!s || !games || !line_stats || !fault || !n_bad) return (int)hipErrorInvalidValue;
    if (s->n_games < 1 || s->app < 1 || !s->env_game || !s->env_line_stats) return (int)hipErrorInvalidValue;
    if (misaligned4(games) || misaligned4(line_stats) || misaligned4(fault) || misaligned4(n_bad)) return (int)hipErrorInvalidValue;
    const int err = launch_check(games, line_stats, s->n_games, s->app, fault, n_bad, (hipStream_t)stream);
    if (err) return err;
    hipLaunchKernelGGL(k_env_copy, dim3(copy_blocks(s->n_games)), dim3(GS_THREADS), 0, (hipStream_t)stream, games, line_stats,
                       s->env_game, s->env_line_stats, s->n_games, (const int32_t*)n_bad);
    return (int)hipGetLastError();
}

int tm_episode_resume(int n_games, int first_id, const int32_t* move_idx, int32_t* slot_state, int32_t* counters, void* stream) {
    if (!move_idx || !slot_state || !counters || n_games < 1 || first_id < 0) return (int)hipErrorInvalidValue;
    if (misaligned4(move_idx) || misaligned4(slot_state) || misaligned4(counters)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_episode_resume, dim3((n_games + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_games, first_id, move_idx,
                       slot_state, counters);
    return (int)hipGetLastError();
}

}  // extern "C"
