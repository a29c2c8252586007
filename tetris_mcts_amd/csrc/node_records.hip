// Node records: the tuples the collections harvest (tree.hip, the keepmask of the harvest: packed observation, value, variance,
// visits of every freed observation with enough visits) moved out of the per-game buffers tm_store::replay_obs / replay_stat into
// ONE dense ring of 64-byte rows that is the file's row (tetris_mcts_amd/nodes.py), and back from such rows into the arrays of a
// packed fit.  A row is the harvest's own tuple, bit for bit, with the game index in the stat's spare word.
//
// tm_nodes_drain = k_nr_scan + k_nr_copy, tm_nodes_sweep = k_nr_sweep_count + k_nr_scan + k_nr_sweep_write; no atomics anywhere,
// no workgroup waits for another one: the order of the rows follows from the counts alone.
//
// k_nr_scan: ONE workgroup of 1024 threads turns the games' counts into ring rows.  Thread t owns the games [t per, (t+1) per),
// per = ceil(G / 1024): it adds their counts, the 1024 partial sums are scanned (a shuffle scan per wave, the sixteen waves' totals
// through LDS), and the thread writes offsets[g] = head + (the counts before g) for its games.  Any G >= 1 takes the same path: one
// game, fewer games than a wave, more than a workgroup has threads.  Every offset is SATURATED at ring_cap, so that
// offsets[g+1] - offsets[g] is the number of game g's rows that FIT: the writers need no other bound.  The thread that owns the
// last game advances the counters: head by what fits, lost by the rest, drains by one.  The drain reads the counts from
// replay_count (clamped to [0, replay_cap]) and clears them; the sweep reads them from offsets itself, in place (a thread reads
// its games before the workgroup's barriers and writes them after).
//
// k_nr_copy: a workgroup per (game, split); four lanes a row, one 16-byte piece each - three from replay_obs, the fourth
// replay_stat's (value, variance, visit, slot) - so a wave loads 768 + 256 contiguous bytes and stores 1 KiB contiguous bytes of the
// ring per step.  A game's rows are dealt to its NR_SPLIT workgroups 64 at a time.
//
// k_nr_sweep_count / k_nr_sweep_write: a workgroup per game walks the observation slots low_obs .. max_nodes-1 in chunks of 256 in
// ascending order; the collection's own test on the statistics word; a wave ballot and the waves' counts in LDS give a passing slot
// its rank (k_episode_advance's scheme), a lane writes its row as four 16-byte stores.  The store is only read.
//
// k_node_targets: four lanes a row again: three copy the observation's pieces, the fourth copies the value and variance bits and
// computes the weight (tm_episode_targets' four rules with the row's visit count).
//
// The harvest of a TM_KIND_DIST store (replay_dist beside replay_obs / replay_stat) has rows of its own, the node row followed by the
// 64 floats of the distribution: tm_nodes_drain_dist = k_nr_scan + k_nr_copy_dist, tm_node_dist_targets = k_node_dist_targets (the
// kernels' own comments, below the value net's).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tetris_mcts_hip.h"

namespace tmcts {

constexpr int NR_ROW_DW = TM_NODE_ROW_BYTES / 4, NR_THREADS = 256, NR_WAVES = NR_THREADS / 64;
constexpr int NR_SCAN_THREADS = 1024, NR_SCAN_WAVES = NR_SCAN_THREADS / 64;
constexpr int NR_SPLIT = 8;                        // workgroups a game in k_nr_copy
constexpr int NR_STEP_ROWS = NR_THREADS / 4;       // rows a workgroup moves per step
static_assert(NR_ROW_DW == 16 && TM_OBS_DW == 12, "a row is the observation's three 16-byte pieces and the statistics' one");

__device__ __forceinline__ int nr_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// FROM_REPLAY: counts = min(max(replay_count[g], 0), replay_cap), cleared; else counts = offsets[g], in place
template <bool FROM_REPLAY>
__global__ __launch_bounds__(NR_SCAN_THREADS) void k_nr_scan(int n_games, int replay_cap, int32_t* __restrict__ replay_count,
                                                             int ring_cap, int32_t* __restrict__ counters,
                                                             int32_t* __restrict__ offsets) {
    __shared__ long long s_wave[NR_SCAN_WAVES];
    __shared__ int s_head;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // counters[0] is read ONCE, by one thread, before the barrier, and written once, after it, by the owner of the last game:
    // no wave can see the advanced head
    if (tid == 0) s_head = nr_clamp(counters[0], 0, ring_cap);
    const int per = (n_games + NR_SCAN_THREADS - 1) / NR_SCAN_THREADS;
    const long long first = (long long)tid * per;
    const int g0 = (int)(first < n_games ? first : n_games), g1 = (int)(first + per < n_games ? first + per : n_games);
    long long mine = 0;
    for (int g = g0; g < g1; ++g) mine += FROM_REPLAY ? nr_clamp(replay_count[g], 0, replay_cap) : (offsets[g] > 0 ? offsets[g] : 0);
    // inclusive scan of the threads' sums: inside the wave, then over the waves' totals
    long long incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    long long before = incl - mine, total = 0;
#pragma unroll
    for (int w = 0; w < NR_SCAN_WAVES; ++w) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    const long long cap = ring_cap, head = s_head;
    long long at = head + before;
    for (int g = g0; g < g1; ++g) {
        const int c = FROM_REPLAY ? nr_clamp(replay_count[g], 0, replay_cap) : (offsets[g] > 0 ? offsets[g] : 0);
        offsets[g] = (int32_t)(at < cap ? at : cap);
        if (FROM_REPLAY) replay_count[g] = 0;
        at += c;
    }
    if (g1 == n_games && g0 < g1) {                // the owner of the last game (one thread: the ranges are disjoint)
        const long long end = head + total, fits = (end < cap ? end : cap) - head, rest = total - fits;
        offsets[n_games] = (int32_t)(head + fits);
        const long long lost = (long long)counters[1] + rest;
        counters[0] = (int32_t)(head + fits);
        counters[1] = (int32_t)(lost < 0x7FFFFFFFll ? lost : 0x7FFFFFFFll);
        counters[2] = counters[2] + 1;
    }
}

__global__ __launch_bounds__(NR_THREADS) void k_nr_copy(const uint4* __restrict__ replay_obs, const uint4* __restrict__ replay_stat,
                                                        int replay_cap, int ring_cap, const int32_t* __restrict__ offsets,
                                                        uint4* __restrict__ ring) {
    const int g = blockIdx.x / NR_SPLIT, split = blockIdx.x % NR_SPLIT;
    const int base = offsets[g];
    const int c = nr_clamp(offsets[g + 1] - base, 0, replay_cap);              // the rows of game g that fit (k_nr_scan saturates)
    const int piece = threadIdx.x & 3;
    const uint4* obs = replay_obs + (size_t)g * replay_cap * 3;
    const uint4* stat = replay_stat + (size_t)g * replay_cap;
    for (int i = split * NR_STEP_ROWS + (threadIdx.x >> 2); i < c; i += NR_SPLIT * NR_STEP_ROWS) {
        const long long row = (long long)base + i;
        if (row >= ring_cap) break;
        uint4 v;
        if (piece < 3) {
            v = obs[(size_t)i * 3 + piece];
        } else {
            v = stat[i];
            v.w = (uint32_t)g;
        }
        ring[(size_t)row * 4 + piece] = v;
    }
}

struct SweepArgs {
    const uint4* obs_stat;      // [G][N]
    const uint4* obs_key;       // [G][N][3]
    const int32_t* gs;
    int n_games, max_nodes, min_visits;
};

// the collection's own test (tree.hip, the keepmask of the harvest)
__device__ __forceinline__ bool nr_keep(uint32_t x, int min_visits) { return (int)x >= min_visits && !(x >> 31); }

template <bool WRITE>
__global__ __launch_bounds__(NR_THREADS) void k_nr_sweep(SweepArgs A, int ring_cap, int32_t* __restrict__ offsets,
                                                         uint4* __restrict__ ring) {
    __shared__ int s_cnt[NR_WAVES];
    const int g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int low = nr_clamp(A.gs[(size_t)g * TM_GS_DW + TM_GS_LOW_OBS], 0, A.max_nodes);
    const uint4* stat = A.obs_stat + (size_t)g * A.max_nodes;
    const uint4* key = A.obs_key + (size_t)g * A.max_nodes * 3;
    const int base = WRITE ? offsets[g] : 0, fit = WRITE ? offsets[g + 1] - base : 0;
    int done = 0;                          // passing slots in the chunks before this one (the same value in every thread)
    for (int o0 = low; o0 < A.max_nodes; o0 += NR_THREADS) {
        const int o = o0 + tid;
        uint4 st = make_uint4(0u, 0u, 0u, 0u);
        if (o < A.max_nodes) st = stat[o];
        const bool keep = o < A.max_nodes && nr_keep(st.x, A.min_visits);
        const uint64_t bal = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int r = done + __popcll(bal & ((1ull << lane) - 1ull)), chunk = 0;
#pragma unroll
        for (int w = 0; w < NR_WAVES; ++w) {
            if (w < wave) r += s_cnt[w];
            chunk += s_cnt[w];
        }
        if (WRITE && keep && r < fit && (long long)base + r < ring_cap) {
            uint4* dst = ring + ((size_t)base + r) * 4;
            const uint4* k = key + (size_t)o * 3;
            dst[0] = k[0]; dst[1] = k[1]; dst[2] = k[2];
            dst[3] = make_uint4(st.y, st.z, __float_as_uint((float)(int)st.x), (uint32_t)g);
        }
        done += chunk;
        __syncthreads();                   // s_cnt is the next chunk's
    }
    if (!WRITE && tid == 0) offsets[g] = done;
}

__global__ __launch_bounds__(NR_THREADS) void k_node_targets(const uint4* __restrict__ rows, int n_rows, int weight_mode, float eps,
                                                             uint32_t* __restrict__ obs, float* __restrict__ value,
                                                             float* __restrict__ variance, float* __restrict__ weight,
                                                             int32_t* __restrict__ fault, int obs_aligned) {
    const long long q = (long long)blockIdx.x * NR_THREADS + threadIdx.x;
    const long long r = q >> 2;
    if (r >= n_rows) return;
    const int piece = (int)(q & 3);
    const uint4 v = rows[q];
    if (piece < 3) {
        uint32_t* dst = obs + (size_t)r * TM_OBS_DW + piece * 4;
        if (obs_aligned) {
            *reinterpret_cast<uint4*>(dst) = v;
        } else {
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
        return;
    }
    const float val = __uint_as_float(v.x), var = __uint_as_float(v.y), visit = __uint_as_float(v.z);
    float w = (weight_mode >= 2) ? visit : 1.0f;
    if (weight_mode == 1 || weight_mode == 3) w = w / (var + eps);
    const bool bad = !(fabsf(val) <= 3.402823466e38f) || !(fabsf(var) <= 3.402823466e38f) || !(visit >= 1.0f);
    if (bad) { w = 0.0f; fault[0] = 1; }
    reinterpret_cast<uint32_t*>(value)[r] = v.x;
    reinterpret_cast<uint32_t*>(variance)[r] = v.y;
    weight[r] = w;
}

// ---- the distributional harvest (TM_KIND_DIST): rows of TM_NODE_DIST_ROW_BYTES = the node row + replay_dist's 64 floats ----------
constexpr int NRD_ROW_Q = TM_NODE_DIST_ROW_BYTES / 16;      // 16-byte pieces a row: 3 observation, 1 statistics, 16 distribution
constexpr int NRD_DIST_Q = TM_DIST_ROW / 4;
static_assert(TM_NODE_DIST_ROW_BYTES == TM_NODE_ROW_BYTES + 4 * TM_DIST_ROW && NRD_ROW_Q == 20 && NRD_DIST_Q == 16,
              "a dist row is the node row's four pieces and the distribution's sixteen");

// k_nr_copy_dist: a workgroup per (game, split) over the game's PIECES, not its rows: piece p of the game (row p / 20, piece
// p % 20) goes to ring piece base * 20 + p, so consecutive lanes store consecutive 16-byte pieces of the ring (a wave stores 1 KiB
// contiguous bytes per step) and read runs of 3, 1 and 16 consecutive pieces of replay_obs, replay_stat and replay_dist, each run
// following the previous row's in its array.  A game's pieces are dealt to its NR_SPLIT workgroups 256 at a time.
__global__ __launch_bounds__(NR_THREADS) void k_nr_copy_dist(const uint4* __restrict__ replay_obs, const uint4* __restrict__ replay_stat,
                                                             const uint4* __restrict__ replay_dist, int replay_cap, int ring_cap,
                                                             const int32_t* __restrict__ offsets, uint4* __restrict__ ring) {
    const int g = blockIdx.x / NR_SPLIT, split = blockIdx.x % NR_SPLIT;
    const int base = offsets[g];
    const int c = nr_clamp(offsets[g + 1] - base, 0, replay_cap);              // the rows of game g that fit (k_nr_scan saturates)
    const uint4* obs = replay_obs + (size_t)g * replay_cap * 3;
    const uint4* stat = replay_stat + (size_t)g * replay_cap;
    const uint4* dist = replay_dist + (size_t)g * replay_cap * NRD_DIST_Q;
    const long long pieces = (long long)c * NRD_ROW_Q;
    for (long long p = (long long)split * NR_THREADS + threadIdx.x; p < pieces; p += (long long)NR_SPLIT * NR_THREADS) {
        const long long i = p / NRD_ROW_Q;
        const int piece = (int)(p - i * NRD_ROW_Q);
        if ((long long)base + i >= ring_cap) break;
        uint4 v;
        if (piece < 3) {
            v = obs[(size_t)i * 3 + piece];
        } else if (piece == 3) {
            v = stat[i];
            v.w = (uint32_t)g;
        } else {
            v = dist[(size_t)i * NRD_DIST_Q + (piece - 4)];
        }
        ring[(size_t)base * NRD_ROW_Q + (size_t)p] = v;
    }
}

__device__ __forceinline__ bool nr_finite(float x) { return fabsf(x) <= 3.402823466e38f; }

// k_node_dist_targets: sixteen lanes a row (four rows a wave).  Lane l of a row loads distribution piece l (atoms 4l .. 4l+3),
// copies the atoms below `atoms` and tests all four; lanes 0 .. 2 also copy the observation's pieces, lane 3 reads the statistics.
// Two wave ballots carry the row's verdict to its lane 3 (any float at fault; any atom above 0), which writes the weight: no sum
// is formed, so the verdict does not depend on an order.
__global__ __launch_bounds__(NR_THREADS) void k_node_dist_targets(const uint4* __restrict__ rows, int n_rows, int atoms, int weight_mode,
                                                                  uint32_t* __restrict__ obs, uint32_t* __restrict__ target,
                                                                  int target_stride, float* __restrict__ weight,
                                                                  int32_t* __restrict__ fault, int obs_aligned) {
    const long long q = (long long)blockIdx.x * NR_THREADS + threadIdx.x;
    const long long r = q >> 4;
    const int l = (int)(q & 15), lane = threadIdx.x & 63;
    const bool live = r < n_rows;
    bool bad = false, pos = false;
    uint4 head = make_uint4(0u, 0u, 0u, 0u);
    if (live) {
        const uint4* row = rows + (size_t)r * NRD_ROW_Q;
        const uint4 d = row[4 + l];
        if (l < 4) head = row[l];
        const uint32_t w[4] = {d.x, d.y, d.z, d.w};
        uint32_t* dst = target + (size_t)r * target_stride;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 4 * l + j;
            const float x = __uint_as_float(w[j]);
            if (k < atoms) {
                dst[k] = w[j];
                bad |= !nr_finite(x) || x < 0.0f;
                pos |= x > 0.0f;
            } else {
                bad |= x != 0.0f;           // (a NaN included) a file recorded with more atoms than the model has
            }
        }
        if (l < 3) {
            uint32_t* o = obs + (size_t)r * TM_OBS_DW + l * 4;
            if (obs_aligned) {
                *reinterpret_cast<uint4*>(o) = head;
            } else {
                o[0] = head.x; o[1] = head.y; o[2] = head.z; o[3] = head.w;
            }
        }
    }
    const int shift = lane & ~15;
    const bool row_bad = ((__ballot(bad) >> shift) & 0xFFFFull) != 0, row_pos = ((__ballot(pos) >> shift) & 0xFFFFull) != 0;
    if (live && l == 3) {
        const float visit = __uint_as_float(head.z);
        float w = (weight_mode == 2) ? visit : 1.0f;
        if (row_bad || !row_pos || !nr_finite(visit) || !(visit >= 1.0f)) { w = 0.0f; fault[0] = 1; }
        weight[r] = w;
    }
}

}  // namespace tmcts

using namespace tmcts;

extern "C" {

static bool nr_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what the two ring calls refuse, before the first HIP call
static int check_ring(const tm_store* tree, const void* ring, int ring_cap, const int32_t* counters, const int32_t* offsets) {
    if (!tree || !ring || !counters || !offsets || ring_cap < 1) return (int)hipErrorInvalidValue;
    if (!nr_aligned16(ring)) return (int)hipErrorInvalidValue;
    if (tree->kind == TM_KIND_DIST || tree->n_games < 1) return (int)hipErrorInvalidValue;
    return 0;
}

int tm_nodes_drain(tm_store* tree, void* ring, int ring_cap, int32_t* counters, int32_t* offsets, void* stream) {
    const int rc = check_ring(tree, ring, ring_cap, counters, offsets);
    if (rc) return rc;
    if (tree->replay_cap < 1 || !tree->replay_obs || !tree->replay_stat || !tree->replay_count) return (int)hipErrorInvalidValue;
    if (!nr_aligned16(tree->replay_obs) || !nr_aligned16(tree->replay_stat)) return (int)hipErrorInvalidValue;   // read as uint4
    if ((long long)tree->n_games * NR_SPLIT > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_nr_scan<true>, dim3(1), dim3(NR_SCAN_THREADS), 0, (hipStream_t)stream, tree->n_games, tree->replay_cap,
                       tree->replay_count, ring_cap, counters, offsets);
    hipLaunchKernelGGL(k_nr_copy, dim3(tree->n_games * NR_SPLIT), dim3(NR_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint4*>(tree->replay_obs), reinterpret_cast<const uint4*>(tree->replay_stat),
                       tree->replay_cap, ring_cap, offsets, reinterpret_cast<uint4*>(ring));
    return (int)hipGetLastError();
}

int tm_nodes_sweep(const tm_store* tree, void* ring, int ring_cap, int32_t* counters, int32_t* offsets, void* stream) {
    const int rc = check_ring(tree, ring, ring_cap, counters, offsets);
    if (rc) return rc;
    if (tree->max_nodes < 1 || !tree->obs_stat || !tree->obs_key || !tree->gs) return (int)hipErrorInvalidValue;
    if (!nr_aligned16(tree->obs_stat) || !nr_aligned16(tree->obs_key)) return (int)hipErrorInvalidValue;          // read as uint4
    SweepArgs A;
    A.obs_stat = reinterpret_cast<const uint4*>(tree->obs_stat);
    A.obs_key = reinterpret_cast<const uint4*>(tree->obs_key);
    A.gs = tree->gs;
    A.n_games = tree->n_games;
    A.max_nodes = tree->max_nodes;
    A.min_visits = tree->min_visits_to_store > 1 ? tree->min_visits_to_store : 1;      // a count of at least 1 always
    hipLaunchKernelGGL(k_nr_sweep<false>, dim3(A.n_games), dim3(NR_THREADS), 0, (hipStream_t)stream, A, ring_cap, offsets,
                       reinterpret_cast<uint4*>(ring));
    hipLaunchKernelGGL(k_nr_scan<false>, dim3(1), dim3(NR_SCAN_THREADS), 0, (hipStream_t)stream, A.n_games, 0,
                       static_cast<int32_t*>(nullptr), ring_cap, counters, offsets);
    hipLaunchKernelGGL(k_nr_sweep<true>, dim3(A.n_games), dim3(NR_THREADS), 0, (hipStream_t)stream, A, ring_cap, offsets,
                       reinterpret_cast<uint4*>(ring));
    return (int)hipGetLastError();
}

int tm_node_targets(const void* rows, int n_rows, int weight_mode, float eps, uint32_t* obs, float* value, float* variance,
                    float* weight, int32_t* fault, void* stream) {
    if (n_rows < 0 || weight_mode < 0 || weight_mode > 3) return (int)hipErrorInvalidValue;
    if (!rows || !obs || !value || !variance || !weight || !fault) return (int)hipErrorInvalidValue;
    if (!nr_aligned16(rows) || (reinterpret_cast<uintptr_t>(obs) & 3) != 0) return (int)hipErrorInvalidValue;
    if (n_rows > 0x7FFFFFFF / 4) return (int)hipErrorInvalidValue;                           // four lanes a row on a 32-bit grid
    if (n_rows == 0) return 0;
    const long long pieces = (long long)n_rows * 4;
    hipLaunchKernelGGL(k_node_targets, dim3((unsigned)((pieces + NR_THREADS - 1) / NR_THREADS)), dim3(NR_THREADS), 0,
                       (hipStream_t)stream, reinterpret_cast<const uint4*>(rows), n_rows, weight_mode, eps, obs, value, variance,
                       weight, fault, nr_aligned16(obs) ? 1 : 0);
    return (int)hipGetLastError();
}

int tm_nodes_drain_dist(tm_store* tree, void* ring, int ring_cap, int32_t* counters, int32_t* offsets, void* stream) {
    if (!tree || !ring || !counters || !offsets || ring_cap < 1) return (int)hipErrorInvalidValue;
    if (!nr_aligned16(ring)) return (int)hipErrorInvalidValue;
    if (tree->kind != TM_KIND_DIST || tree->n_games < 1 || tree->replay_cap < 1) return (int)hipErrorInvalidValue;
    if (!tree->replay_obs || !tree->replay_stat || !tree->replay_count || !tree->replay_dist) return (int)hipErrorInvalidValue;
    if (!nr_aligned16(tree->replay_obs) || !nr_aligned16(tree->replay_stat) || !nr_aligned16(tree->replay_dist))
        return (int)hipErrorInvalidValue;                                                    // read as uint4
    if ((long long)tree->n_games * NR_SPLIT > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_nr_scan<true>, dim3(1), dim3(NR_SCAN_THREADS), 0, (hipStream_t)stream, tree->n_games, tree->replay_cap,
                       tree->replay_count, ring_cap, counters, offsets);
    hipLaunchKernelGGL(k_nr_copy_dist, dim3(tree->n_games * NR_SPLIT), dim3(NR_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint4*>(tree->replay_obs), reinterpret_cast<const uint4*>(tree->replay_stat),
                       reinterpret_cast<const uint4*>(tree->replay_dist), tree->replay_cap, ring_cap, offsets,
                       reinterpret_cast<uint4*>(ring));
    return (int)hipGetLastError();
}

int tm_node_dist_targets(const void* rows, int n_rows, int atoms, int weight_mode, uint32_t* obs, float* target, int target_stride,
                         float* weight, int32_t* fault, void* stream) {
    if (n_rows < 0 || n_rows > 0x7FFFFFFF / 4 || atoms < 1 || atoms > TM_DIST_ROW || target_stride < atoms)
        return (int)hipErrorInvalidValue;
    if (weight_mode != 0 && weight_mode != 2) return (int)hipErrorInvalidValue;             // 1 and 3 divide by a variance the row lacks
    if (!rows || !obs || !target || !weight || !fault) return (int)hipErrorInvalidValue;
    if (!nr_aligned16(rows)) return (int)hipErrorInvalidValue;
    if (((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(weight)) & 3) != 0)
        return (int)hipErrorInvalidValue;
    if (n_rows == 0) return 0;
    const long long lanes = (long long)n_rows * NRD_DIST_Q;                                  // sixteen lanes a row: at most 2^25 workgroups
    hipLaunchKernelGGL(k_node_dist_targets, dim3((unsigned)((lanes + NR_THREADS - 1) / NR_THREADS)), dim3(NR_THREADS), 0,
                       (hipStream_t)stream, reinterpret_cast<const uint4*>(rows), n_rows, atoms, weight_mode, obs,
                       reinterpret_cast<uint32_t*>(target), target_stride, weight, fault, nr_aligned16(obs) ? 1 : 0);
    return (int)hipGetLastError();
}

}  // extern "C"
