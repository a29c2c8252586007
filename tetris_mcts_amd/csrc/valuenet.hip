// Value network forward for gfx950 (model/model_vv.py:13-52; Model_VV.inference 210-217).
//
// Numerics contract (shared with oracle/valuenet_oracle.c): every output element is ONE fp32 fma chain,
// acc = bias; for k ascending: acc = fma(x_k, w_k, acc), with k = ci*9 + ky*3 + kx for the convolutions and
// the flat input index for the linear layers; sigmoid through tm_exp (explicit fma polynomial).  The MFMA
// kernels (v_mfma_f32_32x32x2_f32 is exactly such a k-ordered fma chain) and the plain kernels below
// therefore produce identical bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <mutex>
#include "../../include/tetris_mcts_hip.h"

namespace tmcts_vn {

constexpr int A1 = 32 * 18 * 8, A2 = 32 * 16 * 6, A3 = 32 * 14 * 4, HID = 256;
constexpr int OFF_C1W = 0, OFF_C1B = 288, OFF_C2W = 320, OFF_C2B = 9536, OFF_C3W = 9568, OFF_C3B = 18784,
              OFF_F1W = 18816, OFF_F1B = 477568, OFF_FOW = 477824, OFF_FOB = 478336, OFF_UB = 478338, OFF_LB = 478340;

#include "net_common.h"     // f32x16, f32x4, tm_exp, lds_fence, max_dynamic_lds

// ---- reference-order plain kernels: one thread per output element ----
template <int CIN, int H, int W>
__global__ void k_conv3x3_relu(const float* __restrict__ in, int in_stride, const int8_t* __restrict__ in8,
                               const float* __restrict__ wt, const float* __restrict__ bias, float* __restrict__ out,
                               int out_stride, int n) {
    constexpr int OH = H - 2, OW = W - 2, PER = 32 * OH * OW;
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * PER) return;
    int s = t / PER, e = t - s * PER;
    int co = e / (OH * OW), p = e - co * (OH * OW), y = p / OW, x = p - y * OW;
    float acc = bias[co];
    for (int ci = 0; ci < CIN; ++ci)
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
                int ii = (ci * H + y + ky) * W + x + kx;
                float xv = in8 ? (float)in8[(size_t)s * 200 + ii] : in[(size_t)s * in_stride + ii];
                acc = fmaf(xv, wt[((co * CIN + ci) * 3 + ky) * 3 + kx], acc);
            }
    out[(size_t)s * out_stride + e] = acc > 0.0f ? acc : 0.0f;
}

__global__ void k_fc1_relu(const float* __restrict__ a3, int stride, const float* __restrict__ w,
                           const float* __restrict__ b, float* __restrict__ h, int hstride, int n) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * HID) return;
    int s = t / HID, j = t - s * HID;
    float acc = b[j];
    const float* x = a3 + (size_t)s * stride;
    const float* wr = w + (size_t)j * A3;
    for (int i = 0; i < A3; ++i) acc = fmaf(x[i], wr[i], acc);
    h[(size_t)s * hstride + j] = acc > 0.0f ? acc : 0.0f;
}

__global__ void k_fc_out(const float* __restrict__ h, int hstride, const float* __restrict__ P, float* __restrict__ v,
                         float* __restrict__ var, int n, const int32_t* __restrict__ eval_obs) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 2) return;
    int s = t >> 1, j = t & 1;
    if (eval_obs && eval_obs[s] == 0) return;   // unused evaluation slot: its outputs are never read
    float acc = P[OFF_FOB + j];
    const float* x = h + (size_t)s * hstride;
    const float* wr = P + OFF_FOW + j * HID;
    for (int i = 0; i < HID; ++i) acc = fmaf(x[i], wr[i], acc);
    double e = tm_exp(-(double)acc);
    float sg = (float)(1.0 / (1.0 + e));
    float tt = sg * P[OFF_UB + j];
    float o = tt + P[OFF_LB + j];
    if (j == 0) v[s] = o; else var[s] = o;
}

}  // namespace tmcts_vn
namespace tmcts_vn {

// ===================================================================================================
// MFMA path.  v_mfma_f32_32x32x2_f32: D[32x32] += A[32x2] * B[2x32]; lane l supplies A[i=l&31][k=l>>5] and
// B[k=l>>5][j=l&31]; lane l holds D[i=(r&3)+8*(r>>2)+4*(l>>5)][j=l&31] in register r of 16.  Per output it is
// the chain fma(a_k1,b_k1, fma(a_k0,b_k0, C)): stepping k in pairs, ascending, reproduces the reference order.
// Orientation: i = output channel / hidden unit (weights are the A operand), j = output position / state.
//
// Prepared weights ("T4" streams): for MFMA step s the A operand of lane l is W[row=l&31][k=2s+(l>>5)];
// four consecutive steps are stored together so one global_load_dwordx4 per lane feeds four MFMAs:
//   T4[(s/4)*64 + l][s%4]
// ===================================================================================================
constexpr int SCHED_REGION_QUADS = 6;   // conv_mfma closes its scheduling region every this many quads of MFMA steps
constexpr int PREP_W2 = 0, PREP_W3 = 9216, PREP_W1 = 18432, PREP_TOTAL = 18432 + 458752;
constexpr int A1CS = 145;   // conv1-output channel stride in LDS (18*8 = 144, +1 against bank conflicts)
constexpr int A2CS = 97;    // conv2-output channel stride in LDS (16*6 = 96, +1)
// Two workgroups per CU: conv2's outputs live in registers until its last LDS read of a1 has been issued, so a2 can
// take a1's place; a wave then needs 19.4 KB instead of 31.8 KB and two workgroups (8 waves) fit a CU's 160 KB: the
// vector-ALU phases of one wave (render, conv1, epilogues) run under the other wave's MFMAs (measured, r01: 118 us -> 104 us
// per launch of 4096 states).
constexpr int CONV_WG_PER_CU = 2;
constexpr int WAVE_LDS = 32 * A1CS + 200;               // floats per wave: a1 (a2 overlays it), input

__global__ void k_vn_prepare(const float* __restrict__ P, float* __restrict__ prep) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 2 * 9216) {
        const float* W = P + (t < 9216 ? OFF_C2W : OFF_C3W);
        int e = t % 9216;
        int q = e / 256, l = (e / 4) % 64, r = e % 4;
        int s = 4 * q + r;
        int k = 2 * s + (l >> 5), row = l & 31;
        prep[t] = W[row * 288 + k];
    } else if (t < PREP_TOTAL) {
        // fc1 runs on v_mfma_f32_16x16x4_f32: lane l supplies A[row = l&15][k = 4s + (l>>4)] for step s of a 16-row tile
        int e = t - 18432;
        int ht = e / (112 * 256), e2 = e % (112 * 256);
        int q = e2 / 256, l = (e2 / 4) % 64, r = e2 % 4;
        int s = 4 * q + r;
        int k = 4 * s + (l >> 4), row = 16 * ht + (l & 15);
        prep[t] = P[OFF_F1W + (size_t)row * A3 + k];
    }
}

// 3x3 valid convolution, 32 -> 32 channels, as TILES position tiles of 32 on the matrix cores.
// in: LDS activations [32][IN_CS] (rows of IN_W), boff[t][j]: this lane's LDS float offset for tile t and the
// j-th step of an 18-k (two input channel) block; W: prepared T4 stream (+lane already applied).
template <int TILES, int IN_CS>
__device__ __forceinline__ void conv_mfma(const float* __restrict__ in, const int (&boff)[TILES][9],
                                          const float4* __restrict__ W, f32x16 (&acc)[TILES]) {
    // Software pipeline: the B operands (LDS) of quad q+1 and the weights (global) of quad q+2 are requested
    // while the 4*TILES MFMAs of quad q issue; accumulators rotate so consecutive MFMAs are independent.
    float4 wq[3];
    float bb[2][4][TILES];
    auto load_b = [&](int q, int buf) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = 4 * q + r, cp = s / 9, j = s % 9;   // 18 k per pair of input channels
#pragma unroll
            for (int t = 0; t < TILES; ++t) bb[buf][r][t] = in[boff[t][j] + cp * 2 * IN_CS];
        }
    };
    wq[0] = W[0];
    wq[1] = W[64];
    load_b(0, 0);
#pragma unroll
    for (int q = 0; q < 36; ++q) {
        if (q + 2 < 36) wq[(q + 2) % 3] = W[(q + 2) * 64];
        if (q + 1 < 36) load_b(q + 1, (q + 1) & 1);
        const float4 w4 = wq[q % 3];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a = (r == 0) ? w4.x : (r == 1) ? w4.y : (r == 2) ? w4.z : w4.w;
#pragma unroll
            for (int t = 0; t < TILES; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb[q & 1][r][t], acc[t], 0, 0, 0);
        }
        // issue order inside the quad: one LDS read behind every MFMA, the weight load up front
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
#pragma unroll
        for (int i = 0; i < 4 * TILES; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        // Close the scheduling region every few quads: the group solver's cost grows steeply with the number of
        // groups in one region (all 36 quads in one region take minutes to compile).
        if (q % SCHED_REGION_QUADS == SCHED_REGION_QUADS - 1) __builtin_amdgcn_sched_barrier(0);
    }
}

// Input: either int8 states [n][200], or (states == nullptr) the evaluation requests of the tree engine's dense list (ReqList
// below): entry p = (request slot, packed observation of the slot's game, ENGINE_SPEC.md section 7), rendered here on the fly
// (0 empty, 1 locked, -1 falling piece).
constexpr int CONV_WAVES_PER_SIMD = 2;   // two workgroups per CU = two waves per SIMD: 256 registers each
// The tree engine's dense request list (include/tetris_mcts_hip.h, tm_store::eval_list): `segs` segments with one counter
// each under the current parity; entry d of segment sg is list[(sg + segs * (d / slots)) * slots + d % slots] = (request slot,
// observation index).  Dense position p counts through the segments in order.
struct ReqList {
    const int2* list;
    const int32_t* cnt;
    int parity, segs, slots;
    // the request cap (tm_store::eval_cap): a launch serves the first `cap` dense positions only (0: all of them), counted through
    // the segments cyclically from segment `rot`; block 0 of the convolution kernel writes served[s] = how many entries of
    // segment s that is (with cap == 0: the segment's count) for the tree kernel's next launch.  served == nullptr: nobody asks.
    int cap, rot;
    int32_t* served;
};
// The cap's arithmetic, host and device (tm_request_served / tm_request_at export it for tests/test_request_cap.py): the i-th
// segment of the rotated order; how many of a segment's `count` entries lie inside the first `cap` dense positions when `before`
// entries precede it in that order; where entry d of segment sg lives in the list.
__host__ __device__ constexpr int req_segment(int i, int rot, int segs) { return i + rot >= segs ? i + rot - segs : i + rot; }
__host__ __device__ constexpr int req_served(int before, int count, int cap) {
    return cap <= 0 || cap - before >= count ? count : cap - before > 0 ? cap - before : 0;
}
__host__ __device__ constexpr int req_entry(int sg, int d, int segs, int slots) { return (sg + segs * (d / slots)) * slots + d % slots; }
// lane i: inclusive prefix of the counts of the first i + 1 segments of the rotated order; total = the requests this launch serves
__device__ __forceinline__ int req_prefix(const ReqList& rq, int lane, int& total) {
    int incl = lane < rq.segs ? rq.cnt[req_segment(lane, rq.rot, rq.segs) * 2 + rq.parity] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    total = __shfl(incl, 63, 64);
    if (rq.cap > 0) total = min(total, rq.cap);
    return incl;
}
// what the launch serves of every segment, for the tree kernel (one wave of the launch calls it, every lane of the wave)
__device__ __forceinline__ void req_publish_served(const ReqList& rq, int incl, int lane) {
    const int up = __shfl_up(incl, 1, 64), before = lane > 0 ? up : 0;
    if (rq.served && lane < rq.segs) rq.served[req_segment(lane, rq.rot, rq.segs)] = req_served(before, incl - before, rq.cap);
}
// index into rq.list of dense position p (wave-uniform, p < total; every lane of the wave calls it)
__device__ __forceinline__ int req_at(const ReqList& rq, int incl, int p, int lane) {
    const int sg = __popcll(__ballot(lane < rq.segs && incl <= p));     // the first segment (rotated order) whose inclusive prefix exceeds p
    const int before = __shfl(incl, sg > 0 ? sg - 1 : 0, 64);
    const int d = p - (sg > 0 ? before : 0);
    return req_entry(req_segment(sg, rq.rot, rq.segs), d, rq.segs, rq.slots);
}
// The request-list render as functions, for k_vn_conv_x3 (valuenet_x3.inc).  k_vn_conv keeps its own inline copy of the same
// statements: calling these from it changes its machine code (measured on the code object), and the fp32 kernel stays as it is.
// lane < 12: word `lane` of the packed observation of dense request p (0 past the end; every lane of the wave calls it)
__device__ __forceinline__ uint32_t req_obs_word(const ReqList& rq, int incl, const uint32_t* __restrict__ obs_key, int max_nodes,
                                                 int n, int p, int lane) {
    if (p >= n) return 0u;
    const int2 e = rq.list[req_at(rq, incl, p, lane)];
    return lane < 12 ? obs_key[((size_t)(e.x / rq.slots) * max_nodes + e.y) * 12 + lane] : 0u;
}
// the packed observation held in lanes 0..11 of kw, rendered into x0[0..200): 0 empty, 1 locked, -1 falling piece
__device__ __forceinline__ void render_obs(uint32_t kw, int lane, float* x0) {
    const uint32_t cells = __shfl((int)kw, 10, 64), endw = __shfl((int)kw, 11, 64);
#pragma unroll
    for (int it = 0; it < 4; ++it) {   // uniform trip count: the shuffles below need every lane active
        const int i = lane + 64 * it, ic = min(i, 199);
        int r = ic / 10, c = ic - 10 * r;
        uint32_t w2 = (uint32_t)__shfl((int)kw, r >> 1, 64);
        float v = (float)((w2 >> (16 * (r & 1) + c)) & 1u);
        bool pc = ((cells & 0xFF) == (uint32_t)ic) | (((cells >> 8) & 0xFF) == (uint32_t)ic) |
                  (((cells >> 16) & 0xFF) == (uint32_t)ic) | ((cells >> 24) == (uint32_t)ic);
        if (!(endw & 0xFFu) && pc) v = -1.0f;
        if (i < 200) x0[i] = v;
    }
}
#include "valuenet_conv.inc"

// fc1 (1792 -> 256) + ReLU on v_mfma_f32_16x16x4_f32 (D[16x16] += A[16x4] B[4x16]; lane l: A[i=l&15][k=l>>4],
// B[k=l>>4][j=l&15], D[i=(l>>4)*4+r][j=l&15]; per output a k-ordered fma chain, 4 terms per instruction).
// A workgroup of 8 waves owns a tile of ROWS = 16 RT states x 256 / NY hidden units (NY workgroups per tile): wave w one
// 16-row hidden tile and NST 16-state tiles, two waves per SIMD so one wave's waits hide behind the other's MFMAs.
// Activations are staged through LDS in KC-wide K chunks (requested two chunks ahead), the B operands read from LDS a group
// of steps ahead, the weights held in a ring of WRING groups.  Two shapes, the same arithmetic and the same bits (every
// output element is its own k-ordered chain whatever the tiling):
//   <2, 4, 256, 6>  32-state tiles, four workgroups of 64 units each, 172 registers, one workgroup per CU: the single-leaf
//                   kinds, whose dense request list leaves 60-100 tiles a launch - a latency problem (r03 gave a tile two
//                   workgroups of 128 units: half of the CUs without a workgroup, 40 us whatever the number of tiles; r04 calls
//                   B-G: 51 -> 33 us);
//   <4, 4, 128, 3>  64-state tiles, four workgroups of 64 units each, two workgroups per CU: the leaf-parallel kinds' hundreds
//                   of tiles - an L2-bandwidth problem (every tile streams the 1.8 MB of weights: twice the states per tile =
//                   half the stream).  (<4, 2, 128, 3>, two workgroups of 128 units per tile, reads the activations half as
//                   often and was measured at 121 us against 80: 224 workgroups of four dependent accumulators each.)
// The output layer (256 -> 2, sigmoid, affine) is folded in: a tile's NY workgroups (parts of the hidden units) store
// their part of h with write-through (sc1) stores, wait for them, and arrive on the tile's counter; the LAST to arrive reads
// the other parts with sc1 loads (the valid hand-off form of MI355X_MICROARCH.md: 16-byte sc1 stores and loads, no fences)
// and runs the 2 x 256 fma chains of its states - the same chain, in the same order, as k_fc_out.  Nobody waits for
// anybody.  `cnt`: one int per tile (the first pad word of the scratch row of the tile's first state), zeroed by k_vn_conv at
// the start of every evaluation (the kernel also leaves it zero).
typedef float f32x4v __attribute__((ext_vector_type(4)));
// The grid is one of work ITEMS, not of tiles: an item = (tile, part) of the tiles that exist, `tiles` = ceil(requests / ROWS).
// Workgroup b of a grid of `grid` takes items b, b + grid, ...: any two workgroups' shares differ by at most one item, and the
// launch never holds more workgroups than the chip keeps resident (vn_fc1_launch), so nothing queues behind a workgroup that only
// finds out it has no work.  (Until this the grid was the request SLOTS' tiles x NY: 512 workgroups for the headline's 4096 slots,
// 236 of them with work at its 1 867 requests a launch, the other 276 dispatched in between to read the list's counters and leave.)
// The numbering of the items decides where a tile's parts run, and that is worth more than the dead workgroups (measured: parts
// 59 workgroups apart, on four different XCDs, lost 1.2 us a launch where the dead workgroups were to win one): workgroups go to the
// XCDs round robin, and a tile's NY parts read the same ROWS rows of activations - on ONE XCD they come from memory once and from
// that XCD's L2 three times.  So tiles run fastest, over the whole multiples of FC1_XCDS tiles (item i = part * t8 + tile: a tile's
// parts are t8 = 0 (mod 8) workgroups apart - one XCD, and not on neighbouring CUs at the same moment, which measured + 0.9 us),
// and the up to seven tiles left over follow, tiles fastest again.  The one formula, host and device (tm_fc1_deal exports it for
// tests/test_fc1_items.py):
constexpr int FC1_XCDS = 8;
struct Fc1Item { int tile, part; };
__host__ __device__ constexpr int fc1_item_count(int requests, int rows, int parts) {
    return requests > 0 ? (requests + rows - 1) / rows * parts : 0;
}
// k-th item of workgroup b (valid while fc1_item_index(...) < fc1_item_count(...))
__host__ __device__ constexpr int fc1_item_index(int b, int grid, int k) { return b + k * grid; }
__host__ __device__ constexpr Fc1Item fc1_item(int index, int requests, int rows, int parts) {
    const int tiles = (requests + rows - 1) / rows, t8 = tiles / FC1_XCDS * FC1_XCDS, bulk = t8 * parts;
    if (index < bulk) return Fc1Item{index % t8, index / t8};
    const int rest = tiles - t8, j = index - bulk;
    return Fc1Item{t8 + j % rest, j / rest};
}
#ifdef TM_FC1_TIMELINE   // (measurement builds, scripts/fc1_timeline.py: thread 0's s_memrealtime at the kernel's stations, in the pad words of
                         //  scratch row s0 + part)
#define FC1_STAMP(i) do { if (tid == 0 && s0 + part < n) reinterpret_cast<int*>(hout)[(size_t)(s0 + part) * hstride + HID + 1 + (i)] = (int)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FC1_STAMP(i) do { } while (0)
#endif
// (a call, not inline: inside k_vn_fc1's item loop the compiler otherwise hoists tm_exp's twenty-odd 64-bit constants out of the loop
//  and keeps them in registers through the K loop - the 64-state shape then no longer fits the 128 registers of two workgroups a CU)
__device__ __noinline__ float fc1_sigmoid(float a) {
    const double e = tm_exp(-(double)a);
    return (float)(1.0 / (1.0 + e));
}
// (waves per SIMD: four for the 64-state shape - two workgroups a CU, at most 128 registers - two for the other)
template <int RT, int NY, int KC, int WRING, int PF>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(RT == 4 ? 4 : 2))) void k_vn_fc1(const float* __restrict__ P, const float* __restrict__ prep,
                                                const float* __restrict__ a3, int a3stride, int n,
                                                float* __restrict__ hout, int hstride,
                                                ReqList rq, int32_t* __restrict__ cnt, int cnt_stride,
                                                float* __restrict__ v_out, float* __restrict__ var_out) {
    // (the shape's constants and the item loop: valuenet_fc1_body.inc, the text k_vn_conv_fc1 runs as its second phase)
#define FC1_LDS() \
    __shared__ __attribute__((aligned(16))) float bt[2][BT]; \
    __shared__ int row_slot[ROWS];        /* request mode: where row j of the tile delivers its outputs */ \
    __shared__ int last_flag; \
    __shared__ __attribute__((aligned(16))) float wo[(WO + 3) / 4 * 4]
#define FC1_ROWS() \
    const int lane = threadIdx.x & 63; \
    int incl = 0; \
    if (rq.list) { \
        incl = req_prefix(rq, lane, n); \
        n = __builtin_amdgcn_readfirstlane(n);      /* (the same in every lane: say so, or the items' tile, part and s0 are vector arithmetic) */ \
    }
#define FC1_A3_LOAD(row, k, c) (*reinterpret_cast<const float4*>(a3 + (size_t)(row) * a3stride + (k) + (c)))
#define FC1_TILE_WAIT() do { } while (0)
#include "valuenet_fc1_body.inc"
#undef FC1_LDS
#undef FC1_ROWS
#undef FC1_A3_LOAD
#undef FC1_TILE_WAIT
}

#include "valuenet_fused.inc"

#include "valuenet_x3.inc"
#include "valuenet_fc1_x3.inc"

}  // namespace tmcts_vn

using namespace tmcts_vn;

// compute units of the current device (asked once: every device of a process is the same part)
static int vn_compute_units() {
    static std::once_flag once;
    static int cus = 0;
    std::call_once(once, [&] {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
    });
    return cus;
}

// k_vn_fc1 over rows [0, n) of the scratch (request mode: n = the request slots, the kernel reads the list's length itself).
// The grid: the items there can be, and no more workgroups than stay resident at once - one a CU for the 152-register shape,
// two for the other (116 registers).
template <int RT, int NY, int KC, int WRING, int PF, int WG_PER_CU>
static int vn_fc1_launch_shape(const float* P, const float* prepared, const ReqList& rq, int n, float* v, float* var,
                               float* scratch, hipStream_t stream) {
    constexpr int SS = TM_VALUENET_SCRATCH_MFMA, ROWS = 16 * RT;
    const int cus = vn_compute_units();
    if (cus <= 0) return (int)hipErrorInvalidDevice;
    const int items = fc1_item_count(n, ROWS, NY), resident = cus * WG_PER_CU;
    hipLaunchKernelGGL((k_vn_fc1<RT, NY, KC, WRING, PF>), dim3(items < resident ? items : resident), dim3(512), 0, stream, P,
                       prepared, scratch, SS, n, scratch + A3, SS, rq, reinterpret_cast<int32_t*>(scratch + A3 + HID), ROWS * SS,
                       v, var);
    return (int)hipGetLastError();
}
static int vn_fc1_launch(const float* P, const float* prepared, const ReqList& rq, int n, float* v, float* var, float* scratch,
                         hipStream_t stream) {
    if (n >= 8192)      // (request slots: the leaf-parallel kinds' seven per game)
        return vn_fc1_launch_shape<4, 4, 128, 3, 2, 2>(P, prepared, rq, n, v, var, scratch, stream);
    return vn_fc1_launch_shape<2, 4, 256, 6, 2, 1>(P, prepared, rq, n, v, var, scratch, stream);
}

// k_vn_fc1_x3 (valuenet_fc1_x3.inc) in k_vn_fc1's place.  Two shapes, both 6 bytes x 4 096 elements of planes a buffer: tiles of 32
// states in chunks of 128 k, one workgroup a CU (the single-leaf kinds: a launch's items fit one round), and tiles of 64 states
// in chunks of 64 k, two workgroups a CU, once the 32-state tiles of n rows would be more than two rounds of the former's grid
// (n > 4 096 on 256 CUs: the leaf-parallel kinds' request slots; half the weight traffic a state).
template <int RT, int NY, int KC, int WRING, int PF, int WG_PER_CU>
static int vn_fc1_x3_launch_shape(const float* P, const __bf16* fc1_planes, const ReqList& rq, int n, float* v, float* var,
                                  float* scratch, hipStream_t stream, int cus) {
    constexpr int SS = TM_VALUENET_SCRATCH_MFMA, ROWS = 16 * RT;
    const int items = fc1_item_count(n, ROWS, NY), resident = cus * WG_PER_CU;
    hipLaunchKernelGGL((k_vn_fc1_x3<RT, NY, KC, WRING, PF>), dim3(items < resident ? items : resident), dim3(512), 0, stream, P,
                       fc1_planes, scratch, SS, n, scratch + A3, SS, rq, reinterpret_cast<int32_t*>(scratch + A3 + HID), ROWS * SS,
                       v, var);
    return (int)hipGetLastError();
}
static int vn_fc1_x3_launch(const float* P, const __bf16* fc1_planes, const ReqList& rq, int n, float* v, float* var,
                            float* scratch, hipStream_t stream) {
    const int cus = vn_compute_units();
    if (cus <= 0) return (int)hipErrorInvalidDevice;
    if (fc1_item_count(n, 32, 4) > 2 * cus)
        return vn_fc1_x3_launch_shape<4, 4, 64, 3, 2, 2>(P, fc1_planes, rq, n, v, var, scratch, stream, cus);
    return vn_fc1_x3_launch_shape<2, 4, 128, 6, 2, 1>(P, fc1_planes, rq, n, v, var, scratch, stream, cus);
}

// ---- k_vn_conv_fc1 (valuenet_fused.inc): the host side ----
#ifndef TM_FC1_TIMELINE
constexpr bool VN_FUSED_DEFAULT = true;      // what TM_VALUENET_FUSED unset means
// TM_VALUENET_FUSED (read once): 0 forces the two kernels, 1 asks for the one launch - for A/B runs and the tests, not a user feature
static bool vn_fused_wanted() {
    static std::once_flag once;
    static bool on = VN_FUSED_DEFAULT;
    std::call_once(once, [&] {
        const char* e = getenv("TM_VALUENET_FUSED");
        if (e && e[0] && !e[1] && (e[0] == '0' || e[0] == '1')) on = e[0] == '1';
    });
    return on;
}
// the launch's grid, asked once: one workgroup a CU up to 256, or 0 - the two-kernel path for good - when the LDS is refused or
// the chip does not hold that many workgroups at once (a poller must never wait for a workgroup that is not resident)
static int vn_fused_grid() {
    static std::once_flag once;
    static int grid = 0;
    std::call_once(once, [&] {
        const int cus = vn_compute_units(), lds = FUSED_LDS_FLOATS * (int)sizeof(float);
        int per_cu = 0;
        if (cus <= 0 || max_dynamic_lds<k_vn_conv_fc1>(lds) != 0) return;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_vn_conv_fc1, 512, (size_t)lds) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            return;
        }
        grid = cus < 256 ? cus : 256;
    });
    return grid;
}
// the sticky error word (mapped host memory: a poller that gave up writes it, the host reads it after any synchronisation)
static int32_t* vn_fused_err_host = nullptr;
static int32_t* vn_fused_err() {
    static std::once_flag once;
    static int32_t* dev = nullptr;
    std::call_once(once, [&] {
        void* h = nullptr;
        void* d = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocDefault) != hipSuccess) return;
        *static_cast<int32_t*>(h) = 0;
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipHostFree(h); return; }
        vn_fused_err_host = static_cast<int32_t*>(h);
        dev = static_cast<int32_t*>(d);
    });
    return dev;
}
// the case the one launch serves: fp32, request mode, the single-leaf shape
static bool vn_fused_serves(int backend, int fc1, const int8_t* states, const ReqList& rq, int n) {
    return backend == TM_VALUENET_FP32 && fc1 == TM_VALUENET_FC1_FP32 && !states && rq.list && n > 0 && n < 8192;
}
// grid 0: the launch's own grid.  `run`: the caller's proof that the launch's ready words are clear (valuenet_fused.inc) - *run is
// the list parity of the launch before this one in an unbroken run of one-launch evaluations on this scratch and stream, which
// cleared this launch's words, or -1; nullptr, -1 or the same parity again: the words are cleared here first
static int vn_fused_launch(const float* P, const float* prepared, const uint32_t* obs_key, const ReqList& rq, int max_nodes, int n,
                           float* v, float* var, float* scratch, hipStream_t stream, int grid, int32_t* run) {
    constexpr int SS = TM_VALUENET_SCRATCH_MFMA;
    const int resident = vn_fused_grid(), parity = rq.parity & 1;
    int32_t* err = vn_fused_err();
    if (resident <= 0 || !err || grid < 0 || grid > resident) return (int)hipErrorInvalidValue;
    if (!run || *run != (parity ^ 1)) {
        const int tiles = (n + 31) / 32;
        hipLaunchKernelGGL(k_vn_ready_clear, dim3((tiles + 255) / 256), dim3(256), 0, stream,
                           reinterpret_cast<int32_t*>(scratch + A3 + HID), tiles, 32 * SS, FUSED_READY_WORD + parity);
    }
    if (run) *run = parity;
    hipLaunchKernelGGL(k_vn_conv_fc1, dim3(grid > 0 ? grid : resident), dim3(512), FUSED_LDS_FLOATS * sizeof(float), stream, P,
                       prepared, obs_key, rq, max_nodes, n, scratch, SS, v, var, err);
    return (int)hipGetLastError();
}
#else
static bool vn_fused_wanted() { return false; }
static int vn_fused_grid() { return 0; }
static int32_t* vn_fused_err_host = nullptr;
static bool vn_fused_serves(int, int, const int8_t*, const ReqList&, int) { return false; }
static int vn_fused_launch(const float*, const float*, const uint32_t*, const ReqList&, int, int, float*, float*, float*, hipStream_t, int, int32_t*) {
    return (int)hipErrorInvalidValue;
}
#endif

extern "C" {

// the one check of the value net's mode: (FP32, FC1_FP32), (BF16X3, FC1_FP32), (BF16X3, FC1_BF16X3).  Host arithmetic only.
int tm_valuenet_check_mode(int backend, int fc1) {
    const bool ok = (backend == TM_VALUENET_FP32 && fc1 == TM_VALUENET_FC1_FP32) ||
                    (backend == TM_VALUENET_BF16X3 && (fc1 == TM_VALUENET_FC1_FP32 || fc1 == TM_VALUENET_FC1_BF16X3));
    return ok ? 0 : (int)hipErrorInvalidValue;
}

// the parts of `prepared` the mode names, in the buffer's order: the fp32 streams always, then the convolutions' planes, then fc1's
int tm_valuenet_prepare(const float* P, float* prepared, int backend, int fc1, void* stream_) {
    if (const int e = tm_valuenet_check_mode(backend, fc1)) return e;
    if (!prepared) return (int)hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_vn_prepare, dim3((PREP_TOTAL + 255) / 256), dim3(256), 0, stream, P, prepared);
    if (backend == TM_VALUENET_BF16X3)
        hipLaunchKernelGGL(k_vn_prepare_x3, dim3((2 * 18 * 64 * 8 + 255) / 256), dim3(256), 0, stream, P,
                           reinterpret_cast<__bf16*>(prepared + TM_VALUENET_PREPARED));
    if (fc1 == TM_VALUENET_FC1_BF16X3)
        hipLaunchKernelGGL(k_vn_prepare_fc1_x3, dim3((HID * A3 + 255) / 256), dim3(256), 0, stream, P,
                           reinterpret_cast<__bf16*>(prepared + TM_VALUENET_PREPARED + TM_VALUENET_PREPARED_X3));
    return (int)hipGetLastError();
}

// reference-order plain kernels (one thread per output); scratch: n x TM_VALUENET_SCRATCH floats
int tm_valuenet_forward_plain(const float* P, const int8_t* states, int n, float* v, float* var, float* scratch,
                              void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n <= 0) return 0;
    constexpr int SS = TM_VALUENET_SCRATCH;
    float* a1 = scratch;            // per state: a1 at 0, a2 at A1, a3 at A1+A2, h at A1+A2+A3
    const int T = 256;
    hipLaunchKernelGGL((k_conv3x3_relu<1, 20, 10>), dim3((n * A1 + T - 1) / T), dim3(T), 0, stream, (const float*)nullptr,
                       0, states, P + OFF_C1W, P + OFF_C1B, a1, SS, n);
    hipLaunchKernelGGL((k_conv3x3_relu<32, 18, 8>), dim3((n * A2 + T - 1) / T), dim3(T), 0, stream, a1, SS,
                       (const int8_t*)nullptr, P + OFF_C2W, P + OFF_C2B, a1 + A1, SS, n);
    hipLaunchKernelGGL((k_conv3x3_relu<32, 16, 6>), dim3((n * A3 + T - 1) / T), dim3(T), 0, stream, a1 + A1, SS,
                       (const int8_t*)nullptr, P + OFF_C3W, P + OFF_C3B, a1 + A1 + A2, SS, n);
    hipLaunchKernelGGL(k_fc1_relu, dim3((n * HID + T - 1) / T), dim3(T), 0, stream, a1 + A1 + A2, SS, P + OFF_F1W,
                       P + OFF_F1B, a1 + A1 + A2 + A3, SS, n);
    hipLaunchKernelGGL(k_fc_out, dim3((n * 2 + T - 1) / T), dim3(T), 0, stream, a1 + A1 + A2 + A3, SS, P, v, var, n,
                       (const int32_t*)nullptr);
    return (int)hipGetLastError();
}

// backend BF16X3: the convolutions of the split-precision backend (k_vn_conv_x3) on the planes behind prepared's streams, fc1 and
// the output layer as always - unless fc1 is FC1_BF16X3: k_vn_fc1_x3 on fc1's planes behind those
static int vn_forward_two(const float* P, const float* prepared, int backend, int fc1, const int8_t* states,
                          const uint32_t* obs_key, const ReqList& rq, int max_nodes, int n, float* v, float* var,
                          float* scratch, hipStream_t stream) {
    constexpr int SS = TM_VALUENET_SCRATCH_MFMA;
    if (backend == TM_VALUENET_BF16X3) {
        const int lds = 4 * X3_WAVE_BYTES;
        if (const int e = max_dynamic_lds<k_vn_conv_x3>(lds)) return e;
        const int blocks = (n + 3) / 4 < 256 ? (n + 3) / 4 : 256;     // one workgroup per CU, waves stride over the states
        const __bf16* planes = reinterpret_cast<const __bf16*>(prepared + TM_VALUENET_PREPARED);
        hipLaunchKernelGGL(k_vn_conv_x3, dim3(blocks), dim3(256), lds, stream, P, planes, states, obs_key, rq,
                           max_nodes, n, scratch, SS, reinterpret_cast<int32_t*>(scratch + A3 + HID), 32 * SS);
    } else {
        const int lds = 4 * WAVE_LDS * (int)sizeof(float);
        if (const int e = max_dynamic_lds<k_vn_conv>(lds)) return e;
        int blocks = (n + 3) / 4;
        if (blocks > 256 * CONV_WG_PER_CU) blocks = 256 * CONV_WG_PER_CU;   // resident workgroups, waves stride over the states
        hipLaunchKernelGGL(k_vn_conv, dim3(blocks), dim3(256), lds, stream, P, prepared, states, obs_key, rq,
                           max_nodes, n, scratch, SS, reinterpret_cast<int32_t*>(scratch + A3 + HID), 32 * SS);
    }
    if (fc1 == TM_VALUENET_FC1_BF16X3)
        return vn_fc1_x3_launch(P, reinterpret_cast<const __bf16*>(prepared + TM_VALUENET_PREPARED + TM_VALUENET_PREPARED_X3), rq, n, v, var, scratch, stream);
    return vn_fc1_launch(P, prepared, rq, n, v, var, scratch, stream);
}

static int vn_forward_impl(const float* P, const float* prepared, int backend, int fc1, const int8_t* states,
                           const uint32_t* obs_key, const ReqList& rq, int max_nodes, int n, float* v, float* var,
                           float* scratch, hipStream_t stream, int32_t* run = nullptr) {
    if (const int e = tm_valuenet_check_mode(backend, fc1)) return e;
    if (n <= 0) return 0;
    if (backend == TM_VALUENET_BF16X3 && !prepared) return (int)hipErrorInvalidValue;
    constexpr int SS = TM_VALUENET_SCRATCH_MFMA;   // a3 (1792) + hidden (256) + 16 pad words (word 0 of a tile's first row: its arrival counter)
    static_assert(SS >= A3 + HID + 1 && SS % 4 == 0, "scratch row");
    // one launch for the convolutions and fc1 where it serves (valuenet_fused.inc); the two kernels otherwise
    if (vn_fused_wanted() && vn_fused_serves(backend, fc1, states, rq, n) && vn_fused_grid() > 0)
        return vn_fused_launch(P, prepared, obs_key, rq, max_nodes, n, v, var, scratch, stream, 0, run);
    return vn_forward_two(P, prepared, backend, fc1, states, obs_key, rq, max_nodes, n, v, var, scratch, stream);
}

// matrix-core path; prepared: tm_valuenet_prepare's output for this mode or a larger one; scratch: n x TM_VALUENET_SCRATCH_MFMA floats
int tm_valuenet_forward(const float* P, const float* prepared, int backend, int fc1, const int8_t* states, int n, float* v,
                        float* var, float* scratch, void* stream_) {
    return vn_forward_impl(P, prepared, backend, fc1, states, nullptr, ReqList{nullptr, nullptr, 0, 0, 1, 0, 0, nullptr}, 0, n, v, var, scratch,
                           (hipStream_t)stream_);
}

// the tree engine's evaluation requests, rendered inside the first kernel: v/var -> s->eval_v / s->eval_var
static int vn_forward_requests(const float* P, const float* prepared, int backend, int fc1, const tm_store* s, float* scratch,
                               void* stream_, int32_t* run) {
    // the requests of the last tm_sim_step launch, drawn from its dense list (s->eval_parity = that launch's)
    // (s->eval_cap / eval_rot / eval_served: the request cap, tm_search_set_request_cap; a store without it serves every request)
    const int segs = TM_EVAL_SEGS(s->n_games);
    const bool capped = s->eval_served != nullptr;
    if (capped && (s->eval_cap < 0 || s->eval_rot < 0 || s->eval_rot >= segs)) return (int)hipErrorInvalidValue;
    const ReqList rq{reinterpret_cast<const int2*>(s->eval_list), s->eval_cnt, s->eval_parity, segs, s->eval_slots,
                     capped ? s->eval_cap : 0, capped ? s->eval_rot : 0, capped ? s->eval_served : nullptr};
    return vn_forward_impl(P, prepared, backend, fc1, nullptr, s->obs_key, rq, s->max_nodes, s->n_games * s->eval_slots,
                           s->eval_v, s->eval_var, scratch, (hipStream_t)stream_, run);
}
int tm_valuenet_forward_requests(const float* P, const float* prepared, int backend, int fc1, const tm_store* s, float* scratch,
                                 void* stream_) {
    return vn_forward_requests(P, prepared, backend, fc1, s, scratch, stream_, nullptr);
}
// the same for a caller that issues a run of evaluations (search.hip): *run = -1 before the first; the library keeps it
int tm_valuenet_forward_requests_run(const float* P, const float* prepared, int backend, int fc1, const tm_store* s, float* scratch,
                                     void* stream_, int32_t* run) {
    return vn_forward_requests(P, prepared, backend, fc1, s, scratch, stream_, run);
}

// k_vn_fc1's item dealing (host arithmetic only: callable without a GPU): the items of workgroup b of a grid of `grid` workgroups
// at `requests` requests, tiles of `rows` states in `parts` parts - (tile, part) pairs into items[0 .. 2 * cap); returns how many
// the workgroup takes (they may be more than cap), -1 on arguments that make no grid
int tm_fc1_deal(int requests, int rows, int parts, int grid, int b, int32_t* items, int cap) {
    if (requests < 0 || rows <= 0 || parts <= 0 || grid <= 0 || b < 0 || b >= grid) return -1;
    const int n_items = fc1_item_count(requests, rows, parts);
    int k = 0;
    for (int i = fc1_item_index(b, grid, 0); i < n_items; i = fc1_item_index(b, grid, ++k)) {
        const Fc1Item it = fc1_item(i, requests, rows, parts);
        if (items && k < cap) { items[2 * k] = it.tile; items[2 * k + 1] = it.part; }
    }
    return k;
}

// the count a tile's poller waits for in k_vn_conv_fc1 (host arithmetic only): the rows of tile `tile` of 32 at `requests` requests
int tm_fused_tile_rows(int requests, int tile) {
    if (requests < 0 || tile < 0) return -1;
    const int left = requests - 32 * tile;
    return left <= 0 ? 0 : left < 32 ? left : 32;
}
// tm_valuenet_forward_requests with the path named (a test entry): grid > 0: k_vn_conv_fc1 on `grid` workgroups (at most the
// resident ones), 0: on its own grid, < 0: the two kernels.  hipErrorInvalidValue where the one launch does not serve.
int tm_valuenet_forward_requests_grid(const float* P, const float* prepared, int backend, int fc1, const tm_store* s, float* scratch,
                                      void* stream_, int grid) {
    if (const int e = tm_valuenet_check_mode(backend, fc1)) return e;
    const int segs = TM_EVAL_SEGS(s->n_games);
    const bool capped = s->eval_served != nullptr;
    if (capped && (s->eval_cap < 0 || s->eval_rot < 0 || s->eval_rot >= segs)) return (int)hipErrorInvalidValue;
    const ReqList rq{reinterpret_cast<const int2*>(s->eval_list), s->eval_cnt, s->eval_parity, segs, s->eval_slots,
                     capped ? s->eval_cap : 0, capped ? s->eval_rot : 0, capped ? s->eval_served : nullptr};
    const int n = s->n_games * s->eval_slots;
    if (n <= 0) return 0;
    if (grid < 0)
        return vn_forward_two(P, prepared, backend, fc1, nullptr, s->obs_key, rq, s->max_nodes, n, s->eval_v, s->eval_var, scratch,
                              (hipStream_t)stream_);
    if (!vn_fused_serves(backend, fc1, nullptr, rq, n)) return (int)hipErrorInvalidValue;
    return vn_fused_launch(P, prepared, s->obs_key, rq, s->max_nodes, n, s->eval_v, s->eval_var, scratch, (hipStream_t)stream_, grid, nullptr);
}
// k_vn_conv_fc1's sticky error word, one a process: nonzero once a poller's bounded wait ran out in any launch of any handle or
// device (read it after a synchronisation).  reset != 0: clears it
int tm_valuenet_fused_error(int reset) {
    if (!vn_fused_err_host) return 0;
    const int e = __atomic_load_n(vn_fused_err_host, __ATOMIC_RELAXED);
    if (reset && e) __atomic_store_n(vn_fused_err_host, 0, __ATOMIC_RELAXED);
    return e;
}

// k_vn_conv's resident waves, one state each: the cap of the native loop's automatic mode (search.hip)
int tm_valuenet_resident_states(void) {
    const int cus = vn_compute_units();      // (the launch's grid stops at 256 compute units' worth of workgroups: vn_forward_impl)
    return cus > 0 ? (cus < 256 ? cus : 256) * CONV_WG_PER_CU * 4 : 0;
}
// The request cap's arithmetic (host only: callable without a GPU).  counts[segs] = the segments' entries; the launch serves the
// first min(sum, cap) dense positions (cap == 0: all) counted from segment `rot` cyclically.  tm_request_served: served[s] = the
// entries of segment s among them; returns their number, -1 on arguments that make no list.
int tm_request_served(const int32_t* counts, int segs, int rot, int cap, int32_t* served) {
    if (!counts || !served || segs <= 0 || rot < 0 || rot >= segs || cap < 0) return -1;
    int before = 0, n = 0;
    for (int i = 0; i < segs; ++i) {
        const int sg = req_segment(i, rot, segs);
        if (counts[sg] < 0) return -1;
        served[sg] = req_served(before, counts[sg], cap);
        n += served[sg];
        before += counts[sg];
    }
    return n;
}
// tm_request_at: dense position p -> out[0] = its segment, out[1] = its entry within the segment, out[2] = its index in the list of
// `slots` request slots a game; returns 0, -1 when p is not a position of the list
int tm_request_at(const int32_t* counts, int segs, int rot, int slots, int p, int32_t* out) {
    if (!counts || !out || segs <= 0 || rot < 0 || rot >= segs || slots <= 0 || p < 0) return -1;
    int incl = 0;
    for (int i = 0; i < segs; ++i) {          // the first segment of the rotated order whose inclusive prefix exceeds p
        const int sg = req_segment(i, rot, segs), before = incl;
        incl += counts[sg];
        if (incl > p) {
            out[0] = sg; out[1] = p - before; out[2] = req_entry(sg, p - before, segs, slots);
            return 0;
        }
    }
    return -1;
}

}  // extern "C"
