// The split-precision ("bf16x3") fc1 of the value net (included after valuenet_x3.inc at the end of valuenet.hip): the opt-in
// TM_VALUENET_FC1_BF16X3 of the TM_VALUENET_BF16X3 backend.  k_vn_fc1's inputs (a3 rows in fp32 in the TM_VALUENET_SCRATCH_MFMA
// layout, from either convolution kernel; the request list; the tiles' arrival counters) and k_vn_fc1's outputs (h by
// write-through sc1 stores into the scratch row, v / var through the folded output layer): neither convolution kernel nor the
// scratch row knows which fc1 follows.
//
// Numerics contract (DESIGN.md section 3.3; tests/test_fc1_split_precision.py keeps a numpy emulation of it):
//   * both operands of fc1, the 256 x 1 792 weights and the a3 activations, are split exactly into three bf16 planes with
//     bf16x3.h's split3: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid);
//   * the reduction over k runs in 56 steps of 32 k (v_mfma_f32_16x16x32_bf16), ascending, the accumulator initialised with the
//     bias; a step adds the six plane products with i + j <= 2 in the convolutions' order: mid*mid, lo*hi, hi*lo, mid*hi, hi*mid,
//     hi*hi (weight plane first);
//   * ReLU, then the output layer as in k_vn_fc1: one fp32 fma chain over the 256 hidden units in order, sigmoid through tm_exp;
//   * every output element is this one sequence of instructions in every shape launched: a state's v / var depend on that state
//     only - not on the batch, its position in it, the tile shape or the launch.  Not bit-equal to k_vn_fc1's fp32 chain (and
//     not claimed to be); closer to the exact product than it (tests/test_gpu_fc1_x3.py measures both against fp64).
//
// fc1's weights as bf16 planes in the A-operand order of v_mfma_f32_16x16x32_bf16: for the 16-row hidden tile ht and step s lane
// l holds W[row = 16 ht + (l & 15)][k = 32 s + 8 (l >> 4) + j] in element j of plane p at planes[((ht * 56 + s) * 3 + p) * 64 + l][j]:
// one 16-byte load per lane, plane and step, a wave's 1 KB contiguous.
constexpr int FC1X3_STEPS = A3 / 32;
static_assert(FC1X3_STEPS * 32 == A3 && 3 * HID * A3 / 2 == TM_VALUENET_PREPARED_FC1_X3, "fc1 planes buffer");

__global__ void k_vn_prepare_fc1_x3(const float* __restrict__ P, __bf16* __restrict__ planes) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;      // (ht, s, lane, j)
    if (t >= HID * A3) return;
    const int ht = t / (FC1X3_STEPS * 512), s = (t / 512) % FC1X3_STEPS, l = (t / 8) % 64, j = t % 8;
    const int row = 16 * ht + (l & 15), k = 32 * s + 8 * (l >> 4) + j;
    __bf16 h, m, lo;
    split3(P[OFF_F1W + (size_t)row * A3 + k], h, m, lo);
    __bf16* dst = planes + (size_t)((ht * FC1X3_STEPS + s) * 3) * 512 + l * 8 + j;
    dst[0] = h;
    dst[512] = m;
    dst[1024] = lo;
}

// k_vn_fc1's structure - the item grid, chunked staging with PF chunks in flight, the weight ring, the sc1 hand-off and the
// folded output layer (their reasons and measurements are written there) - with another K loop.  (The epilogue is a copy on
// purpose: shared functions change k_vn_fc1's machine code.)
//
// Staging: a chunk is ROWS rows x KC k of fp32 a3 = 512 units of eight consecutive k of one row, one a thread (ROWS * KC =
// 4 096 in both shapes): two 16-byte loads, split in registers, one 16-byte LDS store per plane.  The LDS image of a chunk is
// [step][plane][k group of 8 = l >> 4][row][8 bf16]: the B operand of a lane (state l & 15, eight consecutive k) is one
// ds_read_b128 per plane, its four 16-lane groups (MI355X: {0-3, 12-15, 20-27}, ...) fall on sixteen distinct 16-byte slots of
// the 256-byte bank row - a block of ROWS x 16 bytes is a whole number of bank rows - and the eight lanes of a ds_write_b128
// group (consecutive rows of one block) on 128 contiguous bytes.  6 bytes an element: 24 KB a buffer.
template <int RT, int NY, int KC, int WRING, int PF>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(RT == 4 ? 4 : 2))) void k_vn_fc1_x3(
    const float* __restrict__ P, const __bf16* __restrict__ wplanes, const float* __restrict__ a3, int a3stride, int n,
    float* __restrict__ hout, int hstride, ReqList rq, int32_t* __restrict__ cnt, int cnt_stride, float* __restrict__ v_out,
    float* __restrict__ var_out) {
    constexpr int ROWS = 16 * RT, HS_PITCH = HID + 4;
    constexpr int UNITS = HID / NY, HT = UNITS / 16, SG = 8 / HT, NST = RT / SG;      // as k_vn_fc1
    static_assert(HT * SG == 8 && NST * SG == RT && NST >= 1 && ROWS <= 64, "eight waves = hidden tiles x groups of state tiles; one lane per row");
    static_assert(ROWS * KC == 512 * 8 && KC % 32 == 0, "one unit of eight k a thread and chunk");
    constexpr int SPC = KC / 32, NCH = A3 / KC;       // MFMA steps per chunk, chunks
    static_assert(A3 % KC == 0 && NCH >= 2, "chunking");
    constexpr int PLANES = 3 * ROWS * KC / 2;          // floats per chunk of planes
    constexpr int BT = PLANES > (ROWS * HS_PITCH + 1) / 2 ? PLANES : (ROWS * HS_PITCH + 1) / 2;     // floats per staging buffer
    static_assert(BT % 4 == 0, "16-byte buffers");
    __shared__ __attribute__((aligned(16))) float bt[2][BT];
    __shared__ int row_slot[ROWS];
    __shared__ int last_flag;
    constexpr int WO = 2 * HID + 6;
    __shared__ __attribute__((aligned(16))) float wo[(WO + 3) / 4 * 4];
    const int lane = threadIdx.x & 63;
    int incl = 0;
    if (rq.list) {
        incl = req_prefix(rq, lane, n);
        n = __builtin_amdgcn_readfirstlane(n);
    }
    const int n_items = fc1_item_count(n, ROWS, NY);
    for (int item = fc1_item_index(blockIdx.x, gridDim.x, 0), kth = 0; item < n_items; item = fc1_item_index(blockIdx.x, gridDim.x, ++kth)) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));        // (nothing derived from it is loop-invariant for the compiler: k_vn_fc1)
    const int w = tid >> 6, lane = tid & 63, kk = lane >> 4, l15 = lane & 15;
    const Fc1Item it = fc1_item(item, n, ROWS, NY);
    const int tile = it.tile, part = it.part, s0 = tile * ROWS;
    int my_slot = 0;
    FC1_STAMP(0);
    if (rq.list) {
        if (w == 0) {
            const int p = min(s0 + (lane & (ROWS - 1)), n - 1);
            int sg = 0;
            for (int k = 0; k < rq.segs; ++k) sg += __builtin_amdgcn_readlane(incl, k) <= p ? 1 : 0;
            const int before = __shfl(incl, sg > 0 ? sg - 1 : 0, 64);
            const int d = p - (sg > 0 ? before : 0);
            my_slot = rq.list[req_entry(req_segment(sg, rq.rot, rq.segs), d, rq.segs, rq.slots)].x;
        }
    }
    const int ht = part * HT + (w % HT);             // 16-row hidden tile 0..15
    const int st0 = (w / HT) * NST;                   // this wave's first 16-state tile
    const bf16x8* W = reinterpret_cast<const bf16x8*>(wplanes) + (size_t)ht * FC1X3_STEPS * 3 * 64 + lane;
    f32x4 acc[NST];
#pragma unroll
    for (int t = 0; t < NST; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = P[OFF_F1B + 16 * ht + kk * 4 + r];
    // weights: a ring of WRING steps' three planes, the step WRING - 1 ahead requested while a step is multiplied
    bf16x8 wring[WRING][3];
    auto wload = [&](int s) {
#pragma unroll
        for (int p = 0; p < 3; ++p) wring[s % WRING][p] = W[(s * 3 + p) * 64];
    };
#pragma unroll
    for (int s = 0; s < WRING - 1; ++s) wload(s);      // (before the activations: a wave's loads return in order)
    // this thread's unit of a chunk: row u_row, step u_s, k group u_g (eight lanes = eight consecutive rows: the LDS store; the
    // four k groups of a row and step 8 lanes apart: 128 contiguous bytes of the row)
    const int u_row = (tid & 7) + 8 * ((tid >> 5) % (ROWS / 8)), u_g = (tid >> 3) & 3, u_s = (tid >> 5) / (ROWS / 8);
    float4 st[PF][2];
    auto gload = [&](int chunk) {
        const int sa = s0 + u_row;
        const float4* src = reinterpret_cast<const float4*>(a3 + (size_t)sa * a3stride + chunk * KC + 32 * u_s + 8 * u_g);
#pragma unroll
        for (int i = 0; i < 2; ++i) st[chunk % PF][i] = (sa < n) ? src[i] : make_float4(0, 0, 0, 0);
    };
    auto lstore = [&](int chunk) {
        const float4 x0 = st[chunk % PF][0], x1 = st[chunk % PF][1];
        const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        bf16x8 pl[3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 a, b, c;
            split3(x[j], a, b, c);
            pl[0][j] = a;
            pl[1][j] = b;
            pl[2][j] = c;
        }
        bf16x8* dst = reinterpret_cast<bf16x8*>(&bt[chunk & 1][0]);
#pragma unroll
        for (int p = 0; p < 3; ++p) dst[((u_s * 3 + p) * 4 + u_g) * ROWS + u_row] = pl[p];
    };
    static_assert(PF >= 2 && PF <= NCH, "chunks in flight");
    float wo_r[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < PF; ++c) gload(c);
    FC1_STAMP(1);
    lstore(0);
    __syncthreads();
    FC1_STAMP(2);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c + PF < NCH) gload(c + PF);
        if (c == NCH - 1 && tid < (WO + 3) / 4) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * tid + r < WO) wo_r[r] = P[OFF_FOW + 4 * tid + r];
        }
        // B operands: block (step, plane, kk) of the chunk's image, row 16 (st0 + t) + l15; the next step's are requested while
        // this step's MFMAs issue
        const bf16x8* b0 = reinterpret_cast<const bf16x8*>(&bt[c & 1][0]) + kk * ROWS + 16 * st0 + l15;
        bf16x8 bb[2][NST][3];
        auto load_b = [&](int s, int buf) {
#pragma unroll
            for (int t = 0; t < NST; ++t)
#pragma unroll
                for (int p = 0; p < 3; ++p) bb[buf][t][p] = b0[(s * 3 + p) * 4 * ROWS + 16 * t];
        };
        load_b(0, 0);
#pragma unroll
        for (int s = 0; s < SPC; ++s) {
            const int S = c * SPC + s;
            if (S + WRING - 1 < FC1X3_STEPS) wload(S + WRING - 1);
            if (s + 1 < SPC) load_b(s + 1, (s + 1) & 1);
            const bf16x8 ah = wring[S % WRING][0], am = wring[S % WRING][1], al = wring[S % WRING][2];
            const bf16x8 (&b)[NST][3] = bb[s & 1];
            // the six products in the convolutions' order, the state tiles interleaved (consecutive MFMAs independent)
#pragma unroll
            for (int t = 0; t < NST; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, b[t][1], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NST; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, b[t][0], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NST; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b[t][2], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NST; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, b[t][0], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NST; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b[t][1], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NST; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b[t][0], acc[t], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);      // the requests stay in the step they were written in: that far ahead of their use
        }
        if (c + 1 < NCH) lstore(c + 1);          // (requested PF - 1 chunks ago)
        __syncthreads();
        if (c == NCH - 1) FC1_STAMP(3);
    }
    // ---- from here on k_vn_fc1's epilogue: D[i = kk*4 + r][j = l15] is the 16x16x4_f32 layout ----
    const int i0 = 16 * ht + kk * 4;
    float* hs = &bt[0][0];                      // ROWS x HS_PITCH floats: the K loop is over, its staging buffers are free
    static_assert(ROWS * HS_PITCH <= 2 * BT, "hidden tile fits the staging buffers");
#pragma unroll
    for (int t = 0; t < NST; ++t) {
        f32x4v o0;
#pragma unroll
        for (int r = 0; r < 4; ++r) o0[r] = acc[t][r] > 0.f ? acc[t][r] : 0.f;
        const int row = 16 * (st0 + t) + l15;
        if (s0 + row < n) {
            float* dst = hout + (size_t)(s0 + row) * hstride + i0;
            asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(dst), "v"(o0) : "memory");
        }
        *reinterpret_cast<f32x4v*>(&hs[row * HS_PITCH + i0]) = o0;
    }
    if (rq.list && w == 0 && lane < ROWS) row_slot[lane] = my_slot;
    if (tid < (WO + 3) / 4) *reinterpret_cast<float4*>(&wo[4 * tid]) = make_float4(wo_r[0], wo_r[1], wo_r[2], wo_r[3]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    FC1_STAMP(4);
    if (tid == 0) {
        // (relaxed on purpose, as in k_vn_fc1: the sc1 stores + s_waitcnt before the arrival and the sc1 loads after it carry the
        // hand-off)
        const int old = __hip_atomic_fetch_add(&cnt[(size_t)tile * cnt_stride], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = old;
        if (old == NY - 1) __hip_atomic_store(&cnt[(size_t)tile * cnt_stride], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
    }
    __syncthreads();
    FC1_STAMP(5);
    if (last_flag == NY - 1) {
    // ---- this workgroup arrived last: the other parts of h past the caches (ROWS states x (256 - UNITS) units) ----
    {
        constexpr int OQ = (HID - UNITS) / 4, CNT = ROWS * OQ / 512;
        static_assert(ROWS * OQ % 512 == 0, "whole passes");
        f32x4v wv[CNT];
#pragma unroll
        for (int i = 0; i < CNT; ++i) {
            const int e = i * 512 + tid, row = e / OQ, c = (e % OQ) * 4;
            const int col = c < part * UNITS ? c : c + UNITS;      // skipping this workgroup's own units
            const float* src = hout + (size_t)(s0 + (s0 + row < n ? row : 0)) * hstride + col;
            asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(wv[i]) : "v"(src) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < CNT; ++i) {
            const int e = i * 512 + tid, row = e / OQ, c = (e % OQ) * 4;
            const int col = c < part * UNITS ? c : c + UNITS;
            f32x4v t = wv[i];
            asm volatile("" : "+v"(t));          // (a use the compiler cannot hoist above the wait)
            if (s0 + row < n) *reinterpret_cast<f32x4v*>(&hs[row * HS_PITCH + col]) = t;
        }
    }
    __syncthreads();
    FC1_STAMP(6);
    if (tid < 2 * ROWS) {
        // one chain per lane: state j = t >> 1, output o = t & 1; fma over the 256 hidden units in order
        const int j = tid >> 1, o = tid & 1;
        int sidx = s0 + j;
        const bool live = sidx < n;
        if (rq.list) sidx = row_slot[j];
        if (live) {
            float a = wo[2 * HID + o];
            const float4* x4 = reinterpret_cast<const float4*>(&hs[j * HS_PITCH]);
            const float4* w4 = reinterpret_cast<const float4*>(&wo[o * HID]);
#pragma unroll 8
            for (int i = 0; i < HID / 4; ++i) {
                const float4 xv = x4[i], wv = w4[i];
                a = fmaf(xv.x, wv.x, a); a = fmaf(xv.y, wv.y, a); a = fmaf(xv.z, wv.z, a); a = fmaf(xv.w, wv.w, a);
            }
            const float sg = fc1_sigmoid(a);
            const float tt = sg * wo[2 * HID + 2 + o];
            const float res = tt + wo[2 * HID + 4 + o];
            if (o == 0) v_out[sidx] = res; else var_out[sidx] = res;
        }
    }
    FC1_STAMP(7);
    }   // (arrived last)
    // a further item stages into bt[] and resolves into row_slot[]: not before the output layer above has read them
    if (fc1_item_index(blockIdx.x, gridDim.x, kth + 1) < n_items) __syncthreads();
    }   // (items)
}
