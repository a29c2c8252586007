// k_vn_conv_fc1 (included by valuenet.hip): the convolutions and fc1 of the search's evaluation requests in ONE launch, for the
// fp32 mode in request mode at the single-leaf shape (k_vn_conv + k_vn_fc1<2, 4, 256, 6, 2> otherwise, and always as the reference).
// 512 threads, one workgroup a CU, grid min(CUs, 256): the same 2 048 convolution waves at two a SIMD, and fc1's eight-wave
// workgroup.  LDS: 8 x WAVE_LDS floats for the first phase, fc1's buffers overlaid on them for the second.
//
// Phase 1: every wave runs k_vn_conv's text (valuenet_conv_body.inc) over dense positions wave, wave + waves, ...  A state's a3 row
// is stored write-through (sc1); the wave waits for its stores and adds 1 to the READY counter of the state's tile of 32.  Nothing
// in phase 1 waits for another wave.
// Phase 2: k_vn_fc1's text (valuenet_fc1_body.inc), the same items dealt the same way over this kernel's grid.  An item's weights,
// biases and request slots are requested first; then wave 0 polls the tile's ready counter (sc1 loads, s_sleep between them) until
// it holds the tile's row count, the workgroup meets at a barrier - the one at which its last convolution wave leaves the LDS to
// fc1's buffers - and the activations are read with sc1 loads.  The hand-off is MI355X_MICROARCH.md's form "each storing wave
// adds for itself, a global_load_dword sc1 poll, a workgroup barrier between the poll and every load of the bytes"; the a3 stores
// are 4-byte sc1 stores of the convolution's epilogue.  A poller only ever waits for workgroups that are resident (the launch's
// grid never exceeds what the chip holds at once) and that never wait themselves in phase 1, its own workgroup's included: a
// workgroup reaches phase 2 only when all its waves are out of phase 1.
//
// The pad words of a tile's first scratch row (TM_VALUENET_SCRATCH_MFMA, include/tetris_mcts_hip.h): word 0 fc1's arrival counter,
// words 14 and 15 the ready counters of evaluations under list parity 0 and 1.  A launch counts in its parity's word and clears
// the other one for the next launch (the search alternates parities).  That a launch's own words are clear is for its caller to
// prove (vn_fused_launch's `run`: the launch before it in an unbroken run on this scratch had the other parity); without proof
// a 256-thread clear of them is launched first - every single call, the first launch of a move, a list evaluated twice - so
// nothing depends on what a scratch held or on its address.  LDS: 4 floats behind the convolution's, for the poller's verdict.
// The arrival counter of a tile is cleared by the wave that convolves the tile's first row, before its ready add: every arrival
// follows it.
//
// Bounded wait: a poller gives up after FUSED_WAIT_TICKS of the 100 MHz s_memrealtime counter (10 ms: two hundred launches long,
// far below any watchdog), sets the sticky error word (host memory, tm_valuenet_fused_error) and its workgroup leaves the kernel.
#ifndef TM_FC1_TIMELINE      // (the measurement builds stamp pad words 1 .. 14: they keep the two kernels)
constexpr int FUSED_READY_WORD = 14;
constexpr unsigned long long FUSED_WAIT_TICKS = 1000000ull;
constexpr int FUSED_WAVES = 8;
constexpr int FUSED_LDS_FLOATS = FUSED_WAVES * WAVE_LDS + 4;      // the convolution waves' LDS and, behind it, the poller's verdict (FC1_LDS)
#ifdef TM_FUSED_TIMELINE   // (measurement builds, scripts/fused_timeline.py: s_memrealtime at the kernel's stations, in pad words 1 .. 13 -
                           //  fc1's stations in words 1 .. 8 of scratch row s0 + part as in k_vn_fc1's TM_FC1_TIMELINE build, the launch's entry,
                           //  wave 0 at its wait, the tile seen ready and the barrier behind it in words 9 .. 12 of the same row, the end
                           //  of a convolution wave's state in word 13 of the state's row.  Write-through: the words share lines with counters.)
#define FUSED_STAMP(row, word, value) \
    __hip_atomic_store(&pad[(size_t)(row) * a3stride + (word)], (int32_t)(value), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define FUSED_NOW() __builtin_amdgcn_s_memrealtime()
#else
#define FUSED_STAMP(row, word, value) do { } while (0)
#define FUSED_NOW() 0
#endif

// ready words of `tiles` tiles under one parity (the host's clear, see above)
__global__ void k_vn_ready_clear(int32_t* __restrict__ pad, int tiles, int tile_stride, int word) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < tiles) pad[(size_t)t * tile_stride + word] = 0;
}

__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) void k_vn_conv_fc1(
        const float* __restrict__ P, const float* __restrict__ prep, const uint32_t* __restrict__ obs_key, ReqList rq, int max_nodes,
        int n, float* scr, int a3stride, float* __restrict__ v_out, float* __restrict__ var_out, int32_t* err) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int parity = rq.parity & 1, n_slots = n;
    int32_t* const pad = reinterpret_cast<int32_t*>(scr) + A3 + HID;      // pad word j of scratch row r: pad[r * a3stride + j]
    const int tl_entry = (int)FUSED_NOW();
    (void)tl_entry;
    // the next evaluation's ready counters (write-through: no line of them stays behind in this XCD's L2)
    if (blockIdx.x == 0)
        for (int t = threadIdx.x; t < (n_slots + 31) / 32; t += 512)
            __hip_atomic_store(&pad[(size_t)t * 32 * a3stride + FUSED_READY_WORD + (parity ^ 1)], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // ---- phase 1 ----
    int incl_rows, n_rows;
    {
        const int8_t* const states = nullptr;
        float* const a3out = scr;
#define CONV_WAVES FUSED_WAVES
#define CONV_A3_STORE(ptr, val) __hip_atomic_store((ptr), (val), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CONV_STATE_DONE() do { \
        if ((s & 31) == 0 && lane == 0) __hip_atomic_store(&pad[(size_t)s * a3stride], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
        if (lane == 0) \
            __hip_atomic_fetch_add(&pad[(size_t)(s & ~31) * a3stride + FUSED_READY_WORD + parity], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
        if (lane == 0) FUSED_STAMP(s, 13, FUSED_NOW()); \
    } while (0)
#include "valuenet_conv_body.inc"
#undef CONV_WAVES
#undef CONV_A3_STORE
#undef CONV_STATE_DONE
        incl_rows = incl;
        n_rows = n;
    }
    // ---- phase 2 ----
    constexpr int RT = 2, NY = 4, KC = 256, WRING = 6, PF = 2;
    float* const hout = scr + A3;
    const int hstride = a3stride, cnt_stride = 16 * RT * a3stride;
    int32_t* const cnt = pad;
    const auto a3rs = __builtin_amdgcn_make_buffer_rsrc(scr, (short)0, n_slots * a3stride * 4, 0x00020000);
#define FC1_LDS() \
    float (*bt)[BT] = reinterpret_cast<float (*)[BT]>(smem); \
    float* const wo = smem + 2 * BT; \
    int* const row_slot = reinterpret_cast<int*>(smem + 2 * BT + (WO + 3) / 4 * 4); \
    int& last_flag = *reinterpret_cast<int*>(smem + 2 * BT + (WO + 3) / 4 * 4 + ROWS); \
    /* All of the above overlays the convolution waves' LDS: none of it is written before FC1_TILE_WAIT's barrier of the workgroup's \
       first item, where the last wave leaves phase 1 (valuenet_fc1_body.inc writes bt in lstore, row_slot, last_flag and wo behind \
       the K loop).  The one word written in front of that barrier, the poller's verdict, lies behind the convolution's floats. */ \
    int& wait_failed = *reinterpret_cast<int*>(smem + FUSED_WAVES * WAVE_LDS); \
    static_assert(2 * BT + (WO + 3) / 4 * 4 + ROWS + 1 <= FUSED_WAVES * WAVE_LDS && BT % 4 == 0, "fc1's buffers fit the convolution's LDS"); \
    static_assert(FUSED_LDS_FLOATS > FUSED_WAVES * WAVE_LDS, "the poller's verdict is no convolution wave's LDS")
#define FC1_ROWS() \
    const int incl = incl_rows; \
    n = __builtin_amdgcn_readfirstlane(n_rows)
#define FC1_A3_LOAD(row, k, c) \
    __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(a3rs, ((row) * a3stride + (k) + (c)) * 4, 0, 16))      /* (16: sc1) */
#define FC1_TILE_WAIT() \
    if (w == 0) { \
        const int want = min(ROWS, n - s0); \
        const int32_t* rw = &pad[(size_t)s0 * a3stride + FUSED_READY_WORD + parity]; \
        int failed = 0; \
        if (lane == 0 && s0 + part < n) { FUSED_STAMP(s0 + part, 9, tl_entry); FUSED_STAMP(s0 + part, 10, FUSED_NOW()); } \
        if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(rw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != want) { \
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime(); \
            for (;;) { \
                __builtin_amdgcn_s_sleep(2); \
                if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(rw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == want) break; \
                if (__builtin_amdgcn_s_memrealtime() - t0 > FUSED_WAIT_TICKS) { failed = 1; break; } \
            } \
        } \
        if (lane == 0 && s0 + part < n) FUSED_STAMP(s0 + part, 11, FUSED_NOW()); \
        if (lane == 0) { \
            wait_failed = failed; \
            if (failed) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); \
        } \
    } \
    __syncthreads();      /* (every wave of the workgroup is out of phase 1 behind this barrier, not before: the LDS is fc1's from here) */ \
    if (tid == 0 && s0 + part < n) FUSED_STAMP(s0 + part, 12, FUSED_NOW()); \
    if (wait_failed) break
#ifdef TM_FUSED_TIMELINE
#undef FC1_STAMP
#define FC1_STAMP(i) do { if (tid == 0 && s0 + part < n) FUSED_STAMP(s0 + part, 1 + (i), FUSED_NOW()); } while (0)
#endif
#include "valuenet_fc1_body.inc"
#ifdef TM_FUSED_TIMELINE
#undef FC1_STAMP
#define FC1_STAMP(i) do { } while (0)
#endif
#undef FC1_LDS
#undef FC1_ROWS
#undef FC1_A3_LOAD
#undef FC1_TILE_WAIT
}
#endif
