// One convolution wave's work (included by valuenet_conv.inc's k_vn_conv and by valuenet_fused.inc's k_vn_conv_fc1, inside the
// kernel's body): per-lane constants, then render + conv1 + conv2 + conv3 of dense positions s = wave, wave + waves, ...
// The including kernel supplies P, prep, states, obs_key, rq, max_nodes, n, a3out, a3stride, smem and three hooks:
//   CONV_WAVES             waves of a workgroup
//   CONV_A3_STORE(ptr, v)  the store of one element of the state's a3 row
//   CONV_STATE_DONE()      after a state's last store (s = its dense position)
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
#ifdef TM_FC1_TIMELINE   // (measurement builds, scripts/fc1_timeline.py: this wave's s_memrealtime at the stations of its first state, in
                         //  pad words 9.. of the state's scratch row)
    const int tl_entry = (int)__builtin_amdgcn_s_memrealtime();
#define CONV_STAMP(i) do { if (lane == 0 && s == (int)blockIdx.x * CONV_WAVES + w) reinterpret_cast<int*>(a3out)[(size_t)s * a3stride + A3 + HID + 9 + (i)] = (int)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define CONV_STAMP(i) do { } while (0)
#endif
    float* a1 = smem + w * WAVE_LDS;
    float* a2 = a1;                  // (a2 overlays a1: valuenet.hip, WAVE_LDS)
    float* x0 = a1 + 32 * A1CS;
    // ---- per-lane constants ----
    int koff2[9], koff3[9];   // offsets of k = 2j+half inside a two-channel block
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        int k = 2 * j + half, ci = k / 9, r = k - 9 * ci, ky = r / 3, kx = r - 3 * ky;
        koff2[j] = ci * A1CS + ky * 8 + kx;
        koff3[j] = ci * A2CS + ky * 6 + kx;
    }
    int boff2[3][9], boff3[2][9];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        int p = 32 * t + l31, y = p / 6, x = p - 6 * y;
#pragma unroll
        for (int j = 0; j < 9; ++j) boff2[t][j] = y * 8 + x + koff2[j];
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        int p = min(32 * t + l31, 55), y = p / 4, x = p - 4 * y;
#pragma unroll
        for (int j = 0; j < 9; ++j) boff3[t][j] = y * 6 + x + koff3[j];
    }
    float bias2[16], bias3[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        int i = (r & 3) + 8 * (r >> 2) + 4 * half;
        bias2[r] = P[OFF_C2B + i];
        bias3[r] = P[OFF_C3B + i];
    }
    float w1[5];      // conv1 weights: A operand of step st = W1[co = l31][k = 2 st + half], k = 9 is the zero pad
    int koff1[5];
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const int k = 2 * st + half;
        w1[st] = (k < 9) ? P[OFF_C1W + l31 * 9 + k] : 0.0f;
        koff1[st] = (k < 9) ? (k / 3) * 10 + (k % 3) : 0;
    }
    const float4* W2 = reinterpret_cast<const float4*>(prep + PREP_W2) + lane;
    const float4* W3 = reinterpret_cast<const float4*>(prep + PREP_W3) + lane;

    // Evaluation requests: entry s of the dense list (valuenet.hip ReqList) names a request slot and its observation; the
    // dependent global reads per state (list entry -> packed observation) are issued one state ahead, so they are in flight
    // under the previous state's convolutions instead of in front of this one's.  Row s of the scratch = dense position s.
    const int stride = gridDim.x * CONV_WAVES;
    int s = blockIdx.x * CONV_WAVES + w;
    int incl = 0;
    if (!states) incl = req_prefix(rq, lane, n);          // n = the requests this launch serves: those the last tree launch posted, up to the cap
    // the tree kernel's next launch learns from these which requests were served (a request past the cap is posted again)
    if (!states && blockIdx.x == 0 && w == 0) req_publish_served(rq, incl, lane);
    auto key_of = [&](int p) -> uint32_t {               // lane < 12: word `lane` of the packed observation of request p
        if (p >= n) return 0u;
        const int2 e = rq.list[req_at(rq, incl, p, lane)];
        return lane < 12 ? obs_key[((size_t)(e.x / rq.slots) * max_nodes + e.y) * 12 + lane] : 0u;
    };
    uint32_t kw_next = states ? 0u : key_of(s);
#ifdef TM_FC1_TIMELINE
    if (lane == 0 && s < n) reinterpret_cast<int*>(a3out)[(size_t)s * a3stride + A3 + HID + 9] = tl_entry;
#endif
    for (; s < n; s += stride) {
        CONV_STAMP(1);
        // weight streams re-read per state (an opaque zero offset defeats hoisting them into ~290 registers) so the
        // kernel fits in 256 registers and two waves share a SIMD
        int zoff = 0;
        asm volatile("" : "+s"(zoff));
        const float4* W2s = W2 + zoff;
        const float4* W3s = W3 + zoff;
        const uint32_t kw = kw_next;
        const int sn = s + stride;
        // ---- input ----
        if (states) {
            for (int i = lane; i < 200; i += 64) x0[i] = (float)states[(size_t)s * 200 + i];
        } else {
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
            // the next state's observation (in flight under this state's convolutions)
            kw_next = key_of(sn);
        }
        lds_fence();
        CONV_STAMP(2);
        // ---- conv1 (K = 9) on the matrix cores as well: 144 positions = 5 tiles (the last one half padding), 5 steps of
        // two taps; the tenth tap has weight 0, and fma(0, b, acc) returns acc unchanged for the finite b read there ----
        {
#pragma unroll 1
            for (int t = 0; t < 5; ++t) {
                const int p = 32 * t + l31, pc = min(p, 143), base = (pc >> 3) * 10 + (pc & 7);
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = P[OFF_C1B + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
                for (int st = 0; st < 5; ++st)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[st], x0[base + koff1[st]], acc, 0, 0, 0);
                if (p < 144) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int i = (r & 3) + 8 * (r >> 2) + 4 * half;
                        a1[i * A1CS + p] = acc[r] > 0.0f ? acc[r] : 0.0f;
                    }
                }
            }
        }
        lds_fence();
        CONV_STAMP(3);
        // ---- conv2: 96 positions = 3 tiles ----
        {
            f32x16 acc[3];
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = bias2[r];
            conv_mfma<3, A1CS>(a1, boff2, W2s, acc);
            lds_fence();   // a2 overlays a1: every read of a1 is complete before the first write
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    int i = (r & 3) + 8 * (r >> 2) + 4 * half;
                    float v = acc[t][r];
                    a2[i * A2CS + 32 * t + l31] = v > 0.0f ? v : 0.0f;
                }
        }
        lds_fence();
        CONV_STAMP(4);
        // ---- conv3: 56 positions = 2 tiles (the last 8 lanes of tile 1 are padding) ----
        {
            f32x16 acc[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = bias3[r];
            conv_mfma<2, A2CS>(a2, boff3, W3s, acc);
            float* dst = a3out + (size_t)s * a3stride;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                int p = 32 * t + l31;
                if (p < 56) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        int i = (r & 3) + 8 * (r >> 2) + 4 * half;
                        float v = acc[t][r];
                        CONV_A3_STORE(&dst[i * 56 + p], v > 0.0f ? v : 0.0f);
                    }
                }
            }
        }
        lds_fence();
        CONV_STAMP(5);
        CONV_STATE_DONE();
    }
