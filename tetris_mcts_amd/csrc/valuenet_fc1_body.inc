// fc1's shape constants and item loop (included by valuenet.hip's k_vn_fc1 and by valuenet_fused.inc's k_vn_conv_fc1, inside the
// kernel's body).  The including kernel supplies RT, NY, KC, WRING, PF, P, prep, a3stride, n, hout, hstride, rq, cnt, cnt_stride,
// v_out, var_out and four hooks:
//   FC1_LDS()            declares the LDS buffers bt[2][BT], row_slot[ROWS], last_flag, wo[(WO + 3) / 4 * 4]
//   FC1_ROWS()           declares incl (req_prefix's) and sets n to the rows there are, the same in every lane
//   FC1_A3_LOAD(row, k, c)  16 bytes of activations: floats k + c .. k + c + 3 of scratch row `row`
//   FC1_TILE_WAIT()      in front of an item's first request for activations (the weights, the biases and the rows' request
//                        slots are on their way by then)
    constexpr int ROWS = 16 * RT, PITCH = KC + 4, HS_PITCH = HID + 4;
    constexpr int UNITS = HID / NY, HT = UNITS / 16, SG = 8 / HT, NST = RT / SG;      // hidden tiles per workgroup, groups of state tiles, state tiles per wave
    static_assert(HT * SG == 8 && NST * SG == RT && NST >= 1 && ROWS <= 64, "eight waves = hidden tiles x groups of state tiles; one lane per row");
    constexpr int BT = ROWS * PITCH > (ROWS * HS_PITCH + 1) / 2 ? ROWS * PITCH : (ROWS * HS_PITCH + 1) / 2;     // floats per staging buffer
    // the output layer's operands - its 2 x 256 weights, two biases and the four affine constants, 518 consecutive parameters -
    // fetched by every workgroup under the K loop's last chunk, so that the tile's last workgroup runs its chains on LDS alone
    constexpr int WO = 2 * HID + 6;
    static_assert(OFF_FOB == OFF_FOW + 2 * HID && OFF_UB == OFF_FOB + 2 && OFF_LB == OFF_UB + 2, "the output layer's parameters are consecutive");
    FC1_LDS();
    // rows = dense positions of the request list: its length decides how many items there are (a fixed trip count from here on; a
    // workgroup past the last item leaves before it has asked the memory system for anything else)
    FC1_ROWS();
    const int n_items = fc1_item_count(n, ROWS, NY);
    for (int item = fc1_item_index(blockIdx.x, gridDim.x, 0), kth = 0; item < n_items; item = fc1_item_index(blockIdx.x, gridDim.x, ++kth)) {
    // (the thread's index behind an empty asm: nothing derived from it is loop-invariant for the compiler, which otherwise keeps
    //  some seventy registers of hoisted addresses alive across the items - 233 registers against 163 for the single-leaf shape,
    //  172 against 106 for the other, which then no longer fits two workgroups a CU)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int w = tid >> 6, lane = tid & 63, kk = lane >> 4, l15 = lane & 15;     // (`lane` shadows the one above on purpose)
    const Fc1Item it = fc1_item(item, n, ROWS, NY);
    const int tile = it.tile, part = it.part, s0 = tile * ROWS;
    int my_slot = 0;
    FC1_STAMP(0);
    if (rq.list) {
        if (w == 0) {
            // lane j resolves row j (all list entries in flight together; the slot is needed after the K loop only)
            const int p = min(s0 + (lane & (ROWS - 1)), n - 1);
            int sg = 0;
            for (int k = 0; k < rq.segs; ++k) sg += __builtin_amdgcn_readlane(incl, k) <= p ? 1 : 0;     // first segment whose inclusive prefix exceeds p
            const int before = __shfl(incl, sg > 0 ? sg - 1 : 0, 64);
            const int d = p - (sg > 0 ? before : 0);
            my_slot = rq.list[req_entry(req_segment(sg, rq.rot, rq.segs), d, rq.segs, rq.slots)].x;
        }
    }
    const int ht = part * HT + (w % HT);             // 16-row hidden tile 0..15
    const int st0 = (w / HT) * NST;                   // this wave's first 16-state tile
    const float4* W = reinterpret_cast<const float4*>(prep + PREP_W1) + (size_t)ht * 112 * 64 + lane;
    f32x4 acc[NST];
#pragma unroll
    for (int t = 0; t < NST; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = P[OFF_F1B + 16 * ht + kk * 4 + r];
    constexpr int NCH = A3 / KC;          // chunks of KC k = KC/4 MFMA steps
    // a group = GRP MFMA steps (per state tile) = GRP/4 weight quads; weights: a ring of WRING groups, the group WRING - 1 ahead
    // requested while a group is multiplied (measured, r04 calls C-E per launch of ~60 32-state tiles: chunk-deep weights without
    // the LDS pipeline 45 us, with it 35 us; a ring of three groups 45 us again - the weights need the longer lead when nothing
    // else is resident to cover it)
    constexpr int GRP = 16 / NST, QPG = GRP / 4, NGRP = KC / 4 / GRP;
    static_assert(A3 % KC == 0 && NCH >= 2 && (KC / 4) % GRP == 0, "chunking");
    float4 wring[WRING][QPG];
    auto wload = [&](int G) {          // G = chunk * NGRP + group
#pragma unroll
        for (int q = 0; q < QPG; ++q) wring[G % WRING][q] = W[((size_t)G * QPG + q) * 64];
    };
    // The first weights (and the biases above) are requested BEFORE the activations: a wave's loads return in order, and the first
    // MFMA needs both.  (Which weights is a matter of the item's part, and the item numbering needs the number of tiles: they
    // cannot go out before the request list's counters are back.  On the former grid of slots, where blockIdx.y was the part,
    // every workgroup asking before it read the counters measured 34.4 us against 31.5.)
#pragma unroll
    for (int G0 = 0; G0 < WRING - 1; ++G0) wload(G0);
    // staging: ROWS rows x KC floats per chunk, KC/4 threads per row, 16-byte pieces
    constexpr int TPR = KC / 4, RPP = 512 / TPR, NPASS = ROWS / RPP;
    const int row0 = tid / TPR, c4 = (tid % TPR) * 4;
    // The activations of chunk c + 2 are requested while chunk c is multiplied (two register sets): a tile's rows were written
    // by convolution waves all over the chip, so they come from beyond this XCD's L2, and one chunk of MFMAs (under 2 us) does
    // not cover that round trip.  (Kept as a select: a plain 16-byte copy into the array sent the whole array to scratch
    // memory - tests/test_abi.py holds every hot kernel to a private segment of 0.)
    // r06 (scripts/fc1_timeline.py, the kernel's stations in time): PF register sets = PF chunks in flight, the request for chunk
    // c + PF issued at the START of chunk c's MFMAs (until then it went out after them: one chunk of cover, not two), and the
    // first weights requested before the first activations (a wave's loads return in order).  1 867 states, entry to outputs:
    // 34.2 us before; PF = 2 / 3 / 4 / 7 (the whole tile up front): 28.9 / 29.6 / 30.2 / 32.6 - the more is asked for at once, the
    // later the first chunk is there (4.5 ... 9.4 us), and the K loop does not shorten (18 - 19 us for 12 of matrix time).
    float4 st[PF][NPASS];
    auto gload = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            const int sa = s0 + row0 + RPP * i;
            st[chunk % PF][i] = (sa < n) ? FC1_A3_LOAD(sa, chunk * KC, c4) : make_float4(0, 0, 0, 0);
        }
    };
    auto lstore = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < NPASS; ++i)
            *reinterpret_cast<float4*>(&bt[chunk & 1][(row0 + RPP * i) * PITCH + c4]) = st[chunk % PF][i];
    };
    static_assert(PF >= 2 && PF <= A3 / KC, "chunks in flight");
    float wo_r[4] = {0.f, 0.f, 0.f, 0.f};
    FC1_TILE_WAIT();
#pragma unroll
    for (int c = 0; c < PF; ++c) gload(c);
    FC1_STAMP(1);
    lstore(0);
    __syncthreads();
    FC1_STAMP(2);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c + PF < NCH) gload(c + PF);         // into the register set chunk c's staging has left (lstore(c): before the last barrier)
        if (c == NCH - 1 && tid < (WO + 3) / 4) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * tid + r < WO) wo_r[r] = P[OFF_FOW + 4 * tid + r];
        }
        const float* b0 = &bt[c & 1][(16 * st0 + l15) * PITCH + kk];
        // The B operands (LDS) of the next group of MFMA steps are requested while this group's MFMAs issue (r03 - r04 call C:
        // the compiler's own order was read, wait for it, two MFMAs, read ...: an LDS round trip per pair of MFMAs, 45 us per
        // launch whatever the number of tiles, against 12 us of matrix-core time).
        float bb[2][NST][GRP];
        auto load_b = [&](int grp, int buf) {
#pragma unroll
            for (int t = 0; t < NST; ++t)
#pragma unroll
                for (int i = 0; i < GRP; ++i) bb[buf][t][i] = b0[16 * t * PITCH + 4 * (GRP * grp + i)];
        };
        load_b(0, 0);
#pragma unroll
        for (int gq = 0; gq < NGRP; ++gq) {
            const int G = c * NGRP + gq;
            if (G + WRING - 1 < NCH * NGRP) wload(G + WRING - 1);
            if (gq + 1 < NGRP) load_b(gq + 1, (gq + 1) & 1);
#pragma unroll
            for (int i = 0; i < GRP; ++i) {
                const float4 w4 = wring[G % WRING][i / 4];
                const int r = i & 3;
                const float a = (r == 0) ? w4.x : (r == 1) ? w4.y : (r == 2) ? w4.z : w4.w;
#pragma unroll
                for (int t = 0; t < NST; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb[gq & 1][t][i], acc[t], 0, 0, 0);
            }
            // issue order inside the group: an LDS read behind every other MFMA (the reads pair up into ds_read2_b32)
#pragma unroll
            for (int i = 0; i < NST * GRP / 2; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);      // the next group's reads stay in this group's region: a whole group ahead of their use
        }
        if (c + 1 < NCH) lstore(c + 1);          // (requested PF - 1 chunks ago)
        __syncthreads();
        if (c == NCH - 1) FC1_STAMP(3);
    }
    // D[i = kk*4 + r][j = l15]: four consecutive hidden units of one state per lane -> one 16-byte write-through store,
    // and a copy into LDS (hs[state][hidden unit], the layout the output layer below reads)
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
    if (rq.list && w == 0 && lane < ROWS) row_slot[lane] = my_slot;      // (the list entry has had the whole K loop to arrive)
    if (tid < (WO + 3) / 4) *reinterpret_cast<float4*>(&wo[4 * tid]) = make_float4(wo_r[0], wo_r[1], wo_r[2], wo_r[3]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    FC1_STAMP(4);
    if (tid == 0) {
        // (relaxed on purpose: the hand-off is carried by the write-through sc1 stores + s_waitcnt before the arrival and the sc1
        // loads after it - MI355X_MICROARCH.md's measured form.  With __ATOMIC_ACQ_REL here the compiler adds buffer_wbl2 sc1 /
        // buffer_inv sc1 around the atomic: 33.4 -> 35.8 us per launch, r04; tests/test_gpu_valuenet.py holds the folded output
        // layer to the oracle's bits on every run)
        const int old = __hip_atomic_fetch_add(&cnt[(size_t)tile * cnt_stride], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = old;
        if (old == NY - 1) __hip_atomic_store(&cnt[(size_t)tile * cnt_stride], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
    }
    __syncthreads();
    FC1_STAMP(5);
    if (last_flag == NY - 1) {
    // ---- this workgroup arrived last: the other parts of h past the caches (ROWS states x (256 - UNITS) units) ----
    {
        // all of a thread's 16-byte loads in flight together, one wait (the memory clobbers keep the LDS stores behind it)
        constexpr int OQ = (HID - UNITS) / 4, CNT = ROWS * OQ / 512;      // 16-byte pieces per row of the other parts; per thread
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
        // one chain per lane: state j = t >> 1, output o = t & 1 (k_fc_out's thread t = 2 s + o); fma over the 256 hidden units
        // in order
        const int j = tid >> 1, o = tid & 1;
        int sidx = s0 + j;
        const bool live = sidx < n;
        if (rq.list) sidx = row_slot[j];          // (written by wave 0 before the barrier above)
        if (live) {
            float a = wo[2 * HID + o];
            // the same chain in the same order, its operands fetched four at a time (r06, scripts/fc1_timeline.py: this loop was
            // 4.5 us of the tile's last workgroup - a scalar LDS read and a scalar global read in front of every fma)
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
