// The body of the tree kernel (included by tree.hip, once per kernel): k_sim_step<VANILLA> with CAPPED = false, k_sim_step_capped
// (VANILLA = false, CAPPED = true), the launches under a request cap (tm_store::eval_cap > 0), and k_sim_step_dist (DIST = true:
// TM_KIND_DIST, whose back and front halves are its own; the others hold none of them).  Kernels from one text rather than
// one template of both or a shared function: k_sim_step<...> keeps its name (the committed counter passes are filed under it) and,
// to the instruction, the machine code it has without the cap - a common inlined body did not (1 700 instructions more, 50 more
// scalar spills), and any change to its 45 000 instructions moves a launch by about a microsecond.
    extern __shared__ __attribute__((aligned(16))) unsigned char sim_lds[];
    WaveLds* lds = reinterpret_cast<WaveLds*>(sim_lds);
    MtLds* mt_lds = reinterpret_cast<MtLds*>(sim_lds + WPB * sizeof(WaveLds));   // WPB entries, only in the VANILLA instantiation
    // the wave index is uniform by construction: say so, and every per-game base pointer lives in scalar registers
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    // The first workgroups of the grid are collectors: each looks after the garbage collections of a range of games, in
    // slices of S.gc_slice_cycles per launch (catch-up launches pass TM_SIM_GC_FULL: to completion), beside the
    // simulation workgroups - they are dispatched first and share the CUs with them (a k_sim_step wave needs 70 registers).
    constexpr int FAM = VANILLA ? FAM_ANY : (DIST ? FAM_DIST : FAM_VALUE);      // (the store's kind is the host's to match, tm_sim_step)
    const int n_gc = gc_blocks(S);
    if ((int)blockIdx.x < n_gc) {
        // the dense request list: this launch appends under S.eval_parity; the other set of counters (the list the evaluator
        // drew from before this launch) is cleared for the next one
        if (blockIdx.x == 0 && (flags & TM_SIM_FRONT) && (int)threadIdx.x < TM_EVAL_SEGS(S.n_games))
            S.eval_cnt[(size_t)threadIdx.x * 2 + (S.eval_parity ^ 1)] = 0;
        // (a collector wave shares its SIMD with four simulation waves and is the one a blocked game waits for: it goes first)
        __builtin_amdgcn_s_setprio(3);
#ifdef TM_TIMELINE   // (measurement builds, scripts/launch_timeline.py: when this workgroup started and ended, 100 MHz ticks)
        const unsigned tl0 = (unsigned)__builtin_amdgcn_s_memrealtime();
#endif
        gc_collector_block(S, flags, n_gc, *reinterpret_cast<GcLds*>(sim_lds));
#ifdef TM_TIMELINE
        if (lane == 0 && (flags & TM_SIM_FRONT) && !(flags & TM_SIM_GC_FULL) && !S.game_list && (int)blockIdx.x + 6 * n_gc < S.n_games) {
            // collector b: the spare word 35 of game b's block (start), of game n_gc + b's (end), of game 2 n_gc + b's (the
            // launch); odd launches 3 n_gc further on
            const size_t row = (size_t)blockIdx.x + ((((unsigned)flags >> 8) & 1) ? 3 * n_gc : 0);
            if (w == 0) S.gs[row * TM_GS_DW + TM_GS_GC_RSV1] = (int)tl0;
            if (w == 0) S.gs[(row + 2 * n_gc) * TM_GS_DW + TM_GS_GC_RSV1] = (int)((unsigned)flags >> 8);
            // (the end as launch << 16 | ticks since the start, the largest over the workgroup's waves: grows from launch to launch
            // whatever the 32-bit clock does - good for 65 535 launches)
            const unsigned dt = (unsigned)__builtin_amdgcn_s_memrealtime() - tl0;
            atomicMax(reinterpret_cast<unsigned*>(S.gs + (row + n_gc) * TM_GS_DW + TM_GS_GC_RSV1), ((((unsigned)flags >> 8) & 0xFFFFu) << 16) | (dt < 0xFFFFu ? dt : 0xFFFFu));
        }
#endif
        return;
    }
    // simulation wave i takes game i, or - a launch over some of the games: the catch-up launches - game_list[i]
    const int slot = ((int)blockIdx.x - n_gc) * WPB + w;
    if (slot >= (S.game_list ? S.n_listed : S.n_games)) return;
    const int g = S.game_list ? __builtin_amdgcn_readfirstlane(S.game_list[slot]) : slot;
    GP P = game_ptrs(S, g);
    WaveLds& L = lds[w];
    int32_t* gs = P.gs();
#ifdef TM_TIMELINE
    const unsigned tl0 = (unsigned)__builtin_amdgcn_s_memrealtime();
#endif
    // The game's control block (64 words) in one coalesced load: word i in lane i, read with v_readlane.  A word is read
    // from the snapshot only before this launch writes it (the halves below write each word once, from lane 0).
    int gsv = gs[lane];
    int gc_req_word = (int)(((unsigned)flags >> 8) << 4) | GC_REQ;
    {
        // a collection requested, in progress, or completed in THIS launch: the game does not simulate (what a collector
        // workgroup of this launch writes is not ordered with this wave's reads); completed in an earlier launch: resume;
        // a speculative marking (GC_SPEC_*): the game simulates, with the write barrier once the marking is under way
        const int gcw = GSV(gsv, TM_GS_GC_PHASE), gph = gcw & 15;
        if (gph == GC_SPEC_MARK) gc_req_word = (gc_req_word & ~15) | GC_REQ_SPEC;
        else if (gph == GC_SPEC_REQ) gc_req_word = (gc_req_word & ~15) | GC_REQ_OVER;
        else if (gcw != 0) {
            if (gph != GC_DONE || (gcw >> 4) == (int)((unsigned)flags >> 8)) return;
            if (lane == 0) { gs[TM_GS_GC_PHASE] = 0; gc_active_clear(P); }
            gsv = lane == TM_GS_GC_PHASE ? 0 : gsv;       // (the snapshot's phase word is what the finish stage tests)
        }
    }
    const int pend = GSV(gsv, TM_GS_PENDING);
    if (pend == 2) {
        // the simulation suspended in its expansion: redo the expansion of its leaf, post the evaluation requests
        const int leaf = GSV(gsv, TM_GS_LEAF);
        const uint32_t self_o = P.rec()[(size_t)leaf * TM_REC_DW + TM_REC_OBS];
        const uint32_t self_sc = P.rec()[(size_t)leaf * TM_REC_DW + TM_REC_SCORE];
        wave_front_finish<VANILLA, CAPPED, FAM>(S, P, L, g, lane, leaf, 0, self_o, self_sc, gsv, gc_req_word, flags);
        return;
    }
    // The request cap.  eval_served is what the evaluator's LAST launch served, so the comparison is only right in the launch that
    // follows the evaluator launch which drew this game's request: a game in TM_PENDING_POSTED must run its wave in every launch
    // until it has backed up.  That holds because (1) a game sits launches out only while a collection of its own is under way,
    // which it enters from its expansion alone (pending 2, never 1 or TM_PENDING_POSTED; a speculative marking lets it simulate),
    // (2) a launch over some of the games (game_list) lists every game that owes, and a pending game owes (k_sims_owing), (3) the
    // collector-only launches in between run no evaluator.  Whoever lets a pending game skip a launch has to keep this.
    if (CAPPED && pend == TM_PENDING_POSTED && (flags & TM_SIM_BACKUP) &&
        GSV(gsv, TM_GS_EVAL_ENTRY) >= S.eval_served[g % TM_EVAL_SEGS(S.n_games)]) {
        // the cap left this game's request out of the evaluator's launch: nothing to back up yet.  The same (slot, observation)
        // goes on this launch's list, the game stays as it is and owes a launch (tm_sims_owing).
        if (lane == 0) {
            const int segs = TM_EVAL_SEGS(S.n_games), seg = g % segs;
            const int d = atomicAdd(&S.eval_cnt[(size_t)seg * 2 + S.eval_parity], 1), at = seg + segs * d;      // (eval_slots == 1)
            if (at < S.n_games) reinterpret_cast<int2*>(S.eval_list)[at] = make_int2(g, GSV(gsv, TM_GS_LEAF_OBS));
            else atomicOr(&gs[TM_GS_ERR], TM_ERR_EVAL_LIST);
            gs[TM_GS_EVAL_ENTRY] = d;
            gs[TM_GS_N_EVAL_DEFERRED] = GSV(gsv, TM_GS_N_EVAL_DEFERRED) + 1;
        }
        return;
    }
    const long long t0 = __builtin_readcyclecounter();
    if ((flags & TM_SIM_BACKUP) && (pend == 1 || (CAPPED && pend == TM_PENDING_POSTED))) {
        if (DIST) wave_dist_back(S, P, L, g, lane, gsv);
        else wave_sim_back(S, P, L, lane, gsv, flags);
        __threadfence_block();
    }
    const long long t1 = __builtin_readcyclecounter();
#ifndef TM_TIMELINE
    if (lane == 0) gs[TM_GS_CYC_BACK] = (int)(t1 - t0);
#endif
    // the per-move quota (tm_move_begin): games that lost launches to a collection catch up in extra launches
    if ((flags & TM_SIM_FRONT) && GSV(gsv, TM_GS_SIM_STARTED) < GSV(gsv, TM_GS_SIM_TARGET)) {
        if (DIST) wave_dist_front<VANILLA, FAM>(S, P, L, g, lane, gsv, gc_req_word, flags);
        else wave_sim_front<VANILLA, CAPPED, FAM>(S, P, L, VANILLA ? &mt_lds[w] : nullptr, g, lane, gsv, gc_req_word, flags);
    }
    else if (lane < S.eval_slots) P.eval_obs()[lane] = 0;   // nothing started: no request (the evaluator skips empty slots)
#ifdef TM_TIMELINE
    if (lane == 0 && (flags & TM_SIM_FRONT) && !(flags & TM_SIM_GC_FULL) && !S.game_list &&
        GSV(gsv, TM_GS_SIM_STARTED) < GSV(gsv, TM_GS_SIM_TARGET)) {      // (the move's regular launches: all games; a simulation was started)
        gs[TM_GS_CYC_BACK] = (int)tl0;            // (in place of the phase cycles, which nothing on the device reads)
        gs[TM_GS_CYC_SELECT] = (int)__builtin_amdgcn_s_memrealtime();
        gs[TM_GS_CYC_EXPAND] = (int)((unsigned)flags >> 8);
    }
#endif
