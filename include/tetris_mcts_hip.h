/*
 * tetris_mcts_hip.h — C ABI of libtetris_mcts_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the reference's hot path:
 *   - environment step            : pyTetris `Tetris.play/copy_from/getState/reset`
 *                                   (call sites play.py:150,165; agents/agent.py:101-129,140-145)
 *   - tree agent (select/expand/backup, transposition + observation tables)
 *                                 : agents/cppmodule/agent.cpp TreeAgent/MCTSAgent (agent.cpp:84-568) and the
 *                                   Python twins agents/agent.py:90-193, ValueSim.py:52-99, ValueSimLP.py:13-70
 *   - the five `agents.cppmodule.core` functions (core.cpp:20-26) in batched form over device arrays
 *   - leaf evaluator              : model/model_vv.py:13-52,210-217
 * All pointers are DEVICE pointers unless named host_*.  Every function enqueues work on `stream`
 * (a hipStream_t passed as void*) and returns a hipError_t value (0 = success); nothing synchronises.
 * No torch types cross this boundary.  One process drives one GPU; games shard across processes.
 */
#ifndef TETRIS_MCTS_HIP_H
#define TETRIS_MCTS_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TM_NACT 7
#define TM_GAME_DW 16      /* packed game, ENGINE_SPEC.md section 2 (64 bytes) */
#define TM_OBS_DW 12       /* packed observation, ENGINE_SPEC.md section 7 (48 bytes) */
#define TM_REC_DW 32       /* node record (128 bytes = one cache line): eight 16-byte pieces.  Pieces 0..6 = the node's unique
                              children in selection order: (child, obs, child score bits, own score bits); piece 7 =
                              (TM_REC_PCHILD, TM_REC_OBS, TM_REC_SCORE, TM_REC_HDR); see DESIGN.md "node store" */
#define TM_REC_PCHILD 28   /* the child the last walk through this node descended into (0: none yet): the walk prefetches it */
#define TM_REC_OBS 29      /* node_to_obs */
#define TM_REC_SCORE 30    /* float32 score of the node's game */
#define TM_REC_HDR 31      /* bits 0-2 number of unique children, bit 24 game ended, bit 25 expanded */
#define TM_KIDS_DW 8       /* raw children row: child[7] in action order + the node's observation */
#define TM_GS_DW 64        /* per-game control block */
#define TM_LEAF_DW 32      /* per-game leaf hand-off between the front and back halves of a simulation */
#define TM_DIST_ROW 64       /* floats per row of node_dist / eval_dist (dist_bins <= 64 atoms, zero padded) */
#define TM_GC_PART_DW 192   /* per-game scratch of a collection: (free nodes, free observations, harvested tuples) per collector workgroup */
#define TM_VALUENET_PARAMS 478342
#define TM_VALUENET_SCRATCH 9728       /* floats of scratch per state, tm_valuenet_forward_plain */
#define TM_VALUENET_SCRATCH_MFMA 2064  /* floats of scratch per state, tm_valuenet_forward / _requests in every mode; no initial contents
                                          required (the kernels keep a counter per tile of 32 or 64 states in the rows' padding: every
                                          evaluation clears them first).  The 16 pad words of a tile's first row: word 0 fc1's arrival
                                          counter; words 14 and 15 k_vn_conv_fc1's ready counters of evaluations under list parity 0
                                          and 1 (a launch clears the other parity's; the library clears a launch's own first unless the caller
                                          proves that the launch before it did: tm_valuenet_forward_requests_run); words
                                          1 .. 14 the measurement builds' time stamps (TM_FC1_TIMELINE: they keep the two kernels) */
/* the parts of tm_valuenet_prepare's buffer, in its order */
#define TM_VALUENET_PREPARED 477184    /* floats: conv2 + conv3 + fc1 operand streams (every mode) */
#define TM_VALUENET_PREPARED_X3 27648  /* floats (55 296 bf16): conv2 + conv3 weights as bf16 hi / mid / lo planes (TM_VALUENET_BF16X3) */
#define TM_VALUENET_PREPARED_FC1_X3 688128  /* floats (1 376 256 bf16 = 3 x 256 x 1 792): fc1's weights as bf16 hi / mid / lo planes
                                          (TM_VALUENET_FC1_BF16X3) */
/* evaluator backends (the value net's and the distributional head's `backend` argument, tm_search_set_valuenet) */
#define TM_VALUENET_FP32 0             /* fp32 matrix cores, the oracle's bits (the default) */
#define TM_VALUENET_BF16X3 1           /* the convolutions after the first as three-way bf16 splits, fp32 accumulation */
/* fc1 of the value net (its `fc1` argument); TM_VALUENET_FC1_BF16X3 goes with TM_VALUENET_BF16X3 only */
#define TM_VALUENET_FC1_FP32 0         /* k_vn_fc1: the fp32 fma chain (the default) */
#define TM_VALUENET_FC1_BF16X3 1       /* k_vn_fc1_x3: fc1 as a three-way bf16 split as well */
/* floats of the prepared buffer of a mode */
#define TM_VALUENET_PREPARED_TOTAL(backend, fc1) (TM_VALUENET_PREPARED + ((backend) == TM_VALUENET_BF16X3 ? TM_VALUENET_PREPARED_X3 : 0) + \
                                                  ((fc1) == TM_VALUENET_FC1_BF16X3 ? TM_VALUENET_PREPARED_FC1_X3 : 0))
#define TM_DISTNET_PREPARED_TOTAL(backend) (TM_DISTNET_PREPARED + ((backend) == TM_VALUENET_BF16X3 ? TM_DISTNET_PREPARED_X3 : 0))
#define TM_DISTNET_PARAMS(atoms) (279232 + 129 * (atoms))  /* floats: conv1.w[32][1][4][4] conv1.b[32] conv2.w[32][32][4][4] conv2.b[32]
                                          fc1.w[128][2048] fc1.b[128] fc_v.w[atoms][128] fc_v.b[atoms] (model/model_distributional.py:33-42) */
#define TM_DISTNET_PARAMS_50 285682    /* TM_DISTNET_PARAMS(50) */
#define TM_DISTNET_PREPARED 278528     /* floats: conv2 + fc1 operand streams (every backend) */
#define TM_DISTNET_PREPARED_X3 24576   /* floats (49 152 bf16): conv2's weights as bf16 hi / mid / lo planes (TM_VALUENET_BF16X3) */
#define TM_DISTNET_SCRATCH 2048        /* floats of scratch per state (conv2's output), tm_distnet_forward / _requests */

/* per-game control block (int32 words) */
enum {
    TM_GS_ROOT = 0, TM_GS_EPISODE, TM_GS_NFREE_NODE, TM_GS_NFREE_OBS, TM_GS_TRACE_LEN, TM_GS_PENDING,
    TM_GS_ERR, TM_GS_N_EXPAND, TM_GS_N_SIMS, TM_GS_N_GC, TM_GS_RNG_POS, TM_GS_N_NQ_FALLBACK,
    TM_GS_LEAF, TM_GS_LEAF_END, TM_GS_K_EVAL, TM_GS_LEAF_SCORE,
    TM_GS_TRACE_SUM, /* sum of trace lengths over all simulations (for bytes/simulation accounting) */
    TM_GS_N_EVAL,    /* leaf states handed to the evaluator (requests posted) */
    TM_GS_N_POOL_RESET, /* tm_pool_reset calls that hit this game */
    TM_GS_MAX_TRACE,    /* longest trace of any simulation so far */
    TM_GS_CYC_BACK = 20, TM_GS_CYC_SELECT, TM_GS_CYC_EXPAND, /* shader cycles of the last simulation's phases */
    TM_GS_CYC_TAIL,      /* duration of the last GC in units of 16 cycles; +1: nodes reachable at that GC */
    TM_GS_N_DROPPED = 25, /* replay tuples a GC could not store because the harvest buffer was full (drain it more often) */
    TM_GS_LOW_NODE = 26, TM_GS_LOW_OBS,  /* lowest node / observation index ever allocated (GC skips untouched entries) */
    TM_GS_FIRST_MISS = 28, /* levels of the last walk that were taken over from the walk before it (verified in parallel, tree.hip) */
    TM_GS_PREFIX_SUM,      /* sum of TM_GS_FIRST_MISS over all simulations */
    TM_GS_EVAL_ENTRY,      /* under a request cap (tm_store::eval_cap), TM_GS_PENDING == TM_PENDING_POSTED: the pending request's entry
                              within its segment of the dense list, held against eval_served by the next launch */
    TM_GS_N_EVAL_DEFERRED, /* requests posted again because the evaluator's launch left them out (TM_GS_N_EVAL counts a request once,
                              when it is first posted) */
    /* garbage collection by the collector workgroups of tm_sim_step (a game that collects does not simulate; tree.hip) */
    TM_GS_GC_PHASE = 32, /* 0 none; (launch << 4) | 1 requested; 2 marking, 3 counting + re-inserting the kept nodes, 4 writing the free
                            lists + re-inserting the kept observations; (launch << 4) | 7 complete (the game resumes in a later
                            launch); speculative marking while the game simulates: (launch << 4) | 8 requested, 9 under way,
                            (launch << 4) | 10 the pool ran dry meanwhile */
    TM_GS_GC_ARRIVE,     /* collector workgroups that have done their share of the current step (bits 8..: some left work) */
    TM_GS_GC_ACTIVE4,    /* in the control block of every FOURTH game (game 4k of the store or slice - slices begin at multiples of four
                            games): bit j = game 4k + j's phase word may be non-zero.  The collector workgroups of a launch look at
                            these words and read the phase words they point at, instead of every game's (set with the request by the
                            game's wave, cleared by it when it resumes; a bit without a phase is harmless, a phase without its bit
                            would never be served) */
    TM_GS_GC_RSV1,       /* (unused) */
    TM_GS_GC_WORK,       /* marking: chunks were flagged when the last launch that looked ended (the next one marks) */
    TM_GS_GC_MARK_LAUNCHES, /* launches in which a collector workgroup marked for this game (all collections) */
    TM_GS_GC_SLICES,     /* launches in which collector workgroups worked on a collection of this game (all collections) */
    TM_GS_GC_RETRY,      /* the suspended expansion has already been through a collection */
    /* per-move simulation quota: tm_move_begin adds `sims` to the target; a launch starts a simulation for a game only
       while started < target, so games that lost launches to a collection catch up in extra launches (tm_sims_remaining) */
    TM_GS_SIM_TARGET = 40, TM_GS_SIM_STARTED,
    TM_GS_CYC_VERIFY,    /* shader cycles of the last walk's parallel prefix verification (part of TM_GS_CYC_SELECT) */
    TM_GS_N_WALK_MISS,   /* tree levels at which the walk descended into another child than the predicted one (all simulations) */
    TM_GS_POOL_FULL,     /* the reachable tree fills the pool (TM_ERR_POOL): no collection is attempted until the root moves */
    TM_GS_GC_IN_MOVE,    /* a collection has completed since the root last moved: until it moves again nothing becomes unreachable
                            (the search only adds links), so the next exhaustion is counted as the reference's collection that
                            frees nothing (agents/agent.py:96-97) and goes straight to TM_GS_POOL_FULL */
    TM_GS_GC_REQ_AT,     /* the launch in which the game asked for the collection it is waiting for (the waiting games' steps that
                            do not all fit a launch are served oldest request first) */
    TM_GS_LEAF_OBS,      /* the pending leaf's observation (TM_SIM_EVAL_NEEDED: where the backup files the evaluator's output) */
    TM_GS_N_EVAL_SKIP,   /* leaf-parallel kinds: unique children of expanded leaves whose evaluation the backup would discard
                            (observation already visited / finished) - not posted under TM_SIM_EVAL_NEEDED, counted always */
    TM_GS_N_EVAL_CACHED, /* TM_KIND_VALUESIM / TM_KIND_CPPAGENT under TM_SIM_EVAL_NEEDED: leaves answered from obs_eval */
    TM_GS_GC_NGC,        /* collector workgroups of the launch that began the collection under way (its shares are cut for that many) */
    TM_GS_GC_BLOCKS,     /* the marker's work, all collections: blocks of child rows loaded (tree.hip GC_BLOCK_NODES nodes each), */
    TM_GS_GC_ITERS,      /* ... rounds of its block-local marking (one workgroup barrier each), */
    TM_GS_GC_MARK_CYC,   /* ... shader cycles / 64 it was at it (summed over its workgroups) */
    TM_GS_GC_FLAGS       /* 4 words = 128 flags, the marking's work list: chunks of the index range (tree.hip gc_chunk_log2) that hold
                            pending nodes - marked, children not looked at yet (device-scope atomics: a marking workgroup takes the
                            flags of its share of the range and returns what it leaves, the other marking workgroups of the game and
                            the write barrier of a speculative marking raise them) */
    , TM_GS_GC_MARK_PARTS = 58, /* sum over the marking launches of the marking workgroups the game had (each owns a share of its range) */
    TM_GS_GC_MARK_SHARED,      /* sum over the marking launches of the games its marking workgroup had in that launch (its time is shared) */
    TM_GS_GC_CYC_LOAD,         /* the marker's waves, shader cycles / 64: waiting for a block's rows, */
    TM_GS_GC_CYC_ROUNDS,       /* ... marking inside a block, */
    TM_GS_GC_CYC_WAVES,        /* ... in their loop all in all (the rest: looking for work, waiting for it), */
    TM_GS_GC_IDLE_TURNS        /* turns of that loop that found nothing flagged */
};
#define TM_GC_FLAG_WORDS 4
/* TM_GS_PENDING: 0 no simulation under way; 1 the leaf is expanded, its requests posted, the backup is due; 2 suspended in the
   expansion (a collection under way); TM_PENDING_POSTED as 1, under a request cap: the evaluator may have left the request out */
#define TM_PENDING_POSTED 3
/* error bits in TM_GS_ERR */
#define TM_ERR_POOL 1      /* node pool exhausted even after reclaiming unreachable nodes */
#define TM_ERR_TRACE 2     /* trace longer than max_trace */
#define TM_ERR_TABLE 4     /* transposition table full */
#define TM_ERR_EVAL_LIST 8 /* the dense request list overflowed: the caller did not flip eval_parity between two TM_SIM_FRONT launches */
#define TM_ERR_GC_GRID 16  /* a collection under way was met by a launch with another number of collector workgroups than the launch
                              that began it (launches over another range of games: a sub-batch, the full store): the shares and the
                              arrival count would not add up, so the collection is not touched and the game is flagged */

/* agent numerics (which reference twin is reproduced bit for bit) */
#define TM_KIND_VALUESIM 0     /* agents/ValueSim.py:76-94      : evaluate the leaf, fp64 carry             */
#define TM_KIND_VALUESIM_LP 1  /* agents/ValueSimLP.py:44-70    : evaluate the leaf's unique children, core.h:303-381 */
#define TM_KIND_CPPAGENT_LP 2  /* agent.cpp:420-436,517-566     : float carry, end_obs[o], no gamma^2       */
#define TM_KIND_CPPAGENT 3     /* agent.cpp:437-446,496-513     : float carry, single leaf                 */
#define TM_KIND_VANILLA 4      /* agents/Vanilla.py:42-64       : random rollout to the end of the game (CPython MT19937 randint), variance 1e3 */
#define TM_KIND_VANILLA_C 5    /* agents/VanillaC.py:5-14 via agent.cpp:447-455 (evaluator type 1): rollout with randint(0, 7),
                                  variance 1e5, float carry, the C++ agent's root statistics */
#define TM_KIND_DIST 6         /* DistValueSim: the reference's unfinished distributional agent (agents/DistValueSimOnline.py, does
                                  not import) rebuilt from its working parts - agents/core_distributional.py:12-124 - on a tree without
                                  the observation projection: obs_stat[node] = (visit, mean, variance, M2) as floats, node_dist[node] =
                                  dist_bins atoms over [dist_vmin, dist_vmax); the evaluator fills eval_dist; low = 5 */

typedef struct tm_store {
    /* sizes */
    int32_t n_games;      /* games owned by this process (one wavefront each) */
    int32_t max_nodes;    /* node / observation pool size per game (agents/agent.py:36, ValueSim.py:16) */
    int32_t table_cap;    /* transposition table slots per game, power of two >= 2*max_nodes */
    int32_t max_trace;    /* trace capacity per game */
    int32_t eval_slots;   /* leaf-evaluation slots per game: 1 (ValueSim) or 7 (leaf-parallel) */
    int32_t nq_size;      /* entries in nq_table */
    /* environment (pyTetris ctor arguments, play.py:75) */
    int32_t app, scoring, randomizer;
    /* search */
    int32_t low;          /* check_low threshold (core.h:65-77): 1 for ValueSim/LP, 5 for Vanilla */
    int32_t kind;         /* TM_KIND_* */
    int32_t min_visits_to_store; /* ValueSim.py:14 / ValueSimLP.py:11 */
    int32_t online;       /* harvest replay tuples on GC (ValueSim.py:109-115) */
    int32_t replay_cap;   /* capacity (tuples) of the replay buffer */
    int32_t gc_slice_cycles; /* shader cycles the collector workgroups of a tm_sim_step launch may spend marking (0: no limit) */
    double gamma;
    /* node store, per game contiguous */
    uint32_t *node_rec;   /* [G][N][32] 7 x (child, obs, score, own score) unique children in selection order, then (0, self_obs, self_score, hdr) */
    uint32_t *node_game;  /* [G][N][16] packed game */
    uint32_t *obs_stat;   /* [G][N][4]  visit (bits 0-30) | end << 31, value(f32), variance(f32), sqrtf(variance / (float)visit)
                             (the exploration term of policy_clt, core.h:98, evaluated when the statistics change) */
    uint32_t *obs_key;    /* [G][N][12] packed observation */
    uint64_t *node_tab;   /* [G][cap]   (hash>>32)<<32 | node index ; index 0 = empty */
    uint64_t *obs_tab;    /* [G][cap] */
    int32_t *free_node;   /* [G][N] free-index stacks (pop from the end, agents/agent.py:99) */
    int32_t *free_obs;    /* [G][N] */
    int32_t *gs;          /* [G][TM_GS_DW] control blocks */
    uint32_t *rng;        /* [G][32] glibc rand() state (31 words) per game (core.h:62,76) */
    uint32_t *env_game;   /* [G][16] the real games */
    int32_t *env_line_stats; /* [G][4] */
    uint32_t *trace;      /* [G][max_trace][4] the last walk: per level (node, its observation, its score bits, its record's header) */
    int32_t *leaf;        /* [G][32] unique children of the leaf: node[7], obs[7], score bits[7], end[7] */
    int32_t *eval_obs;    /* [G*eval_slots] observation index inside the game's pool, 0 = unused slot */
    float *eval_v;        /* [G*eval_slots] evaluator outputs */
    float *eval_var;
    const float *nq_table;/* [nq_size] (float)norm_quantile(n), special.h:26-33, built on the host with libm */
    uint8_t *gc_mark;     /* [G][2][N/8 rounded to 16B] scratch bitmaps for GC: reachable nodes, observations of reachable nodes */
    int32_t *gc_queue;    /* [G][N] queue scratch of the one-group collection (update_root's exhausting pop, the single calls) */
    /* replay tuples harvested at GC (ValueSim.py:122-159): per game ring, gathered by the host side */
    uint32_t *replay_obs; /* [G][replay_cap][12] */
    float *replay_stat;   /* [G][replay_cap][4] value, variance, visit, 0 */
    int32_t *replay_count;/* [G] */
    uint32_t *mt_state;   /* [G][625] CPython random state per game (624 words + index), TM_KIND_VANILLA / TM_KIND_VANILLA_C rollouts (Vanilla.py:4,52) */
    uint32_t *node_child; /* [G][N][8] raw child[7] per action (agents/agent.py:61) + the node's own observation (node_to_obs once more:
                             the collectors' marker reads children and observation in one 32-byte row) */
    int32_t *gc_part;     /* [G][TM_GC_PART_DW] per-collector counts of a collection in progress */
    /* TM_KIND_DIST only */
    float *node_dist;     /* [G][N][TM_DIST_ROW] the nodes' value distributions (agents/core_distributional.py node_dist) */
    float *eval_dist;     /* [G][TM_DIST_ROW] the evaluator's distribution for the game's pending leaf (model_distributional.Net) */
    const double *nq_table_d; /* [nq_size] norm_quantile(n) in double (policy_dist multiplies in double), host libm */
    double dist_vmin, dist_vmax;
    int32_t dist_bins;
    int32_t gc_spec_nodes; /* a game with fewer free nodes than this has its tree marked speculatively while it goes on simulating
                              (tree.hip GC_SPEC_*); 0: never */
    /* dense evaluation requests: beside the per-game slots (eval_obs) every tm_sim_step launch appends the requests it posts to
       a list the built-in evaluators draw dense work from (conv waves, 32-row FC tiles).  TM_EVAL_SEGS(n_games) segments (game
       g appends to segment g % segs: one device atomic per game and launch, spread over the segments' counters); entry d of
       segment s lives at eval_list[(s + segs * (d / eval_slots)) * eval_slots + d % eval_slots].  Two sets of counters: a launch
       with TM_SIM_FRONT appends under eval_parity and clears the other set, so the CALLER FLIPS eval_parity before every such
       launch; the evaluator call that follows reads s->eval_parity from the struct it is handed, so it must be handed THE SAME
       tm_store value (parity included) as the tm_sim_step before it - not a stale copy.  tm_move_begin clears both sets.  A
       caller that does not flip lets a segment's counter grow from launch to launch: the append is bounded and the game is
       flagged TM_ERR_EVAL_LIST.  tm_sim_step / tm_move_begin return hipErrorInvalidValue when eval_list / eval_cnt are NULL. */
    int32_t *eval_list;   /* [G*eval_slots][2] (request slot, observation index) */
    int32_t *eval_cnt;    /* [G][2] entries per segment and parity (segment s of the games of *this at [s][parity]) */
    /* TM_KIND_VALUESIM / TM_KIND_CPPAGENT with TM_SIM_EVAL_NEEDED: the evaluator's output per observation, (v, var, epoch bits, 0);
       valid while epoch == eval_epoch (>= 1; the owner of the weights bumps it when they change); NULL: no cache */
    float *obs_eval;      /* [G][N][4] */
    int32_t eval_parity;  /* 0 / 1, see eval_list */
    int32_t eval_epoch;
    /* TM_KIND_DIST with online != 0: the distributions of the harvested nodes (DistValueSimOnline.store_nodes,
       agents/DistValueSimOnline.py:116-141: a freed node with >= min_visits_to_store visits whose seven children have all been
       visited; replay_obs = its packed observation, replay_stat = (0, 0, visits, 0)) */
    float *replay_dist;   /* [G][replay_cap][TM_DIST_ROW] */
    /* a launch over SOME of the games (the catch-up launches at the end of a move: a handful of games that spent launches
       collecting garbage still owe simulations): simulation wave i of tm_sim_step takes game game_list[i], i < n_listed; the
       collector workgroups look after all n_games as always.  NULL: every game (wave i = game i).  Filled by tm_sims_owing. */
    const int32_t *game_list;
    int32_t n_listed;
    int32_t gc_cost_units; /* cost units of bounded collection steps (init 1, count + re-insertion of the nodes 6, write + re-insertion of
                              the observations 7: about 5 microseconds a unit) the collector workgroups of one tm_sim_step launch take
                              on; 0: the default (13).  More units serve more collections per launch and make the launch longer. */
    int32_t gc_collectors; /* collector workgroups per tm_sim_step launch (half for the bounded steps, half for the marking); 0: the
                              default (128), at most 128.  A collection must be continued by launches with the same number. */
    /* the request cap (single-leaf kinds, eval_slots == 1, the built-in value net; tm_search_set_request_cap): the evaluator serves
       the first eval_cap dense positions of a launch's list, counted through the segments cyclically from segment eval_rot (the
       caller advances it every launch, so that no segment stands last every time), and writes eval_served[s] = the entries of
       segment s among them.  The game of a request left out posts it again in the next tm_sim_step launch, does not back up and
       owes a launch (tm_sims_owing).  eval_cap == 0: every request is served; eval_served == NULL: a store without the cap.
       eval_cap changes between moves only (no request is pending there): launches under a cap run a kernel of their own. */
    int32_t eval_cap;
    int32_t eval_rot;      /* in [0, TM_EVAL_SEGS(n_games)) */
    int32_t *eval_served;  /* [G] (segment s of the games of *this at [s]) */
} tm_store;
#define TM_EVAL_SEGS(n_games) ((n_games) < 64 ? (n_games) : 64)

/* pools, free lists, tables, rng (seed 1), control blocks.  Everything else must be zero-filled by the caller. */
int tm_pool_init(const tm_store *s, void *stream);
/* re-initialise the trees of the games with mask[g] != 0 (pool exhausted beyond what GC can reclaim; the reference has
 * undefined behaviour there, agent.cpp:227-231); clears TM_ERR_POOL; the caller re-roots with tm_update_root */
int tm_pool_reset(const tm_store *s, const uint8_t *mask, void *stream);
/* the trees of ALL games as tm_pool_init leaves them in a newly built (zero-filled) store: pools, tables, free lists, low-water
 * marks, the whole control block (counters and error flags included), the rand() stream re-seeded (seed 1), replay_count, and
 * trace, leaf, the evaluation slots, eval_list / eval_cnt / eval_served, obs_eval, the collector scratch and, for TM_KIND_DIST,
 * node_dist / eval_dist.  NOT touched: env_game / env_line_stats, mt_state (the caller's Vanilla random states), replay_obs /
 * replay_stat / replay_dist (unread beyond replay_count), the tables of constants.  Between two moves only; the caller re-roots
 * with tm_update_root and tells its search handles (tm_search_fresh).  hipErrorInvalidValue for a store without its buffers. */
int tm_pool_fresh(const tm_store *s, void *stream);
/* host helper: fills host_table[n] = (float)norm_quantile((double)i) with this machine's libm */
void tm_fill_norm_quantile(float *host_table, int n);
void tm_fill_norm_quantile_f64(double *host_table, int n);      /* the same values in double (TM_KIND_DIST: nq_table_d) */

/* environment (batched pyTetris) */
int tm_env_init(const tm_store *s, const uint32_t *seeds, void *stream);                /* Tetris(...) */
int tm_env_step(const tm_store *s, const int32_t *actions, void *stream);               /* game.play(a) */
int tm_env_reset(const tm_store *s, const uint8_t *mask, void *stream);                 /* game.reset() where mask!=0 (NULL: where ended) */
int tm_env_render(const tm_store *s, int8_t *out /* [G][200] */, void *stream);         /* game.getState() */
int tm_env_info(const tm_store *s, int32_t *out /* [G][8]: end, score, lines, combo, ls[4] */, void *stream);

/* tree agent */
int tm_update_root(const tm_store *s, void *stream);                                    /* agent.update_root(game) */
/* TreeAgent's single calls as agents.cppmodule.agent exports them (agent.cpp:829 new_node, :833 expand, :828 remove_nodes;
 * agents/agent.py:90-145,246-257), one game state per tree.  games: device [G][16] packed games (the layout of
 * s->env_game; a pyTetris buffer in the reference); mask: device [G] or NULL (all games); out_idx: device [G] or NULL,
 * the node index new_node(game) returned (-1 where masked out).  tm_tree_expand = idx = new_node(game), then
 * child[idx][a] = new_node(game.play(a)) for the seven actions (agent.cpp:201-208), with the record's unique-child list.
 * A collection runs at the exhausting pop exactly as in the reference, so - as there - `game` must be reachable from the
 * root (or the pool must not run dry) for its node to survive the call. */
int tm_tree_new_node(const tm_store *s, const uint32_t *games, const uint8_t *mask, int32_t *out_idx, void *stream);
int tm_tree_expand(const tm_store *s, const uint32_t *games, const uint8_t *mask, int32_t *out_idx, void *stream);
int tm_tree_remove_nodes(const tm_store *s, const uint8_t *mask, void *stream);             /* agent.remove_nodes() */
/* One move of every game = tm_move_begin(sims), then launches of tm_sim_step(BACKUP|FRONT) each followed by the leaf
 * evaluator, until tm_sims_remaining reports 0: a launch starts a new simulation for a game only while the game has
 * quota left, backs up its pending one, or - when the game's node pool ran dry - runs one slice of its garbage
 * collection instead (s->gc_slice_cycles), so `sims` launches + 1 are enough unless a game collected in this move. */
int tm_move_begin(const tm_store *s, int sims, void *stream);
int tm_sims_remaining(const tm_store *s, int32_t *out /* device int[2]: max over games of launches still needed; games whose collection is under way */, void *stream);
/* the same, and WHICH games still need launches: out[2] = their number, list[0 .. out[2]) = their indices (any order; list:
 * device int32[n_games]) - what a caller puts into tm_store::game_list / n_listed for the launches that follow */
int tm_sims_owing(const tm_store *s, int32_t *out /* device int[3] */, int32_t *list, void *stream);
/* one step of every garbage collection under way (the collector workgroups of tm_sim_step alone, no simulation): what the
 * driver launches instead of whole simulation launches while it waits for collections at the end of a move */
int tm_gc_step(const tm_store *s, void *stream);
#define TM_SIM_BACKUP 1  /* finish the pending simulation: backup with eval_v/eval_var */
#define TM_SIM_FRONT 2   /* start one: select, expand, post evaluation requests into eval_obs */
#define TM_SIM_GC_FULL 4 /* a game that is collecting garbage finishes the collection in this launch (catch-up launches) */
#define TM_SIM_EVAL_NEEDED 8 /* the evaluator is a pure function of the observation (the built-in value net): post only the
                                requests whose outputs the backup will use - leaf-parallel kinds: the children on their first
                                visit (core.h:341-350; agent.cpp:536-545: and not finished); TM_KIND_VALUESIM / TM_KIND_CPPAGENT:
                                not a leaf whose observation was evaluated under the current weights (s->obs_eval).  Results
                                are identical either way; a Python evaluator callable keeps receiving all k children
                                (agent.cpp:424-436), so the Python-driven loop sets it only where the caller promises a pure
                                evaluator (TreeAgent's evaluator_pure) */
#define TM_SIM_GC_MEM_MARKS 16 /* the collector workgroups keep their mark bitmaps in memory whatever the pool's size (the form pools of
                                  more than 100 000 nodes take, tree.hip gc_marks_in_lds); set by tm_sim_step / tm_gc_step themselves when
                                  TM_GC_MARKS_IN_MEMORY=1 is in the environment (tests) */
int tm_sim_step(const tm_store *s, int flags, void *stream);
/* The tree kernel exists once per agent family, each without the others' code; tm_sim_step picks by the store's kind and cap alone.
 * tm_sim_step_kernel is that choice (host only, no GPU needed): one of TM_SIM_KERNEL_*, or -1 where tm_sim_step returns
 * hipErrorInvalidValue - an unknown kind, a negative cap, or a cap on a kind that can not carry one (TM_KIND_DIST among them). */
#define TM_SIM_KERNEL_VALUE 0    /* k_sim_step<false>: the value kinds (TM_KIND_VALUESIM .. TM_KIND_CPPAGENT) */
#define TM_SIM_KERNEL_ROLLOUT 1  /* k_sim_step<true>: TM_KIND_VANILLA, TM_KIND_VANILLA_C */
#define TM_SIM_KERNEL_CAPPED 2   /* k_sim_step_capped: TM_KIND_VALUESIM / TM_KIND_CPPAGENT with eval_cap > 0 */
#define TM_SIM_KERNEL_DIST 3     /* k_sim_step_dist: TM_KIND_DIST */
int tm_sim_step_kernel(int kind, int eval_cap);
int tm_eval_render(const tm_store *s, int8_t *out /* [G*eval_slots][200] */, void *stream);
/* Dense requests for an evaluator the engine does not own (eval_requests.hip): instead of rendering every slot, hand the
 * evaluator the posted ones only and put its rows back.  The REQUESTS of *s are the slots j in [0, n_games * eval_slots) with
 * eval_obs[j] != 0, in ascending j; R = their number.  (eval_obs, not eval_list: the order is the same from run to run and the
 * call does not depend on eval_parity.)  *s may be a tm_store_slice: slots are relative to it.
 * tm_eval_gather, n = min(R, cap): for p < n, slots[p] = the p-th request and states[p] = the 200 bytes the render call above
 * writes for that slot (TM_KIND_DIST: the node's observation, packed from node_game); with m = min(cap, ceil(n / pad) * pad),
 * rows n <= p < m are all-zero states with slots[p] = -1, so the evaluator sees few distinct batch shapes; count[0] = R,
 * count[1] = n; nothing at or beyond row m is written.  R > cap is no error: the caller sees it in count.  A request whose index
 * lies outside the pool (no launch posts one) is listed and its row written as zeros.  states: 4-byte aligned.
 * tm_eval_scatter: eval_v[slots[p]] = v[p], eval_var[slots[p]] = var[p] for p < count[1]; a slot outside the store is skipped;
 * nothing else is written.  count is read on the device: the host needs no value to launch it.
 * tm_eval_scatter_dist (TM_KIND_DIST only): the first dist_bins floats of row p of dist (rows of dist_stride floats) into
 * eval_dist[slots[p]], nothing else of that row; hipErrorInvalidValue for any other kind and for dist_stride < dist_bins.
 * All three enqueue on stream; they do not allocate, synchronise or read anything back.  hipErrorInvalidValue, nothing launched,
 * for a NULL pointer, cap < 1 or pad < 1: checked before the first HIP call, so these answer on a machine without a GPU.
 * A workgroup of the gather takes TM_EVAL_GATHER_SHARE slots and counts the requests before them itself: no workgroup waits
 * for another one, no atomic decides the order. */
#define TM_EVAL_GATHER_SHARE 512
int tm_eval_gather(const tm_store *s, int cap, int pad, int8_t *states /* [cap][200] */, int32_t *slots /* [cap] */,
                   int32_t *count /* device int32[2] */, void *stream);
int tm_eval_scatter(const tm_store *s, const int32_t *slots, const int32_t *count, const float *v, const float *var, void *stream);
int tm_eval_scatter_dist(const tm_store *s, const int32_t *slots, const int32_t *count, const float *dist, int dist_stride,
                         void *stream);

/* Self-play records on the device (episodes.hip): what the reference's DataSaver.add collects through getters every move
 * (util/Data.py:14-26,63-96; play.py:131-132), written by the device into rows that are the file's rows, plus a log of the
 * episodes that end.  A State row, TM_EPISODE_ROW_BYTES, little-endian:
 *     0 episode i4 | 4 cycle i4 | 8 slot i4 (game index) | 12 move i4 (0-based index of the row within its episode) |
 *    16 combo i4 | 20 lines i4 | 24 score i4 (the fields of the info call above, before the action) | 28 line_stats i4[4] |
 *    44 value f4 | 48 variance f4 (the root observation's: TreeAgent.get_value_and_variance()) |
 *    52 child_stats f4[3][7] (the caller's root statistics buffer, copied) |
 *   136 policy f4[7]: child_stats[0][a] / (the seven visits added in index order), fp32 IEEE division; no visit: NaN |
 *   164 board i1[20][10] (the render call's bytes for that game) | 364 action i1 | 365 three pad bytes, written as 0
 * An episode row, TM_EPISODE_DONE_BYTES: episode, cycle, slot, moves (the State rows of the episode), score, lines,
 * line_stats[4], all i4, the last three FINAL: taken after the action that ended the game.
 * Per-slot state slot_state: int32 [G][TM_EPISODE_SLOT_DW] = episode_id, move_idx, live, one spare; counters: int32 [2] =
 * next_id, n_done.
 * tm_episode_init: episode_id[g] = first_id + g, move_idx = live = 0, next_id = first_id + G, n_done = 0.
 * tm_episode_record, after the search and before the action is applied, writes exactly G rows (rows: [G][368], 4-byte aligned):
 * for a game that has not ended the row above, and live = 1; for one that has (a slot the caller did not reset) episode = -1 and
 * every other byte 0, live untouched.  env: the games (env_game, env_line_stats, n_games); tree: the agent's store or NULL
 * (value = variance = 0); stats [G][3][7] and action [G] as the root statistics call left them (or what is actually played).
 * tm_episode_advance, after the action is applied and before ended games are reset: a slot with live set whose game has now
 * ended is finished - its episode row goes to done[n_done + r], episode_id = next_id + r, move_idx = 0, r its rank among the
 * slots that finish in this call IN ASCENDING SLOT ORDER; a live slot whose game goes on gets move_idx += 1; live is cleared
 * everywhere; next_id and n_done advance by the number finished.  done rows at or beyond cap are not written, n_done advances all
 * the same: the caller sees the overflow in the count.  (With one game the ids are the reference's ngames counter; with G games
 * the first G episodes are the slots, later ids follow play.py's Episode: lines - by move, then by slot.)
 * All three enqueue on stream; they do not allocate, synchronise or read anything back, use no atomics, are deterministic and
 * write nothing outside the arrays named.  hipErrorInvalidValue, nothing launched, for a NULL pointer (tree excepted),
 * n_games < 1, cap < 1, first_id < 0, a misaligned rows / done or a tree of another n_games: checked before the first HIP call,
 * so these answer on a machine without a GPU. */
#define TM_EPISODE_ROW_BYTES 368
#define TM_EPISODE_DONE_BYTES 40
#define TM_EPISODE_SLOT_DW 4
int tm_episode_init(int n_games, int first_id, int32_t *slot_state, int32_t *counters, void *stream);
int tm_episode_record(const tm_store *env, const tm_store *tree, const float *stats, const int32_t *action, int cycle,
                      int32_t *slot_state, void *rows, void *stream);
int tm_episode_advance(const tm_store *env, int cycle, int32_t *slot_state, int32_t *counters, void *done, int cap, void *stream);

/* Position rows (episodes.hip): the game a State row was recorded from, so that the move can be searched again under other
 * weights (reanalyse.py).  A position row, TM_POSITION_ROW_BYTES, little-endian:
 *     0 episode i4 | 4 cycle i4 | 8 slot i4 | 12 move i4: the four values of the State row of that game and move |
 *    16 game u4[16]: the packed game (ENGINE_SPEC.md section 2) as it stood when the row was recorded, before the action |
 *    80 line_stats i4[4]
 * tm_episode_record_positions, right after tm_episode_record and before tm_episode_advance, on the same env, slot_state and
 * cycle, writes exactly G rows (rows: [G][96], 4-byte aligned) in slot order: for a game that has ended episode = -1 and every
 * other byte 0, as its State row.  It reads slot_state and writes nothing but rows.
 * tm_episode_rerecord: n <= G old State rows on the device, env the environment into which their positions were loaded (slot i =
 * row i), tree the store searched from those roots and stats its tm_root_stats buffer -> n new State rows (rows: [n][368]).
 * episode, cycle, slot, move and the action's dword (its pad bytes included) are the old row's; combo, lines, score, line_stats and
 * board are recomputed from the loaded game by tm_episode_record's own rule; value, variance, child_stats and policy are
 * tm_episode_record's from tree and stats.  THE GUARD: the recomputed columns must be the old row's bit for bit, and the loaded
 * game must not have ended (such a game has no row).  fault: device int32 [2], set to (INT32_MAX, 0) by the caller; a row that
 * fails does atomicMin(fault[0], 4 * row + group) with group the first of TM_REREC_* that differs, and atomicAdd(fault[1], 1);
 * the caller then discards rows (they are written all the same).  Integer atomics only: the result does not depend on their order.
 * Both enqueue one kernel on stream, allocate nothing and read nothing back.  hipErrorInvalidValue, nothing launched, for a NULL
 * pointer, n_games < 1, n outside [0, G], a tree of another n_games, a misaligned buffer: checked before the first HIP call. */
#define TM_POSITION_ROW_BYTES 96
#define TM_REREC_SCALARS 0     /* combo, lines, score */
#define TM_REREC_LINE_STATS 1
#define TM_REREC_BOARD 2
#define TM_REREC_ENDED 3       /* the loaded game has ended */
int tm_episode_record_positions(const tm_store *env, const int32_t *slot_state, int cycle, void *rows, void *stream);
int tm_episode_rerecord(const tm_store *env, const tm_store *tree, const float *stats, const void *old_rows, int n, void *rows,
                        int32_t *fault, void *stream);

/* Root-distribution rows (episodes.hip): the distribution the search of a TM_KIND_DIST tree backed up into the root, beside the
 * State row of that game and move - what the distributional head is fitted to (train.py --head dist --td --bootstrap search) and
 * what a re-analysis of DistValueSim's moves makes again (reanalyse.py --root_dists).  A root-distribution row,
 * TM_ROOT_DIST_ROW_BYTES, little-endian:
 *     0 episode i4 | 4 cycle i4 | 8 slot i4 | 12 move i4: the four values of the State row of that game and move |
 *    16 dist f4[TM_DIST_ROW]: node_dist[g][root][0 .. 63] with root = gs[g][TM_GS_ROOT] (DistValueSim.get_value's node): the atoms
 *       b < dist_bins as their bits, never converted; the atoms b >= dist_bins written as 0
 * tm_episode_record_root_dists, right after tm_episode_record or tm_episode_rerecord on the same tree: state_rows are the n State
 * rows (stride TM_EPISODE_ROW_BYTES) that call has just written on the device for the slots 0 .. n-1 of tree, rows: [n][272].  The
 * identity is copied from the State rows, so the two tables cannot drift apart and neither env nor slot_state is read; a State row
 * with episode == -1 (a game that has ended) gives episode = -1 and every other byte 0, as its State and position rows.  A root
 * index outside [0, max_nodes) is never made an address: the row's dist is zeros.
 * It enqueues one kernel on stream (plain stores, no atomics), allocates nothing, synchronises with nothing, reads nothing back and
 * writes nothing outside rows; n == 0 returns 0 and launches nothing.  hipErrorInvalidValue, nothing launched, for a NULL pointer,
 * n < 0 or n > tree->n_games, a tree whose kind is not TM_KIND_DIST or whose node_dist / gs is NULL, max_nodes < 1, dist_bins
 * outside 1 .. TM_DIST_ROW, a state_rows / rows that is not 4-byte aligned: checked before the first HIP call, so these answer on a
 * machine without a GPU. */
#define TM_ROOT_DIST_ROW_BYTES 272
int tm_episode_record_root_dists(const tm_store *tree, const void *state_rows, int n, void *rows, void *stream);

/* Training targets from recorded episodes (episode_targets.hip; the reference's train.py:81-131).  rows: n_rows State rows on the
 * device in ANY order (file order - move-major, slot-minor - is the normal case; they are read in place, 4-byte aligned).
 * order: int32 [n_rows]; seg: int32 [n_seg + 1]: segment e is the sorted positions seg[e] .. seg[e+1]-1, and rows[order[j]] over
 * them is one episode in ascending move order.  Per segment a tail: tail_kind u8 (1: one virtual element (tail_score, tail_value)
 * follows the episode's last row - an episode that ended, its FINAL score, value 0; 0: nothing follows), tail_score i32,
 * tail_value f32.  Outputs by sorted position j: value[j], variance[j], weight[j], float32.
 * With s_k the row's score (int) and v_k its value column over the series k = 0 .. (the tail included if there is one):
 *   mode 0 (Monte Carlo): value_i = s_end - s_i, s_end the tail's score, without a tail the last row's; integer arithmetic,
 *       converted to float once.
 *   mode 1 (lambda-return): value_i = sum_k lambda^k (s_{i+k} + v_{i+k} - s_i) / sum_k lambda^k over k = 0 .. end of the series,
 *       accumulated in fp64 (N_i = v_i + lambda (N_{i+1} + B_{i+1} (s_{i+1} - s_i)), B_i = 1 + lambda B_{i+1}, value_i = N_i / B_i)
 *       and rounded to fp32 once; lambda = 0 gives v_i, lambda = 1 the plain mean.
 *   mode 2: value_i = v_i, the bits copied.
 * variance[j]: the row's variance column, the bits copied, in every mode.  weight[j] by weight_mode: 0: 1; 1: 1.0f / (variance +
 * eps), IEEE fp32; 2: the seven visits child_stats[0][a] added in index order; 3: that sum / (variance + eps).  Nothing is
 * normalised (the fit divides the weights by their mean).
 * An order[j] outside [0, n_rows) is never made an address: position j gets value = variance = weight = 0, *fault = 1 (a device
 * int32 the caller cleared; a plain store), and the position is left out of its episode's series.  seg entries outside
 * [0, n_rows] are clamped and set *fault as well.
 * tm_episode_gather_states: out float32 [n][200] (16-byte aligned) = the board cells of rows[idx[k]], the int8 values the row
 * holds; an idx[k] outside [0, n_rows) gives a board of zeros and *fault = 1.
 * Both enqueue one kernel on stream and make no other HIP call; they write nothing outside their outputs and *fault, use no
 * atomics and are deterministic.  hipErrorInvalidValue, nothing launched, for n_rows < 0, n_seg < 0, n < 0, a mode outside 0..2,
 * a weight_mode outside 0..3, a lambda outside [0, 1] (a NaN included), and - when there is work - a NULL pointer or a misaligned
 * rows / out; n_rows == 0, n_seg == 0 or n == 0 returns 0 and launches nothing.  All checked before the first HIP call.
 * Run on an MI355X against a numpy statement of these definitions and an exact oracle (tests/test_gpu_offline.py) and timed there
 * (profiles/offline_targets_timing.json); a table of more than 2^31 - 64 rows is refused and has not been run. */
int tm_episode_targets(const void *rows, int n_rows, const int32_t *order, const int32_t *seg, int n_seg, const uint8_t *tail_kind,
                       const int32_t *tail_score, const float *tail_value, int mode, double lambda, int weight_mode, float eps,
                       float *value, float *variance, float *weight, int32_t *fault, void *stream);
int tm_episode_gather_states(const void *rows, int n_rows, const int32_t *idx, int n, float *out, int32_t *fault, void *stream);

/* tm_episode_targets with a discount per move and, optionally, another source for the values.  Everything not named here is
 * tm_episode_targets' own: the rows read in place, order / seg / the tails, the outputs by sorted position, variance[j] and
 * weight[j] (always from the ROW's variance and visits), the bounds rules, one kernel on stream and no other HIP call, no
 * atomics, deterministic, nothing written outside the three outputs and *fault.
 * v_rows: NULL, or float32 [n_rows] BY TABLE ROW (4-byte aligned): v_k of a row is then v_rows[order[.]] instead of the row's value
 * column; the tail's value stays tail_value.  With r_k = s_{k+1} - s_k (integers) over the series, the tail included:
 *   mode 0: value_i = sum_{k >= i} gamma^(k-i) r_k; without a tail the last row is the end (value 0).  gamma == 1.0 takes
 *       tm_episode_targets' integer statement; otherwise D_i = r_i + gamma D_{i+1} in fp64, rounded to fp32 once.
 *   mode 1: value_i = sum_k lambda^k T_{i,k} / sum_k lambda^k, T_{i,k} = sum_{j<k} gamma^j r_{i+j} + gamma^k v_{i+k}, k to the end
 *       of the series: N_i = v_i + lambda (gamma N_{i+1} + B_{i+1} r_i), B_i = 1 + lambda B_{i+1}, value_i = N_i / B_i, in
 *       fp64, rounded to fp32 once.
 *   mode 2: value_i = v_i, the bits copied from v_rows or from the row.
 * At gamma == 1.0 and v_rows == NULL the three outputs and *fault are tm_episode_targets' bit for bit in every mode and weight
 * mode (tests/test_gpu_offline_discount.py).  A non-finite v_rows[k] is not an error: it propagates by IEEE rules into the values
 * of its episode.
 * hipErrorInvalidValue, nothing launched, checked before the first HIP call: everything tm_episode_targets refuses; a gamma
 * outside (0, 1] (a NaN included); v_rows given with mode 0 (mode 0 reads no value); a misaligned v_rows. */
int tm_episode_targets_discounted(const void *rows, int n_rows, const int32_t *order, const int32_t *seg, int n_seg,
                                  const uint8_t *tail_kind, const int32_t *tail_score, const float *tail_value,
                                  const float *v_rows, int mode, double lambda, double gamma, int weight_mode, float eps,
                                  float *value, float *variance, float *weight, int32_t *fault, void *stream);

/* Categorical targets for the distributional head from the same rows (episode_dist_targets.hip): the search's distributional
 * backup (shift by the score gained, mix) along the moves played.  rows, order, seg, tail_kind and tail_score are
 * tm_episode_targets' (seg does not fall: a position finds its segment by bisection); there is no tail value: the tail element is
 * tail_score with ALL MASS IN ATOM 0, the search's v_dummy of a finished game.  atoms K in 1 .. TM_DIST_ROW over [vmin, vmax),
 * delta = (vmax - vmin) / K in double.
 * The shift S_c(p) by an integer score difference c >= 0 is tm_distpy_shift's rule: bs = (double)c / delta, n = floor(bs),
 * f = bs - n; source atom a gives p[a] (1 - f) to lb = min(a + n, K-1) and p[a] f to min(lb + 1, K-1); mass that reaches the top
 * atom stays there.  The series of an episode is its rows in move order, then the tail element where tail_kind == 1.
 *   mode 0 (Monte Carlo): target_i = S_{s_end - s_i}(e_0), e_0 = all mass in atom 0, s_end the tail's score, without a tail the last
 *       row's: atom lb gets (float)(1 - f), atom lb + 1 (float)f, and 1 where the two are the top atom; no distribution is read.
 *   mode 1 (truncated lambda-return): target_i = sum_{k=0..m} lambda^k S_{s_{i+k} - s_i}(P_{i+k}) / sum_{k=0..m} lambda^k with
 *       m = min(horizon, elements after i); P of a row = p_rows[row] (float32 [n_rows][p_stride] BY TABLE ROW, atoms first; the
 *       padding is never read), P of the tail = e_0.  Per atom in fp64 in ascending k (the weight by repeated multiplication; a
 *       term in gather form, out[b] = p[b-n] (1 - f) + p[b-n-1] f, the top atom = the fp64 sum p[K-1] + p[K-2] + .. down to atom
 *       max(K-1-n, 0), added in that order, + p[K-2-n] f), divided once and rounded to fp32 once.  lambda == 0 copies P_i.
 * There is no discount (the distributional backup has none) and no mode 2: with the root-distribution rows of
 * tm_episode_record_root_dists as p_rows, mode 1 at lambda = 0 copies the recorded distribution, which is that mode.
 * Outputs by sorted position j: target[j * target_stride + b] for b < atoms ONLY, weight[j] by tm_episode_targets' four
 * weight_mode rules from the row's visits and variance.  *fault (a device int32 the caller cleared): bit 0 - an order[j] outside
 * [0, n_rows) (never made an address: a zero target row, weight 0, left out of its episode's series) or a seg entry outside
 * [0, n_rows] (clamped); bit 1 - a negative score difference, taken as 0.
 * Enqueues two kernels on stream (the weights and the bounds first; the second stores bit 1 into the word as the first left it)
 * and makes no other HIP call: no allocation, no synchronisation, no read-back, no atomics, deterministic, nothing written outside
 * target[:, :atoms], weight and *fault.  hipErrorInvalidValue, nothing launched, checked before the first HIP call: everything
 * tm_episode_targets refuses (its value pointers excepted: there are none); atoms outside 1 .. 64; target_stride < atoms, and
 * p_stride < atoms in mode 1; vmax <= vmin or a bound that is not finite; horizon < 0; a mode outside 0 .. 1; p_rows == NULL in
 * mode 1 when there is work; a p_rows or target that is not 4-byte aligned.  n_rows == 0 or n_seg == 0 returns 0.
 * Held on an MI355X to a numpy statement of these definitions and to an exact rational oracle (tests/test_gpu_offline_dist.py);
 * timed there (profiles/offline_dist_targets_timing.json). */
int tm_episode_dist_targets(const void *rows, int n_rows, const int32_t *order, const int32_t *seg, int n_seg,
                            const uint8_t *tail_kind, const int32_t *tail_score, const float *p_rows, int p_stride, int atoms,
                            double vmin, double vmax, int mode, double lambda, int horizon, int weight_mode, float eps,
                            float *target, int target_stride, float *weight, int32_t *fault, void *stream);

/* Node records (node_records.hip): the tuples the collections harvest into replay_obs / replay_stat (online != 0: the packed
 * observation, value, variance and visits of every freed observation with at least min_visits_to_store visits), moved into one
 * dense ring of rows that are a file's rows, and such rows turned into the arrays of a packed fit.  The reference writes its
 * nodes at every collection (Agent.save_nodes, agents/agent.py:246-289); the policy, the child statistics and the action of its
 * rows are not kept by the harvest and are not part of this row.  A node row, TM_NODE_ROW_BYTES, little-endian:
 *     0 obs u4[12] (the packed observation, ENGINE_SPEC.md section 7) | 48 value f4 | 52 variance f4 | 56 visit f4 |
 *    60 slot i4 (the game index)
 * The first 60 bytes are the harvest's tuple, bit for bit.
 * counters: device int32[4] = head (the ring rows in use), lost (rows that did not fit the ring), drains (calls), one spare; the
 * caller clears them and, after it has copied the ring out, head.  offsets: device int32[n_games + 1] of scratch, no initial
 * contents required (on return offsets[g] is game g's first ring row, saturated at ring_cap).
 * tm_nodes_drain: with c[g] = min(replay_count[g], replay_cap) (a negative count is taken as 0), game g's tuples 0 .. c[g]-1 go
 * to the ring rows head + sum_{h<g} c[h] + i - game-major, harvest order within a game, the order of TreeStore.replay() - and
 * replay_count[g] = 0.  Rows at or beyond ring_cap are not written and are counted in lost; head advances by what was written.
 * It belongs on the stream of the search, between two moves: it must not run beside tm_sim_step, whose collectors append to the
 * same buffers.
 * tm_nodes_sweep appends in the same way the observations still in the pools (the reference's save_occupied; once, at the end of
 * a run): per game in ascending index every slot o >= gs[TM_GS_LOW_OBS] whose statistics word passes the collection's own test,
 * (int)stat.x >= max(min_visits_to_store, 1) with bit 31 (a finished game) clear; the tuple is okey[o], stat.y, stat.z,
 * (float)(int)stat.x.  It reads the store and changes nothing in it.
 * tm_node_targets: rows (n_rows node rows, 16-byte aligned) -> obs [n][12] (4-byte aligned), value[n] and variance[n] (the bits
 * copied), weight[n] by tm_episode_targets' four weight_mode rules with the row's visit in place of the seven visits' sum -
 * 0: 1; 1: 1.0f / (variance + eps); 2: visit; 3: visit / (variance + eps), IEEE fp32.  A row whose value or variance is not
 * finite or whose visit is below 1 gets weight 0 and sets *fault = 1 (a device int32 the caller cleared; a plain store).
 * All three enqueue on stream (drain two kernels, sweep three, targets one) and make no other HIP call: no allocation, no
 * synchronisation, nothing read back, no atomics, deterministic; the scan over the games is one workgroup whose threads own runs
 * of games, for any n_games >= 1.  Nothing is written outside the ring's first ring_cap rows, counters, offsets and replay_count
 * (drain), or outside the four outputs and *fault (targets).  hipErrorInvalidValue, nothing launched, checked before the first
 * HIP call (so these answer on a machine without a GPU): a NULL pointer (a NULL array of the store that the call reads included);
 * ring_cap < 1, n_rows < 0 or above 2^29 - 1, a weight_mode outside 0..3; a ring or rows that is not 16-byte aligned, an obs
 * that is not 4-byte aligned, a replay_obs / replay_stat (drain) or obs_stat / obs_key (sweep) of the store that is not 16-byte
 * aligned (they are read as 16-byte pieces; torch allocations and tm_store_slice keep them so); a store with n_games < 1, with replay_cap < 1 (drain) or of TM_KIND_DIST (drain and sweep: its
 * harvest is of another shape, replay_dist).  n_rows == 0 returns 0 and launches nothing.
 * Held on an MI355X to numpy statements of these definitions and to TreeStore.replay() inside a search (tests/test_gpu_nodes.py). */
#define TM_NODE_ROW_BYTES 64
int tm_nodes_drain(tm_store *tree, void *ring, int ring_cap, int32_t *counters, int32_t *offsets, void *stream);
int tm_nodes_sweep(const tm_store *tree, void *ring, int ring_cap, int32_t *counters, int32_t *offsets, void *stream);
int tm_node_targets(const void *rows, int n_rows, int weight_mode, float eps, uint32_t *obs, float *value, float *variance,
                    float *weight, int32_t *fault, void *stream);

/* Node records of the distributional head (node_records.hip): what the collections of a TM_KIND_DIST store harvest (online != 0:
 * the packed observation, the backed-up distribution and the visits of every freed node with at least min_visits_to_store visits
 * whose seven children have all been visited - replay_obs, replay_dist, replay_stat = (0, 0, visit, 0)), moved into one dense ring
 * of rows that are a file's rows, and such rows turned into the arrays of a packed fit of the head (tm_distnet_fit_grad_packed).
 * A dist node row, TM_NODE_DIST_ROW_BYTES, little-endian:
 *     0 .. 63   the node row exactly as tm_nodes_drain would form it from this harvest: obs u4[12] | 48, 52 replay_stat words 0
 *               and 1, bit for bit (the harvest leaves 0) | 56 visit f4 | 60 slot i4 (the game index)
 *    64 .. 319  dist f4[TM_DIST_ROW]: the row of replay_dist, bit for bit (atoms beyond the store's dist_bins are the zero
 *               padding the harvest wrote)
 * tm_nodes_drain_dist is tm_nodes_drain on these rows, with the same counters and offsets: with c[g] = min(replay_count[g],
 * replay_cap) (a negative count is taken as 0), game g's tuples 0 .. c[g]-1 go to the ring rows head + sum_{h<g} c[h] + i -
 * game-major, harvest order within a game, the order of TreeStore.replay_dist() - and replay_count[g] = 0.  Offsets saturate at
 * ring_cap; rows at or beyond ring_cap are not written and are counted in lost; head advances by what was written; drains by
 * one.  It belongs on the stream of the search, between two moves: it must not run beside tm_sim_step, whose collectors append
 * to the same buffers.
 * tm_node_dist_targets: rows (n_rows dist node rows, 16-byte aligned) -> obs [n][12], target[i * target_stride + k] = atom k of
 * row i for k < atoms, the bits copied (the floats from atoms to target_stride are not touched), weight[i] = 1.0f (weight_mode
 * 0) or the row's visit (weight_mode 2); modes 1 and 3 of tm_node_targets divide by a variance, which this row does not carry,
 * and are refused.  A row is at fault when its visit is not finite or is below 1, when one of its first `atoms` floats is not
 * finite or is negative, when none of them is above 0 (no sum is formed: the rule has no summation order), or when a float
 * from atoms to 63 compares unequal to 0 (a file recorded with more atoms than the model has).  Such a row gets weight 0 and
 * sets *fault = 1 (a device int32 the caller cleared; a plain store); its obs and target are copied all the same.
 * Both enqueue on stream (drain two kernels - tm_nodes_drain's scan and a copy of twenty 16-byte pieces a row -, targets one) and
 * make no other HIP call: no allocation, no synchronisation, nothing read back, no atomics, deterministic.  Nothing is written
 * outside the ring's first ring_cap rows, counters, offsets and replay_count (drain), or outside obs, target[:, :atoms], weight
 * and *fault (targets).  hipErrorInvalidValue, nothing launched, checked before the first HIP call (so these answer on a machine
 * without a GPU): a NULL pointer (replay_obs, replay_stat, replay_count or replay_dist of the store included); ring_cap < 1; a
 * ring, a replay_obs, a replay_stat or a replay_dist that is not 16-byte aligned; a store with n_games < 1, with replay_cap < 1
 * or of a kind other than TM_KIND_DIST (tm_nodes_drain has the others); n_rows < 0 or above 2^29 - 1; atoms outside 1 ..
 * TM_DIST_ROW; target_stride < atoms; a weight_mode other than 0 or 2; rows that are not 16-byte aligned; an obs, target or weight
 * that is not 4-byte aligned.  n_rows == 0 returns 0 and launches nothing.  There is no sweep of the pools for this kind: its
 * harvest is per node and needs the seven-children test.
 * Held on an MI355X to numpy statements of these definitions and to TreeStore.replay_dist() inside a search
 * (tests/test_gpu_dist_nodes.py). */
#define TM_NODE_DIST_ROW_BYTES 320
int tm_nodes_drain_dist(tm_store *tree, void *ring, int ring_cap, int32_t *counters, int32_t *offsets, void *stream);
int tm_node_dist_targets(const void *rows, int n_rows, int atoms, int weight_mode, uint32_t *obs, float *target, int target_stride,
                         float *weight, int32_t *fault, void *stream);

/* Game snapshots (games_snapshot.hip): the games of an environment copied out and, after a check on the device, back in, so
 * that the games alive when a self-play run stops go on in the next one.  A game is its packed record (TM_GAME_DW dwords,
 * ENGINE_SPEC.md section 2) and its four line statistics; trees are not carried (tm_update_root builds a root from any game).
 * The engine trusts a packed game - piece and rot index its tables, a lock writes rows[y + i] - so bytes from outside pass
 * tm_env_check first.  fault[g] is a set of TM_GAME_BAD_* bits, 0 for a well-formed game:
 *   TM_GAME_BAD_PIECE       piece > 6
 *   TM_GAME_BAD_ROT         rot > 3
 *   TM_GAME_BAD_ROWS        a row with a bit above column 9, or a full row (0x3FF: a full row never survives a lock)
 *   TM_GAME_BAD_PLACE       the placement of the falling piece.  A game that has NOT ended: x outside -3..9 or y outside -3..19
 *                           (the only ranges in which a box can have a cell inside the well), or - evaluated only when piece <= 6
 *                           and rot <= 3 - the engine's collides(rows, PIECE_MASK[piece][rot], x, y): no collision is what keeps
 *                           every cell of the piece inside rows 0..19 and columns 0..9.  A game that HAS ended (flag bit 0): the
 *                           piece is where the engine leaves it.  The only place that sets the bit is spawn(), which has just set
 *                           (rot, x, y) = (0, 3, 0), and play() returns at once for an ended game, so anything but
 *                           (rot, x, y) == (0, 3, 0) is a fault (the piece's box is then inside the well whatever the rows hold).
 *   TM_GAME_BAD_FIELDS      drop_ctr >= app, a flag bit other than 0 and 1, combo < -1, or piece_count == 0
 *   TM_GAME_BAD_LINE_STATS  a negative line_stats entry (only when line_stats is given)
 * No value read from a game is used as an index, an address or a shift count before it has passed its test.
 * tm_env_check(games [n][16], line_stats [n][4] or NULL, n, app): writes fault[n] and n_bad[0] = the number of games with a fault
 *   (added in a fixed order; no atomics).
 * tm_env_save: games and line_stats <- s->env_game, s->env_line_stats (s->n_games games), a stream-ordered copy.
 * tm_env_load: tm_env_check with s->n_games and s->app, then a launch that reads n_bad ON THE DEVICE and copies every game and
 *   line statistic into s->env_game / s->env_line_stats only if it is 0: with any fault not one byte of the store changes.  The
 *   caller reads fault / n_bad back when it likes; the call itself does not synchronise.
 * tm_episode_resume: tm_episode_init with move_idx[g] taken from the array (a negative entry counts as 0): the recorder goes on
 *   in the middle of loaded games.  The value is only ever written into rows.
 * All four enqueue on stream, allocate nothing, read nothing back and write nothing outside the arrays named.
 * hipErrorInvalidValue, nothing launched, for a NULL pointer (tm_env_check's line_stats excepted), n < 1, app < 1, first_id < 0 or
 * a buffer that is not 4-byte aligned: checked before the first HIP call, so these answer on a machine without a GPU. */
#define TM_GAME_BAD_PIECE 1
#define TM_GAME_BAD_ROT 2
#define TM_GAME_BAD_ROWS 4
#define TM_GAME_BAD_PLACE 8
#define TM_GAME_BAD_FIELDS 16
#define TM_GAME_BAD_LINE_STATS 32
int tm_env_check(const uint32_t *games, const int32_t *line_stats, int n, int app, int32_t *fault, int32_t *n_bad, void *stream);
int tm_env_save(const tm_store *s, uint32_t *games, int32_t *line_stats, void *stream);
int tm_env_load(const tm_store *s, const uint32_t *games, const int32_t *line_stats, int32_t *fault, int32_t *n_bad, void *stream);
int tm_episode_resume(int n_games, int first_id, const int32_t *move_idx, int32_t *slot_state, int32_t *counters, void *stream);

/* The store of games [first, first+n) of *s (every array is per game contiguous: a slice is the same struct with
 * offset pointers).  Sub-batches of one process, shards of a multi-GPU job.  `first` is a multiple of four (a tree-kernel
 * workgroup's games; the groups of TM_GS_GC_ACTIVE4): hipErrorInvalidValue otherwise. */
int tm_store_slice(const tm_store *s, int first, int n, tm_store *out);

/* Native driver of one move's search = the reference's `for i in range(sims)` loop (agents/ValueSim.py:76-94,
 * agents/agent.py:147-150, agent.cpp:407-460) as a host launch loop.  The games are cut into n_sub sub-batches on
 * their own HIP streams so that one sub-batch's tree kernel runs under another's value-net kernels; results per game do
 * not depend on n_sub.  tm_search_run returns when all `sims` simulations of every game are complete (it issues the
 * catch-up launches of games that collected garbage, tm_sims_remaining).  vn_params == NULL: no evaluator launches
 * (TM_KIND_VANILLA).  The evaluator follows the store's kind: the value net (tm_valuenet_forward_requests; vn_scratch:
 * n_games * eval_slots * TM_VALUENET_SCRATCH_MFMA floats, no initial contents required) or, for TM_KIND_DIST, the distributional head
 * (tm_distnet_forward_requests; vn_params / vn_prepared = its blobs, vn_scratch: n_games * TM_DISTNET_SCRATCH floats), in the
 * mode of tm_search_set_valuenet.  ev_every > 0: HIP events
 * around every ev_every-th simulation of sub-batch 0 (on the stream it runs on), read back by tm_search_stats:
 * out = {runs, tree launches, catch-up launches, timed samples, sum tree-kernel ms, sum value-net ms, n_sub}. */
typedef struct tm_search tm_search;
int tm_search_create(tm_search **out, const tm_store *s, int n_sub, int ev_every);
void tm_search_destroy(tm_search *h);
int tm_search_run(tm_search *h, int sims, const float *vn_params, const float *vn_prepared, float *vn_scratch,
                  void *stream);
int tm_search_stats(tm_search *h, double *out, int n, int reset);
/* the evaluator's weights changed: s->eval_epoch of the handle's copy of the store (outputs filed in obs_eval under another
 * epoch are not used; epochs are >= 1 and never reused for other weights) */
int tm_search_set_epoch(tm_search *h, int epoch);
/* the mode of tm_search_run's evaluator: `backend` TM_VALUENET_FP32 (the default) or TM_VALUENET_BF16X3, `fc1`
 * TM_VALUENET_FC1_FP32 (the default) or TM_VALUENET_FC1_BF16X3; vn_prepared is then the prepare call's buffer for that mode (or a
 * larger one).  On a TM_KIND_DIST store `backend` is the distributional head's and fc1 must be TM_VALUENET_FC1_FP32.
 * hipErrorInvalidValue, and nothing changed, for any other pair (tm_valuenet_check_mode).  The caller gives every mode's outputs
 * an epoch of their own (tm_search_set_epoch): obs_eval must not mix them (TM_KIND_DIST keeps no obs_eval). */
int tm_search_set_valuenet(tm_search *h, int backend, int fc1);
/* The request cap of tm_search_run (tm_store::eval_cap): the value net's two kernels step up in cost where a launch holds more
 * requests than the convolution has resident waves, so the requests beyond that wait for the next launch and their games catch
 * up at the end of the move like games that collected garbage.  A change of schedule only: every game's results are what they
 * are without the cap.  cap = -1: off; 0: automatic (the default); > 0: that cap for every move (hipErrorInvalidValue where
 * the store cannot carry one).  Automatic mode acts on a store of a single-leaf kind with eval_slots == 1, the built-in value
 * net and n_sub == 1: cap = tm_valuenet_resident_states(), in force for a move when the move before it posted between
 * TM_REQUEST_CAP_LOW x cap and TM_REQUEST_CAP_T x cap requests per simulation; the first move of a handle and the first move
 * under other weights (tm_search_set_epoch) run without.  tm_search_stats: out[2], the catch-up launches, counts the launches
 * the deferred games needed as well, out[11] the moves that ran under a cap. */
int tm_search_set_request_cap(tm_search *h, int cap);
/* after tm_pool_fresh on the handle's store: the handle forgets what it keeps from the moves before (its sub-batches' list
 * parity and cap rotation, the request counts the automatic cap decides from), as a handle just created; the epoch, the value
 * net's mode, the request cap's mode and the counters of tm_search_stats stay.  A host call, no HIP call. */
int tm_search_fresh(tm_search *h);
#define TM_REQUEST_CAP_T 1.32   /* 1 + (cost of the value net's second round) / (cost of a full step): DESIGN.md section 3.6 */
#define TM_REQUEST_CAP_LOW 0.95 /* below this many times cap no launch of the next move reaches the cap, and the capped tree kernel
                                   costs a microsecond a launch over the other one: DESIGN.md section 3.6 */
int tm_root_stats(const tm_store *s, float *stats /* [G][3][7] */, int32_t *action /* [G] */, void *stream);
/* one game's tree in the reference's array layout (agents/agent.py:58-88), for inspection and tests */
int tm_export_game(const tm_store *s, int game, int32_t *child /* [N][7] */, float *score, int32_t *n_to_o,
                   int32_t *visit, float *value, float *variance, uint8_t *end_obs, void *stream);

/* agents.cppmodule.core (core.cpp:20-26) in batched form: B independent trees in the reference's own
 * array layout, tree b at offset b*n_nodes of every array.  rng: [B][32] as in tm_store. */
int tm_core_select_trace_obs(int n_trees, int n_nodes, const int32_t *roots, const int32_t *child,
                             const int32_t *visit, const float *value, const float *variance, const float *score,
                             const int32_t *n_to_o, int low, uint32_t *rng, const float *nq_table, int nq_size,
                             int32_t *trace /* [B][max_trace] */, int32_t *trace_len, int max_trace, void *stream);
int tm_core_backup_trace_obs(int n_trees, int n_nodes, const int32_t *trace, const int32_t *trace_len, int max_trace,
                             int32_t *visit, float *value, float *variance, const int32_t *n_to_o, const float *score,
                             const double *_value, const double *_variance, double gamma, void *stream);
int tm_core_backup_trace_obs_lp(int n_trees, int n_nodes, const int32_t *trace, const int32_t *trace_len,
                                int max_trace, int32_t *visit, float *value, float *variance, const int32_t *n_to_o,
                                const float *score, const uint8_t *end, const int32_t *_child /* [B][7] */,
                                const int32_t *_obs, const int32_t *k, const float *_value, const float *_variance,
                                double gamma, int mixture, int averaged, void *stream);
int tm_core_get_unique_child_obs(int n_trees, int n_nodes, const int32_t *index, const int32_t *child,
                                 const float *score, const int32_t *n_to_o, int32_t *c_nodes /* [B][7] */,
                                 int32_t *c_obs, int32_t *count, void *stream);
int tm_core_get_all_childs(int n_trees, int n_nodes, const int32_t *roots, const int32_t *child,
                           uint8_t *mark /* [B][n_nodes] */, int32_t *queue /* [B][n_nodes] scratch */, void *stream);

/* The array-level distribution helpers below (tm_dist_*, tm_distpy_*) and tm_core_get_all_childs are the compatibility
 * surface of the reference's function-per-call API: ONE LANE PER TREE / DISTRIBUTION (scalar code per lane, as the reference's
 * loops are written), meant for callers that keep the reference's arrays.  The engine's own search does this work at wave
 * level inside tm_sim_step (tree.hip: wave_dist_front / wave_dist_back, one lane per atom; the collectors' breadth-first
 * marking) and does not call them.
 *
 * distributional head helpers (agents/cppmodule/core.h:387-449; defined there, not exported by core.cpp): n categorical
 * distributions of `bins` atoms over [vmin, vmax).  tm_dist_transform: every source bin is an interval `scale` bins wide
 * shifted by shift[i] (in value units), its mass split over the two destination bins it overlaps (mass beyond the last
 * bin is dropped - the reference writes one float past its vector there).  tm_dist_mean_variance: out[i] = (mean, variance)
 * in double, bin centres vmin + (b + 1/2) delta accumulated as the reference does. */
int tm_dist_transform(int n, int bins, const float *dist /* [n][bins] */, double vmin, double vmax,
                      const double *shift /* [n] */, double scale, float *out /* [n][bins] */, void *stream);
int tm_dist_mean_variance(int n, int bins, const float *dist, double vmin, double vmax, double *out /* [n][2] */,
                          void *stream);

/* agents/core_distributional.py, the numba kernels of the reference's unfinished distributional agent, batched (one tree
 * or distribution per index): shift_distribution :12-37 (x[i] >= 0 in value units; mass reaching the top bin stays there),
 * policy_dist :66-79 (child_nodes[B][7] with n_child[B] valid entries, node_stats[B][n_nodes][5] = visit, mean, score,
 * variance, M2; returns the chosen child per tree), backup_trace_distributional :108-124 (updates node_stats and
 * node_dist[B][n_nodes][bins] along trace[B][max_trace]; scratch[B][bins]).  `fastmath` numba code: held to a float
 * tolerance (2e-6 relative), not to bit patterns.  Their mean_dist / mean_variance = tm_dist_mean_variance(vmin = 0,
 * vmax = vmax - vmin). */
int tm_distpy_shift(int n, int bins, const float *dist /* [n][bins] */, const double *x /* [n] */, double vmin, double vmax,
                    float *out /* [n][bins] */, void *stream);
int tm_distpy_policy(int n_trees, int n_nodes, const int32_t *child_nodes, const int32_t *n_child, const float *node_stats,
                     const double *curr_reward /* [B] */, int32_t *out /* [B] */, void *stream);
int tm_distpy_backup(int n_trees, int n_nodes, int bins, const int32_t *trace, const int32_t *trace_len, int max_trace,
                     float *node_stats, float *node_dist, const double *r /* [B] */, const float *leaf_dist /* [B][bins] */,
                     double vmin, double vmax, float *scratch, void *stream);

/* The optimiser step of the online fit, model/yogi.py:39-90 (Yogi: lr, betas, eps, coupled weight decay) over FLAT device buffers:
 * p (parameters), g (gradients), m / v (exp_avg / exp_avg_sq), n floats each; state = 8 doubles on the device, zero before the first
 * step ([0] the step count, [1] [2] beta^t, [3] lr / (1 - beta1^t), [4] sqrt(1 - beta2^t): advanced on the device, so that the call is
 * the same two launches every time and can be captured in a HIP graph).  Per element the reference's operations in its order, fp32,
 * no contraction; step 1 sets exp_avg = 0, exp_avg_sq = g * g first (yogi.py:62-66).  Replaces the per-tensor loop of
 * Yogi.step (12 parameters x 8 launches). */
int tm_yogi_step(float *p, const float *g, float *m, float *v, double *state, int n, double lr, double beta1, double beta2,
                 double eps, double weight_decay, void *stream);
/* torch.optim.Adam's step (torch 2.10, single tensor, not capturable: exp_avg.lerp_, exp_avg_sq.mul_().addcmul_(), maximum,
 * (sqrt / bias_correction2_sqrt).add_(eps), addcdiv_(value=-step_size)) over FLAT device buffers, fp32 per element in that order,
 * with coupled weight decay and, when amsgrad != 0, the running maximum vmax of exp_avg_sq (vmax is not touched otherwise).
 * state: the five doubles of tm_yogi_step, advanced by the same one-thread kernel in front.  beta1 must exceed 0.5 (lerp's other
 * branch is not implemented). */
int tm_adam_step(float *p, const float *g, float *m, float *v, float *vmax, double *state, int n, double lr, double beta1,
                 double beta2, double eps, double weight_decay, int amsgrad, void *stream);
/* The gradient step of the value net's online fit (csrc/valuenet_fit.hip): forward of model.Net, train.batch_loss and the gradient
 * of its MEAN with respect to the ten learnable tensors, for the minibatch rows idx[0 .. batch) of the training set (idx NULL: rows
 * 0 .. batch-1; repeats allowed; every entry must be a valid row - the caller checks).  params / grad: 478338 floats in
 * model.PARAM_ORDER (Yogi's flat p / g buffers as they stand); out_bounds: out_ubound[2], out_lbound[2]; states int8 [rows][200];
 * value / variance / weight fp32 [rows] (weight read only when weighted != 0).  grad is OVERWRITTEN; loss = {mean, population std} of
 * the per-sample losses.  workspace: tm_valuenet_fit_workspace(batch) floats, 16-byte aligned, no initial contents required.
 * Everything is enqueued on `stream` in a sequence of launches whose shapes depend on `batch` alone: no allocation, no host
 * synchronisation, nothing read back - capturable in a HIP graph.  Deterministic (no atomics; fixed-order partial sums).
 * hipErrorInvalidValue, and nothing launched, for a NULL pointer (idx excepted), batch < 1 or batch > 2^20.
 * tm_valuenet_fit_workspace is host arithmetic only (callable without a GPU): -1 for a batch that is refused. */
long long tm_valuenet_fit_workspace(int batch);
int tm_valuenet_fit_grad(const float *params, const float *out_bounds, const int8_t *states, const float *value,
                         const float *variance, const float *weight, const int64_t *idx, int batch, int weighted,
                         float variance_clip, float *grad, float *loss, float *workspace, void *stream);
/* tm_valuenet_fit_grad on PACKED rows: obs is uint32 [rows][12], 4-byte aligned, the 48-byte observations of ENGINE_SPEC section 7 as the engine
 * harvests them (words 0..9: two board rows of 16 bits each, bit c of a row its column c; word 10: the four cell codes 10 r + c of
 * the falling piece; word 11: its low byte non-zero when the game has ended, which leaves no piece).  A cell is -1 where a code
 * names it, else its locked bit, exactly engine.h obs_cell; the kernels are those of tm_valuenet_fit_grad with the cell read through another
 * template argument and every later statement unchanged, so the outputs are bit-identical to tm_valuenet_fit_grad's on the rendered rows.
 * Any 48 bytes are safe to read: nothing taken out of an observation is used as an address - a code is only compared (codes >= 200
 * name no cell) and bits 10..15 of a row are ignored.  Every other argument, the workspace (tm_valuenet_fit_workspace, unchanged), the
 * argument checks and the return codes are the int8 twin's; a misaligned obs is hipErrorInvalidValue too. */
int tm_valuenet_fit_grad_packed(const float *params, const float *out_bounds, const uint32_t *obs, const float *value,
                                const float *variance, const float *weight, const int64_t *idx, int batch, int weighted,
                                float variance_clip, float *grad, float *loss, float *workspace, void *stream);
/* The gradient step of the distributional head's online fit (csrc/distnet_fit.hip): forward of model_distributional.Net,
 * Model_Dist.loss and the gradient of its MEAN with respect to the eight learnable tensors, for the minibatch rows idx[0 .. batch)
 * (idx NULL: rows 0 .. batch-1; repeats allowed; every entry must be a valid row - the caller checks).  params / grad:
 * TM_DISTNET_PARAMS(atoms) floats in model_distributional.PARAM_ORDER (FusedAdam's flat p / g buffers as they stand), 16-byte
 * aligned; states int8 [rows][200]: the 20 visible rows (the kernels put the net's two empty rows on top); target fp32
 * [rows][target_stride], the first `atoms` of a row used, every value finite and >= 0 (a row need not sum to 1: the logit gradient
 * is (w / batch) (p sum t - t)); weight fp32 [rows] (read only when weighted != 0).  grad is OVERWRITTEN; loss = {mean, sample
 * standard deviation (n - 1; NaN for batch 1, as torch.std_mean)} of the per-sample losses w sum_a (t log t - t log p).
 * workspace: tm_distnet_fit_workspace(batch, atoms) floats, 16-byte aligned, no initial contents required.  Everything is enqueued
 * on `stream` in a sequence of launches whose shapes depend on `batch` and `atoms` alone: no allocation, no host synchronisation,
 * nothing read back - capturable in a HIP graph.  Deterministic (no atomics; fixed-order partial sums).  hipErrorInvalidValue, and
 * nothing launched, for a NULL pointer (idx excepted), batch < 1 or > 2^20, atoms outside 1..64 or target_stride < atoms.
 * tm_distnet_fit_workspace is host arithmetic only (callable without a GPU): -1 for arguments that are refused. */
long long tm_distnet_fit_workspace(int batch, int atoms);
int tm_distnet_fit_grad(const float *params, const int8_t *states, const float *target, int target_stride, const float *weight,
                        const int64_t *idx, int batch, int atoms, int weighted, float *grad, float *loss, float *workspace,
                        void *stream);
/* tm_distnet_fit_grad on PACKED rows: obs is uint32 [rows][12], 4-byte aligned, the 48-byte observations of ENGINE_SPEC section 7 as the engine
 * harvests them (words 0..9: two board rows of 16 bits each, bit c of a row its column c; word 10: the four cell codes 10 r + c of
 * the falling piece; word 11: its low byte non-zero when the game has ended, which leaves no piece).  A cell is -1 where a code
 * names it, else its locked bit, exactly engine.h obs_cell; the kernels are those of tm_distnet_fit_grad with the cell read through another
 * template argument and every later statement unchanged, so the outputs are bit-identical to tm_distnet_fit_grad's on the rendered rows.
 * Any 48 bytes are safe to read: nothing taken out of an observation is used as an address - a code is only compared (codes >= 200
 * name no cell) and bits 10..15 of a row are ignored.  Every other argument, the workspace (tm_distnet_fit_workspace, unchanged), the
 * argument checks and the return codes are the int8 twin's; a misaligned obs is hipErrorInvalidValue too. */
int tm_distnet_fit_grad_packed(const float *params, const uint32_t *obs, const float *target, int target_stride,
                               const float *weight, const int64_t *idx, int batch, int atoms, int weighted, float *grad,
                               float *loss, float *workspace, void *stream);
/* The validation pass of the value net's online fit (csrc/valuenet_fit.hip): the forward and the per-sample losses of
 * tm_valuenet_fit_grad (the same kernels with idx NULL, the same statements for the loss) over the n held-out rows, reduced per chunk
 * of `chunk` rows to what train.validation_loss collects: rows_out[c] = {w, mean, std} in double for the rows c*chunk up to
 * min(n, (c+1)*chunk) - w the sum of their weights when weighted != 0, else their count; mean and population std (0 for one row)
 * of their losses, the weight multiplied in when weighted != 0.  rows_out: ceil(n / chunk) x 3 doubles.  With n == chunk == slab the
 * (float) of mean and std are the bits of the gradient step's loss[0], loss[1] on the same rows.  params, out_bounds, states, value,
 * variance, weight: as for the gradient step, n rows of each.  The rows are forwarded `slab` at a time (slab >= chunk >= 1, a
 * multiple of chunk, at most 2^20); the result does not depend on slab.  workspace: tm_valuenet_fit_validate_workspace(slab) floats
 * (a function of slab alone, never of n), 16-byte aligned, no initial contents required.  Everything is enqueued on `stream`: no
 * allocation, no host synchronisation, nothing read back, nothing written outside rows_out and the workspace.  Deterministic (no
 * atomics; one workgroup per chunk adds in double in the order of the gradient step's loss).  hipErrorInvalidValue, and nothing
 * launched, for a NULL pointer, n < 1, a chunk or slab that is refused, or a misaligned workspace.
 * tm_valuenet_fit_validate_workspace is host arithmetic only (callable without a GPU): -1 for a slab that is refused. */
long long tm_valuenet_fit_validate_workspace(int slab);
int tm_valuenet_fit_validate(const float *params, const float *out_bounds, const int8_t *states, const float *value,
                             const float *variance, const float *weight, long long n, int chunk, int slab, int weighted,
                             float variance_clip, double *rows_out, float *workspace, void *stream);
/* tm_valuenet_fit_validate on packed rows (obs uint32 [n][12], 4-byte aligned): as tm_valuenet_fit_grad_packed is to its twin - the
 * same kernels reading the cell from the observation, rows_out bit-identical to the int8 call's on the rendered rows, any 48 bytes
 * safe to read, every other argument, check and return code unchanged, workspace tm_valuenet_fit_validate_workspace(slab). */
int tm_valuenet_fit_validate_packed(const float *params, const float *out_bounds, const uint32_t *obs, const float *value,
                                    const float *variance, const float *weight, long long n, int chunk, int slab, int weighted,
                                    float variance_clip, double *rows_out, float *workspace, void *stream);
/* The Fisher pass of the value net's fit (csrc/valuenet_fit.hip): fisher[i] = (1/n) sum_b (d loss_b / d p_i)^2 over the rows idx[0 .. n)
 * (idx NULL: rows 0 .. n-1; repeats allowed; every entry must be a valid row - the caller checks), loss_b the per-sample loss of
 * tm_valuenet_fit_grad (the weight multiplied in when weighted != 0), i over the 478338 floats of params: the empirical Fisher diagonal
 * at the targets the fit used.  The rows are taken `slab` at a time (1 .. 2^20): per slab the gradient step's forward, its output layer
 * with per-sample scale w (not w / batch) and its data-gradient kernels as they are, and the squared forms of its weight-gradient
 * kernels (fc1: the product of the squared operands; the convolutions: the square of each sample's sum over positions); the slab's sums
 * go through the gradient step's second stages into a temporary and from there into a double accumulator, slab after slab in stream
 * order; after the last slab fisher = (float)(accumulator / n).  No atomics: every sum is in a fixed order that follows from (n, slab)
 * alone, and a slab >= n gives the bits of slab == n.  fisher is OVERWRITTEN, never read.  workspace: tm_valuenet_fit_fisher_workspace(slab)
 * floats = tm_valuenet_fit_workspace(slab) + 478340 (the temporary) + 956676 (the accumulator), 16-byte aligned, no initial contents
 * required.  Everything is enqueued on `stream`: no allocation, no host synchronisation, nothing read back.  hipErrorInvalidValue, and
 * nothing launched, for a NULL pointer (idx excepted), n < 1, a slab that is refused or a misaligned workspace.
 * tm_valuenet_fit_fisher_workspace is host arithmetic only (callable without a GPU): -1 for a slab that is refused. */
long long tm_valuenet_fit_fisher_workspace(int slab);
int tm_valuenet_fit_fisher(const float *params, const float *out_bounds, const int8_t *states, const float *value,
                           const float *variance, const float *weight, const int64_t *idx, long long n, int slab, int weighted,
                           float variance_clip, float *fisher, float *workspace, void *stream);
/* tm_valuenet_fit_fisher on packed rows (obs uint32 [rows][12], 4-byte aligned): as tm_valuenet_fit_grad_packed is to its twin - fisher
 * bit-identical to the int8 call's on the rendered rows, any 48 bytes safe to read, a misaligned obs hipErrorInvalidValue. */
int tm_valuenet_fit_fisher_packed(const float *params, const float *out_bounds, const uint32_t *obs, const float *value,
                                  const float *variance, const float *weight, const int64_t *idx, long long n, int slab, int weighted,
                                  float variance_clip, float *fisher, float *workspace, void *stream);
/* The penalty of elastic weight consolidation over FLAT device buffers of n floats (csrc/yogi.hip): the loss gains
 * 0.5 lambda sum_i F[i] (p[i] - anchor[i])^2 and the gradient lambda F[i] (p[i] - anchor[i]).  Per element, in float, no contraction,
 * in this order: d = p - anchor, t = ((float)lambda F) d, grad = grad + t (grad is ADDED to).  loss[0] (one double on the device) =
 * 0.5 lambda sum F d d in double, F and the float d converted first, summed in two fixed-order stages through the workspace
 * (tm_ewc_penalty_workspace(n) floats, 16-byte aligned, no initial contents required).  Two launches on `stream`, no atomics, no host
 * synchronisation: capturable in a HIP graph.  hipErrorInvalidValue, and nothing launched, for a NULL pointer, n < 1, a lambda that is
 * negative or not finite, a misaligned workspace or loss.  tm_ewc_penalty_workspace is host arithmetic only: -1 for n < 1. */
long long tm_ewc_penalty_workspace(int n);
int tm_ewc_penalty(const float *p, const float *anchor, const float *fisher, int n, double lambda, float *grad, double *loss,
                   float *workspace, void *stream);
/* The validation pass of the distributional head's online fit (csrc/distnet_fit.hip): as the value net's above, with the forward and
 * the per-sample losses of tm_distnet_fit_grad.  rows_out[c] = {w, mean, std}: std is the sample standard deviation (n - 1; NaN for
 * a chunk of one row, as torch.std_mean - train's host loop maps it to 0).  params (16-byte aligned), states, target, target_stride,
 * weight, atoms: as for the gradient step, n rows of each.  workspace: tm_distnet_fit_validate_workspace(slab, atoms) floats, 16-byte
 * aligned.  hipErrorInvalidValue, and nothing launched, for a NULL pointer, n < 1, a chunk or slab that is refused, atoms outside
 * 1..64, target_stride < atoms, or a misaligned workspace.  The workspace function is host arithmetic only: -1 when refused. */
long long tm_distnet_fit_validate_workspace(int slab, int atoms);
int tm_distnet_fit_validate(const float *params, const int8_t *states, const float *target, int target_stride, const float *weight,
                            long long n, int chunk, int slab, int atoms, int weighted, double *rows_out, float *workspace,
                            void *stream);
/* tm_distnet_fit_validate on packed rows (obs uint32 [n][12], 4-byte aligned): as tm_distnet_fit_grad_packed is to its twin - the
 * same kernels reading the cell from the observation, rows_out bit-identical to the int8 call's on the rendered rows (the NaN of a
 * one-row chunk included), any 48 bytes safe to read, every other argument, check and return code unchanged, workspace
 * tm_distnet_fit_validate_workspace(slab, atoms). */
int tm_distnet_fit_validate_packed(const float *params, const uint32_t *obs, const float *target, int target_stride,
                                   const float *weight, long long n, int chunk, int slab, int atoms, int weighted,
                                   double *rows_out, float *workspace, void *stream);
/* The Fisher pass of the distributional head's fit (csrc/distnet_fit.hip): fisher[i] = (1/n) sum_b (d loss_b / d p_i)^2 over the rows
 * idx[0 .. n) (idx NULL: rows 0 .. n-1; repeats allowed; every entry must be a valid row - the caller checks), loss_b the per-sample loss
 * of tm_distnet_fit_grad, w_b sum_a (t log t - t log p) with w_b = 1 when weighted == 0, i over the P = TM_DISTNET_PARAMS(atoms) =
 * 279232 + 129 atoms floats of params: the empirical Fisher diagonal at the targets the fit used.  The rows are taken `slab` at a time
 * (1 .. 2^20): per slab the gradient step's forward, its output layer with the divisor 1 (not batch) and its data-gradient kernels as
 * they are, and the squared forms of its weight-gradient kernels (the FC layers: the product of the squared operands; the convolutions:
 * the square of each sample's sum over positions); the slab's sums go through the gradient step's second stages into a temporary and
 * from there into a double accumulator, slab after slab in stream order; after the last slab fisher = (float)(accumulator / n).  No
 * atomics: every sum is in a fixed order that follows from (n, slab, atoms) alone, and a slab >= n gives the bits of slab == n.  fisher
 * is OVERWRITTEN, never read.  workspace: tm_distnet_fit_fisher_workspace(slab, atoms) floats = tm_distnet_fit_workspace(slab, atoms)
 * + up4(P) (the temporary) + up4(2 P) (the accumulator), up4 rounding up to a multiple of four; 16-byte aligned, no initial contents
 * required.  Everything is enqueued on `stream`: no allocation, no host synchronisation, nothing read back.  hipErrorInvalidValue, and
 * nothing launched, for a NULL pointer (idx excepted), n < 1, slab < 1 or > 2^20, atoms outside 1..64, target_stride < atoms, or a
 * misaligned workspace or params.  tm_distnet_fit_fisher_workspace is host arithmetic only (callable without a GPU): -1 when refused. */
long long tm_distnet_fit_fisher_workspace(int slab, int atoms);
int tm_distnet_fit_fisher(const float *params, const int8_t *states, const float *target, int target_stride, const float *weight,
                          const int64_t *idx, long long n, int slab, int atoms, int weighted, float *fisher, float *workspace,
                          void *stream);
/* tm_distnet_fit_fisher on packed rows (obs uint32 [rows][12], 4-byte aligned): as tm_distnet_fit_grad_packed is to its twin - fisher
 * bit-identical to the int8 call's on the rendered rows, any 48 bytes safe to read, a misaligned obs hipErrorInvalidValue. */
int tm_distnet_fit_fisher_packed(const float *params, const uint32_t *obs, const float *target, int target_stride,
                                 const float *weight, const int64_t *idx, long long n, int slab, int atoms, int weighted,
                                 float *fisher, float *workspace, void *stream);
/* value network forward (model/model_vv.py:13-52; Model_VV.inference 210-217): states int8 [n][200] -> v[n], var[n].
 * params: 478342 floats in PyTorch state_dict layouts (order as in oracle/valuenet_oracle.c).
 * It runs in one of three modes (backend, fc1), checked by tm_valuenet_check_mode (host arithmetic only: 0, or
 * hipErrorInvalidValue for any other pair) before anything else in every call that takes them:
 *   (TM_VALUENET_FP32, TM_VALUENET_FC1_FP32)      fp32 matrix cores; bit-identical to tm_valuenet_forward_plain by construction;
 *   (TM_VALUENET_BF16X3, TM_VALUENET_FC1_FP32)    valuenet_x3.inc (numerics contract in DESIGN.md section 3.3): conv2 and conv3 on
 *       the bf16 matrix cores, every operand split into three bf16 planes, six plane products per fp32 product, fp32 accumulation;
 *       conv1, fc1 and the output layer as in fp32.  Within 1e-4 of the reference, not bit-equal to the fp32 mode;
 *   (TM_VALUENET_BF16X3, TM_VALUENET_FC1_BF16X3)  valuenet_fc1_x3.inc, k_vn_fc1_x3: fc1's weights and its input as three bf16 planes
 *       as well, six plane products per step of 32 k, fp32 accumulation from the bias.  Not bit-equal to the mode above.
 * In every mode a state's outputs depend on that state only.
 * tm_valuenet_prepare re-lays the weights for a mode (call after every weight change) into ONE buffer of
 * TM_VALUENET_PREPARED_TOTAL(backend, fc1) floats: the fp32 MFMA operand streams of conv2 / conv3 / fc1 (always), then the
 * convolutions' planes (TM_VALUENET_BF16X3), then fc1's planes (TM_VALUENET_FC1_BF16X3).  It writes exactly the parts the mode
 * names, so a buffer prepared for a larger mode serves every smaller one.  prepared == NULL: hipErrorInvalidValue.
 * The forwards take that buffer and n x TM_VALUENET_SCRATCH_MFMA floats of scratch; n <= 0: nothing to do, 0. */
int tm_valuenet_check_mode(int backend, int fc1);
int tm_valuenet_prepare(const float *params, float *prepared, int backend, int fc1, void *stream);
int tm_valuenet_forward(const float *params, const float *prepared, int backend, int fc1, const int8_t *states, int n, float *v,
                        float *var, float *scratch, void *stream);
/* evaluate the tree engine's pending requests (s->eval_obs) and write s->eval_v / s->eval_var; the packed
 * observations are rendered inside the first kernel (no int8 staging).  scratch: G*eval_slots x TM_VALUENET_SCRATCH_MFMA */
int tm_valuenet_forward_requests(const float *params, const float *prepared, int backend, int fc1, const tm_store *s,
                                 float *scratch, void *stream);
/* the one-thread-per-output form with the fp32 mode's fma-chain numerics (scratch: n x TM_VALUENET_SCRATCH floats) */
int tm_valuenet_forward_plain(const float *params, const int8_t *states, int n, float *v, float *var, float *scratch,
                              void *stream);
/* How the matrix-core path's fc1 kernel deals its work (host arithmetic only, callable without a GPU; the kernel and its
 * launch use the same formula): `requests` states make ceil(requests / rows) tiles of `parts` parts each; the items (tile,
 * part) are numbered tiles fastest, a tile's parts a multiple of eight apart (valuenet.hip fc1_item: workgroups go to the XCDs
 * round robin); workgroup b of `grid` takes items b, b + grid, ...  Writes the workgroup's (tile, part) pairs to
 * items[0 .. 2 * cap) and returns how many it takes (possibly more than cap); -1 on arguments that make no grid. */
int tm_fc1_deal(int requests, int rows, int parts, int grid, int b, int32_t *items, int cap);
/* The fp32 mode's requests at the single-leaf shape (fewer than 8 192 request slots) run as ONE launch, k_vn_conv_fc1: the
 * convolutions, then fc1 on the same resident workgroups, a tile of 32 states handed over through a ready counter in the scratch
 * rows' padding (TM_VALUENET_SCRATCH_MFMA).  The two kernels remain for everything else, where the chip refuses the launch's LDS
 * or residency, and under TM_VALUENET_FUSED=0 in the environment (read once; 1 asks for the one launch; for A/B runs and tests).
 * A poller's wait is bounded (10 ms): when it runs out the kernel sets a sticky error word and leaves.
 * tm_fused_tile_rows: host arithmetic only - the count tile `tile`'s poller waits for at `requests` requests (32, the remainder
 * in the last tile, 0 past it; -1 on negative arguments).
 * tm_valuenet_forward_requests_grid: tm_valuenet_forward_requests with the path named, for tests - grid > 0: k_vn_conv_fc1 on
 * `grid` workgroups (hipErrorInvalidValue above what is resident, or where the launch does not serve), 0: on its own grid, < 0: the
 * two kernels.
 * tm_valuenet_forward_requests_run: tm_valuenet_forward_requests for a caller that issues a run of evaluations on one scratch and
 * stream with nothing else writing the scratch in between (tm_search_run within a move): *run = -1 before the first, the library
 * keeps it.  It spares the clear of the launch's ready words that every other call puts in front of the one launch.
 * tm_valuenet_fused_error: the sticky error word, one a process whatever the handle or device, to be read after a synchronisation:
 * tm_search_run reads it at every synchronisation of a move and fails with hipErrorLaunchTimeOut; a caller of
 * tm_valuenet_forward_requests reads it itself once the stream is idle, before it uses eval_v / eval_var (Model_VV.inference_requests
 * leaves that to its caller as well).  reset != 0 clears it. */
int tm_fused_tile_rows(int requests, int tile);
int tm_valuenet_forward_requests_grid(const float *params, const float *prepared, int backend, int fc1, const tm_store *s,
                                      float *scratch, void *stream, int grid);
int tm_valuenet_forward_requests_run(const float *params, const float *prepared, int backend, int fc1, const tm_store *s,
                                     float *scratch, void *stream, int32_t *run);
int tm_valuenet_fused_error(int reset);
/* the states k_vn_conv takes in one round: its resident waves (two workgroups of four waves a compute unit); <= 0: no device */
int tm_valuenet_resident_states(void);
/* The request cap's arithmetic (host only, callable without a GPU; the kernels use the same formulas).  counts[segs] = the
 * entries of the dense list's segments; a launch serves the first min(sum, cap) dense positions (cap == 0: all), counted
 * through the segments cyclically from segment rot.  tm_request_served: served[s] = the entries of segment s among them
 * (what k_vn_conv writes to tm_store::eval_served); returns their number.  tm_request_at: dense position p -> out = (segment,
 * entry within it, index into eval_list at `slots` request slots a game); returns 0.  -1 on arguments that make no list. */
int tm_request_served(const int32_t *counts, int segs, int rot, int cap, int32_t *served);
int tm_request_at(const int32_t *counts, int segs, int rot, int slots, int p, int32_t *out);

/* distributional value head (model/model_distributional.py:18-57 `Net`, Model_Dist.inference :100-107), the leaf evaluator
 * of TM_KIND_DIST: states int8 [n][200] (the 20 visible rows; the net's two extra rows on top are empty) -> softmax over
 * `atoms` (<= 64) bins, dist[i * dist_stride + b].  params: TM_DISTNET_PARAMS(atoms) floats in PyTorch state_dict order and
 * layouts.  `backend` (any other value: hipErrorInvalidValue):
 *   TM_VALUENET_FP32    fp32 matrix cores, one k-ordered fma chain per pre-activation (oracle/distnet_oracle.c computes the same bits);
 *   TM_VALUENET_BF16X3  distnet_x3.inc (numerics contract in DESIGN.md section 3.8): conv2 on the bf16 matrix cores, every operand
 *       split into three bf16 planes, six plane products per fp32 product, fp32 accumulation; conv1, fc1, fc_v and the softmax as
 *       in fp32.  Within 1e-6 relative of the reference's Net, not bit-equal to the fp32 backend.
 * A state's outputs depend on that state only.  tm_distnet_prepare re-lays the weights (after every weight change) into ONE
 * buffer of TM_DISTNET_PREPARED_TOTAL(backend) floats: the fp32 operand streams of conv2 / fc1 (always), then conv2's planes
 * (TM_VALUENET_BF16X3); a buffer prepared for TM_VALUENET_BF16X3 serves both backends.  prepared == NULL: hipErrorInvalidValue.
 * scratch: n x TM_DISTNET_SCRATCH floats, no initial contents required. */
int tm_distnet_prepare(const float *params, float *prepared, int backend, void *stream);
int tm_distnet_forward(const float *params, const float *prepared, int backend, const int8_t *states, int n, int atoms,
                       float *dist, int dist_stride, float *scratch, void *stream);
/* the tree engine's pending requests (TM_KIND_DIST: s->eval_obs[g] = the leaf NODE of game g, rendered from its packed game
 * inside the first kernel) -> s->eval_dist[g][0 .. dist_bins); scratch: n_games x TM_DISTNET_SCRATCH floats */
int tm_distnet_forward_requests(const float *params, const float *prepared, int backend, const tm_store *s, float *scratch,
                                void *stream);

const char *tm_version(void);
/* sizeof(tm_store) and a few offsets, so a host mirror of the struct can be checked without a GPU */
int tm_store_layout(int *out, int n);
#ifdef __cplusplus
}
#endif
#endif
