"""What the dense request path (TreeAgent's dense_requests / evaluator_pure, csrc/eval_requests.hip) gives an evaluator the engine
does not own, on one MI355X: ValueSimLP and ValueSim with Model_VV(backend="torch", seed=0) as the evaluator, today's padded path
against the dense path and the dense path with a pure evaluator, at several dense_pad.
    python scripts/bench_dense_requests.py [--games 4096] [--sims 100] [--pads 64,256,1024] [--blocks 3] [--block-moves 2]
                                           [--json profiles/dense_requests_timing.json]
Every variant is an agent of its own on a game of its own (same seeds); after a warm-up of --warmup moves each (which has seen the
batch shapes) the variants are alternated in blocks of --block-moves moves inside this one process, HIP events around whole moves.
Per variant: ms per simulation (median and every block), rows per simulation handed to the evaluator, the distinct batch shapes.
A batch shape the evaluator has not seen costs PyTorch seconds of set-up (MIOpen), so a small --pads entry makes the warm-up long.
Then, on a launch's real requests: gather + read-back + scatter alone against tm_eval_render alone, HIP events around 50 calls."""
import argparse, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tetris_mcts_amd import agents, store as st  # noqa: E402
from tetris_mcts_amd.model import Model_VV  # noqa: E402
from tetris_mcts_amd.pyTetris import Tetris  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=4096)
ap.add_argument("--sims", type=int, default=100)
ap.add_argument("--max-nodes", type=int, default=8000, help="node pool per game: large enough that no game collects in the run")
ap.add_argument("--pads", default="64,256,1024")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--block-moves", type=int, default=2)
ap.add_argument("--agents", default="ValueSimLP,ValueSim")
ap.add_argument("--json", default=os.path.join("profiles", "dense_requests_timing.json"))
args = ap.parse_args()
pads = [int(p) for p in args.pads.split(",")]
env_args = ((20, 10), 1, 0, 0)


class Variant:
    def __init__(self, name, label, **kw):
        self.label, self.kw = label, kw
        self.game = Tetris(*env_args, seed=20260925, n_games=args.games)
        self.agent = getattr(agents, name)(sims=args.sims, env=Tetris, env_args=env_args, n_games=args.games,
                                           max_nodes=args.max_nodes, model=Model_VV(backend="torch", seed=0), online=False, **kw)
        self.agent.update_root(self.game)
        self.rows, self.calls, self.shapes, self.block_ms = 0, 0, set(), []
        plain = self.agent.evaluate

        def counted(states, v_out, var_out):
            self.rows += int(states.shape[0])
            self.calls += 1
            self.shapes.add(int(states.shape[0]))
            return plain(states, v_out, var_out)
        self.agent.evaluate = counted

    def moves(self, n, timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = 0.0
        for _ in range(n):
            e0.record()
            self.agent.mcts(args.sims)
            e1.record()
            act = self.agent.get_action()
            torch.cuda.synchronize()
            ms += e0.elapsed_time(e1)
            self.game.play(act)
            self.agent.update_root(self.game)
        if timed:
            self.block_ms.append(ms / (n * args.sims))
        print("  %s: %d move(s), %.3f ms per simulation, %d batch shapes so far" % (self.label, n, ms / (n * args.sims), len(self.shapes)),
              flush=True)

    def parts(self, pad, reps=50):
        """a launch's real requests: us per (gather + read-back + scatter) and per tm_eval_render, and the requests"""
        a, s = self.agent, self.agent.store
        both = st.SIM_BACKUP | st.SIM_FRONT | (st.SIM_EVAL_NEEDED if a.evaluator_pure else 0)
        s.move_begin(4)
        s.sim_step(both)
        for _ in range(2):
            a.evaluate_requests()
            s.sim_step(both)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = {"slots": s.n_games * s.eval_slots, "requests": int((s.t["eval_obs"] != 0).sum().item())}
        for what in ("dense", "render"):
            for timed in (False, True):
                e0.record()
                for _ in range(reps):
                    if what == "dense":
                        states, _, n = s.gather_eval(pad)
                        s.scatter_eval(*s.dense_outputs(states.shape[0]))
                    else:
                        s.render_eval()
                e1.record()
                torch.cuda.synchronize()
            out[what + "_us"] = 1e3 * e0.elapsed_time(e1) / reps
        return out


result = {"games": args.games, "sims": args.sims, "max_nodes": args.max_nodes, "evaluator": "Model_VV(backend='torch', seed=0)",
          "protocol": "one process; %d warm-up moves per variant, then %d blocks of %d moves per variant, alternated; HIP events around "
                      "whole moves (agent.mcts)" % (args.warmup, args.blocks, args.block_moves),
          "device": torch.cuda.get_device_name(0), "agents": {}}
if os.path.exists(args.json):           # agents measured by an earlier call at the same size stay in the file
    with open(args.json) as f:
        prior = json.load(f)
    if (prior.get("games"), prior.get("sims")) == (args.games, args.sims):
        result["agents"] = prior.get("agents", {})
for name in args.agents.split(","):
    variants = [Variant(name, "padded")]
    for pad in pads:
        variants.append(Variant(name, "dense pad=%d" % pad, dense_requests=True, dense_pad=pad))
        variants.append(Variant(name, "dense+pure pad=%d" % pad, dense_requests=True, dense_pad=pad, evaluator_pure=True))
    for v in variants:
        v.moves(args.warmup, False)
        v.rows, v.calls = 0, 0
    for b in range(args.blocks):
        for v in variants:
            v.moves(args.block_moves, True)
    rows = {}
    for v in variants:
        assert not bool(v.agent.store.errors().any().item()) and v.agent.store.counter("N_GC") == 0
        sims_run = args.blocks * args.block_moves * args.sims
        rows[v.label] = {"ms_per_sim_median": statistics.median(v.block_ms), "ms_per_sim_blocks": v.block_ms,
                         "rows_per_sim": v.rows / sims_run, "evaluator_calls_per_sim": v.calls / sims_run,
                         "distinct_batch_shapes": len(v.shapes), "batch_shapes_min_max": [min(v.shapes), max(v.shapes)]}
        print(name, v.label, json.dumps(rows[v.label]), flush=True)
    parts = {}
    for v in variants:
        if v.kw.get("dense_pad") == 256:
            parts["pure" if v.kw.get("evaluator_pure") else "all children"] = v.parts(256)
    print(name, "parts", json.dumps(parts), flush=True)
    result["agents"][name] = {"dense_pads": pads, "blocks": args.blocks, "variants": rows, "gather_readback_scatter_vs_render": parts}
    del variants
    torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:       # (after every agent: a run cut short keeps what it measured)
        json.dump(result, f, indent=1)
        f.write("\n")
print("wrote", args.json)
