"""How many evaluation requests every launch of the headline workload posts: the benchmark's games (bench.py's seeds, pool and
agent arguments) played through a launch loop driven from here - tm_sim_step, read the dense list's segment counters
(tm_store::eval_cnt under the launch's parity, summed on the device, no host synchronisation), tm_valuenet_forward_requests - so
that launch i of move m here is launch i of move m of `bench.py` (per-game results do not depend on who drives the loop, and
neither run of the first 25 moves has a catch-up launch: the script checks its own).  Joined with a rocprofv3 kernel trace of the
benchmark by scripts/request_cap_histogram.py.

    python scripts/request_counts.py [--games 4096] [--sims 500] [--moves 25] --out counts.json"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tetris_mcts_amd import agents, store as st, dist as tdist  # noqa: E402
from tetris_mcts_amd.model import Model_VV  # noqa: E402
from tetris_mcts_amd.pyTetris import Tetris  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=4096)
ap.add_argument("--sims", type=int, default=500)
ap.add_argument("--moves", type=int, default=25)
ap.add_argument("--max-nodes", type=int, default=100000)
ap.add_argument("--out", required=True)
a = ap.parse_args()
G, sims = a.games, a.sims
env_args = ((20, 10), 1, 0, 0)
model = Model_VV(backend="hip", seed=0)
game = Tetris(*env_args, seed=tdist.game_seeds(20260925, G, 0), n_games=G)
agent = agents.ValueSim(sims=sims, env=Tetris, env_args=env_args, n_games=G, max_nodes=a.max_nodes, model=model, online=False,
                        n_sub=1, ev_every=0, gc_slice_cycles=150000)
agent.update_root(game)
s = agent.store
segs = min(G, 64)
cnt = s.t["eval_cnt"]
log = torch.zeros(a.moves, sims + 1, dtype=torch.int32, device=s.device)
flags = st.SIM_BACKUP | st.SIM_FRONT | st.SIM_EVAL_NEEDED
catchup = []
for m in range(a.moves):
    s.s.eval_epoch = int(model.weights_epoch)
    s.move_begin(sims)
    s.sim_step(flags)
    log[m, 0] = cnt[:segs, s.s.eval_parity].sum()
    for i in range(sims):
        model.inference_requests(s)
        s.sim_step(flags)
        log[m, i + 1] = cnt[:segs, s.s.eval_parity].sum()
    todo, collecting = s.sims_remaining()
    catchup.append(todo)
    while todo or collecting:       # (not expected in the first moves: pools of 100 000 nodes are far from full)
        if collecting:
            for _ in range(6):
                s.gc_step()
        else:
            for _ in range(todo):
                model.inference_requests(s)
                s.sim_step(flags)
        todo, collecting = s.sims_remaining()
    act = agent.get_action()
    game.play(act)
    agent.update_root(game)
    if np.atleast_1d(game.end).any():
        game.reset("ended")
        agent.update_root(game)
torch.cuda.synchronize()
counts = log.cpu().numpy()
doc = {"posted_by_the_launch_after_the_last_simulation": int(counts[:, sims].sum()),      # (0: it only backs up)
"what": "requests posted per launch: counts[m][i] = what evaluator launch i of move m + 1 serves",
       "games": G, "sims": sims, "moves": a.moves, "max_nodes": a.max_nodes, "catchup_launches_by_move": catchup,
       "n_eval": s.counter("N_EVAL"), "error_games": int((s.errors() != 0).sum().item()),
       "counts": counts[:, :sims].tolist()}
doc["counted"] = int(counts.sum())      # (= n_eval: every posted request is on the list)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f)
print("moves %d: mean requests per launch by move %s" % (a.moves, [int(round(x)) for x in counts[:, :sims].mean(axis=1)]), flush=True)
