#!/usr/bin/env python
"""What root-distribution records and DistValueSim's re-analysis cost (profiles/root_dists_timing.json).

    python scripts/root_dists_timing.py [--parent DIR] [--runs 3] [--sims 1000] [--only a|b] [--out FILE]

The protocol of scripts/reanalyse_timing.py (and, through it, the child process and time stamps of
scripts/episode_recording_timing.py): every figure is the median of --runs fresh processes, the variants alternating.
  (a) ms per move of play.py --agent_type DistValueSim --mcts_sims SIMS --min_visit 50 --n_games 4096 --max_moves 200 --ngames 100000000
      with --save --save_root_dists, with --save alone and, with --parent DIR (a built checkout of the parent commit), with --save
      there; the margin is the spread max - min of the baseline's runs.  Every run plays its 200 moves: the 64-move ring is flushed
      at moves 64, 128 and 192, inside the moves timed (after the first 20); the script refuses a run that played fewer.
      With --records (and --parent) the variants are two, this tree and the parent, both with --save --save_positions
      --save_root_dists: the recorder's host path against the parent's.
  (b) re-analysis under DistValueSim at 4096 x 100: a child records 10 moves (positions and root distributions) with a DistValueSim
      whose pool is re-analysis' default (reanalyse.default_max_nodes), then re-analyses two batches of 4096 of the recorded
      positions with it: ms per batch between HIP events, split into upload + load + check, tm_pool_fresh, new roots + search + root
      statistics, and re-record (both tables) + copy."""
import argparse
import importlib.util
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location("tm_" + name, os.path.join(HERE, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def play_args(sims):
    return ["--agent_type", "DistValueSim", "--mcts_sims", str(sims), "--min_visit", "50", "--n_games", "4096", "--max_moves", "200",
            "--ngames", "100000000"]


def part_a(runs, parent, sims, timeout, records=False):
    one = _script("episode_recording_timing").one
    variants = [("save_root_dists", HERE, ["--save", "--save_root_dists"]), ("save", HERE, ["--save"])]
    if parent:
        variants.append(("parent_save", os.path.abspath(parent), ["--save"]))
    if records:
        variants = [(name, repo, ["--save", "--save_positions", "--save_root_dists"])
                    for name, repo in (("records", HERE), ("parent_records", os.path.abspath(parent)))]
    res = {name: [] for name, _, _ in variants}
    for i in range(runs):
        for name, repo, flags in variants:
            tmp = tempfile.mkdtemp(prefix="root_dists_")
            try:
                r = one(repo, 20, play_args(sims) + flags + ["--save_dir", tmp + "/"], timeout)
                if r["moves"] != 200:
                    raise RuntimeError("%s played %d moves, not 200: no flush inside the timed moves" % (name, r["moves"]))
                r["bytes_written"] = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
            res[name].append(r)
            print(name, i, json.dumps(r), flush=True)
    base = variants[-1][0] if parent else "save"
    med = {name: statistics.median(r["ms_per_move"] for r in rs) for name, rs in res.items()}
    return dict(command="play.py " + " ".join(play_args(sims)), flags={name: flags for name, _, flags in variants}, skip_moves=20,
                runs=res, median_ms_per_move=med, baseline=base,
                margin_ms=max(r["ms_per_move"] for r in res[base]) - min(r["ms_per_move"] for r in res[base]),
                **{name + "_minus_baseline_ms": med[name] - med[base] for name in med if name != base or not parent})


def child_b(sims, n_games, moves):
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from tetris_mcts_amd.agents import DistValueSim
    from tetris_mcts_amd.episodes import EpisodeRecorder, RootDistLoader
    from tetris_mcts_amd.model_distributional import Model_Dist
    from tetris_mcts_amd.pyTetris import Tetris
    from tetris_mcts_amd.reanalyse import Reanalyser, default_max_nodes
    stages = _script("reanalyse_timing").STAGES
    env_args = ((20, 10), 1, 0, 0)
    tmp = tempfile.mkdtemp(prefix="root_dists_timing_")
    out = dict(sims=sims, n_games=n_games)
    try:
        game = Tetris(*env_args, seed=0, n_games=n_games)
        agent = DistValueSim(sims=sims, env=Tetris, env_args=env_args, n_games=n_games, online=False,
                             model=Model_Dist(atoms=50, backend="hip", seed=0), max_nodes=default_max_nodes(sims))
        agent.update_root(game)
        rec = EpisodeRecorder(tmp + "/", "data", 0, n_games, ring_moves=8)
        rec.record_positions()
        rec.record_root_dists(agent.atoms, *agent.vrange)
        for _ in range(moves):
            action = agent.play()
            rec.add(agent, game)
            game.play(action)
            rec.advance(game)
            agent.update_root(game)
            if np.atleast_1d(game.end).any():
                game.reset("ended")
                agent.update_root(game)
        rec.close()
        L = RootDistLoader(tmp + "/data0")
        lo = 2 * n_games                                   # (the positions of moves 2 and 3: 4096 different games each)
        R = Reanalyser(agent, Tetris(*env_args, seed=1, n_games=n_games))
        R.submit(L.rows[:n_games], L.positions[:n_games])  # warm-up: buffers, the search handle
        R.collect()
        R.timing = {}
        for k in range(2):
            a = lo + k * n_games
            R.submit(L.rows[a:a + n_games], L.positions[a:a + n_games])
            R.collect()
        torch.cuda.synchronize()
        t = R.timing
        per = [{name: t[x][k].elapsed_time(t[y][k]) for name, x, y in stages} for k in range(2)]
        out.update(max_nodes=agent.max_nodes, batches=per,
                   ms_per_batch=statistics.mean(t["start"][k].elapsed_time(t["rerecorded"][k]) for k in range(2)),
                   **{name: statistics.mean(p[name] for p in per) for name, _, _ in stages})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("TIMING " + json.dumps(out))


def part_b(runs, timeout):
    res = []
    for i in range(runs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child_b", "100"], capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            raise RuntimeError("run failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        res.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TIMING ")][-1][7:]))
        print(i, json.dumps(res[-1]), flush=True)
    keys = ("ms_per_batch", "load_check", "pool_fresh", "search", "rerecord")
    return dict(shape="4096x100", runs=res, median=dict({k: statistics.median(r[k] for r in res) for k in keys}, max_nodes=res[0]["max_nodes"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child_b", type=int, default=0)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sims", type=int, default=1000, help="simulations a move in (a): 1000 is DistValueSim's benchmark batch")
    ap.add_argument("--only", choices=("a", "b"), default=None)
    ap.add_argument("--records", action="store_true", help="(a) as a comparison of the recorder itself: this tree and --parent, both "
                    "with --save --save_positions --save_root_dists (profiles/records_refactor_timing.json)")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child_b:
        return child_b(a.child_b, 4096, 10)
    if a.records and not a.parent:
        ap.error("--records compares with the parent's recorder: it needs --parent")
    out = {}
    if a.only != "a":
        out["reanalysis"] = part_b(a.runs, a.timeout)
    if a.only != "b":
        out["recording"] = part_a(a.runs, a.parent, a.sims, a.timeout, a.records)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
