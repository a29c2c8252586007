#!/usr/bin/env python
"""What position records and re-analysis cost (profiles/reanalyse_timing.json).

    python scripts/reanalyse_timing.py [--parent DIR] [--runs 3] [--only a|b] [--out FILE]

The protocol of scripts/episode_recording_timing.py (whose child process and time stamps this script uses): every figure is the
median of --runs fresh processes, the variants alternating.
  (a) ms per move of play.py --agent_type ValueSim --mcts_sims 100 --n_games 4096 --max_moves 200 --ngames 100000000 with
      --save --save_positions, with --save alone and, with --parent DIR (a built checkout of the parent commit), with --save
      there; the margin is the spread max - min of the baseline's runs.  --ngames keeps the run from stopping at the 50th
      finished episode, so every run plays its 200 moves: the 64-move ring is flushed at moves 64, 128 and 192, inside the
      moves timed (after the first 20) (the script refuses a run that played fewer).
  (b) re-analysis under ValueSim at 4096 x 100 and 4096 x 500: a child records 10 moves with the agent play.py builds (a pool of
      100 000 nodes a game; ms per move beside it), then re-analyses two batches of 4096 of the recorded positions with that agent
      and two with an agent whose pool is re-analysis' default (reanalyse.default_max_nodes): ms per batch between HIP events,
      split into upload + load + check, tm_pool_fresh, new roots + search + root statistics, and re-record + copy.
      The played move beside them is THIS child's loop (agent.play, the recorder with an 8-move ring, game.play, update_root,
      a device synchronisation and a host time stamp every move, moves 3 to 9 of games that have just begun), not play.py's:
      it is there for the search share of a batch to stand beside a move of the same process, and it is not (a)'s figure."""
import argparse
import importlib.util
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAY = ["--agent_type", "ValueSim", "--mcts_sims", "100", "--n_games", "4096", "--max_moves", "200", "--ngames", "100000000"]
STAGES = (("load_check", "start", "loaded"), ("pool_fresh", "loaded", "fresh"), ("search", "fresh", "searched"),
          ("rerecord", "searched", "rerecorded"))


def _recording_timing():
    spec = importlib.util.spec_from_file_location("tm_episode_recording_timing", os.path.join(HERE, "scripts", "episode_recording_timing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def part_a(runs, parent, timeout):
    one = _recording_timing().one
    variants = [("save_positions", HERE, ["--save", "--save_positions"]), ("save", HERE, ["--save"])]
    if parent:
        variants.append(("parent_save", os.path.abspath(parent), ["--save"]))
    res = {name: [] for name, _, _ in variants}
    for i in range(runs):
        for name, repo, flags in variants:
            tmp = tempfile.mkdtemp(prefix="positions_")
            try:
                r = one(repo, 20, PLAY + flags + ["--save_dir", tmp + "/"], timeout)
                if r["moves"] != 200:
                    raise RuntimeError("%s played %d moves, not 200: no flush inside the timed moves" % (name, r["moves"]))
                r["bytes_written"] = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
            res[name].append(r)
            print(name, i, json.dumps(r), flush=True)
    base = "parent_save" if parent else "save"
    med = {name: statistics.median(r["ms_per_move"] for r in rs) for name, rs in res.items()}
    return dict(command="play.py " + " ".join(PLAY), skip_moves=20, runs=res, median_ms_per_move=med, baseline=base,
                margin_ms=max(r["ms_per_move"] for r in res[base]) - min(r["ms_per_move"] for r in res[base]),
                save_positions_minus_baseline_ms=med["save_positions"] - med[base], save_minus_baseline_ms=med["save"] - med[base])


def child_b(sims, n_games, moves):
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from tetris_mcts_amd.agents import ValueSim
    from tetris_mcts_amd.episodes import EpisodeRecorder, PositionLoader
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.pyTetris import Tetris
    from tetris_mcts_amd.reanalyse import Reanalyser, default_max_nodes
    env_args = ((20, 10), 1, 0, 0)
    model = Model_VV(backend="hip", seed=0)
    tmp = tempfile.mkdtemp(prefix="reanalyse_timing_")
    out = dict(sims=sims, n_games=n_games)
    try:
        game = Tetris(*env_args, seed=0, n_games=n_games)
        agent = ValueSim(sims=sims, env=Tetris, env_args=env_args, n_games=n_games, online=False, model=model)
        agent.update_root(game)
        rec = EpisodeRecorder(tmp + "/", "data", 0, n_games, ring_moves=8)
        rec.record_positions()
        stamps = []
        for _ in range(moves):
            torch.cuda.synchronize()
            stamps.append(time.perf_counter())
            action = agent.play()
            rec.add(agent, game)
            game.play(action)
            rec.advance(game)
            agent.update_root(game)
            if np.atleast_1d(game.end).any():
                game.reset("ended")
                agent.update_root(game)
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        rec.close()
        d = [1e3 * (b - a) for a, b in zip(stamps[2:], stamps[3:])]
        out["play_ms_per_move"], out["play_max_nodes"] = statistics.median(d), agent.max_nodes
        L = PositionLoader(tmp + "/data0")
        lo = 2 * n_games                                   # (the positions of moves 2 and 3: 4096 different games each)

        def batches(ag, label):
            R = Reanalyser(ag, Tetris(*env_args, seed=1, n_games=n_games))
            R.submit(L.rows[:n_games], L.positions[:n_games])          # warm-up: buffers, the search handle
            R.collect()
            R.timing = {}
            for k in range(2):
                a = lo + k * n_games
                R.submit(L.rows[a:a + n_games], L.positions[a:a + n_games])
                R.collect()
            torch.cuda.synchronize()
            t = R.timing
            per = [{name: t[x][k].elapsed_time(t[y][k]) for name, x, y in STAGES} for k in range(2)]
            out[label] = dict(max_nodes=ag.max_nodes, batches=per,
                              ms_per_batch=statistics.mean(t["start"][k].elapsed_time(t["rerecorded"][k]) for k in range(2)),
                              **{name: statistics.mean(p[name] for p in per) for name, _, _ in STAGES})
        batches(agent, "pool_of_play")
        del agent
        torch.cuda.empty_cache()
        small = ValueSim(sims=sims, env=Tetris, env_args=env_args, n_games=n_games, online=False, model=model,
                         max_nodes=default_max_nodes(sims))
        batches(small, "pool_default")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("TIMING " + json.dumps(out))


def part_b(runs, timeout):
    res = {"4096x100": [], "4096x500": []}
    for i in range(runs):
        for sims in (100, 500):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child_b", str(sims)], capture_output=True, text=True,
                               timeout=timeout)
            if r.returncode != 0:
                raise RuntimeError("run failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
            one = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TIMING ")][-1][7:])
            res["4096x%d" % sims].append(one)
            print(sims, i, json.dumps(one), flush=True)
    med = {}
    for shape, rs in res.items():
        m = dict(play_ms_per_move=statistics.median(r["play_ms_per_move"] for r in rs))
        for label in ("pool_of_play", "pool_default"):
            m[label] = {k: statistics.median(r[label][k] for r in rs) for k in ("ms_per_batch",) + tuple(s[0] for s in STAGES)}
            m[label]["max_nodes"] = rs[0][label]["max_nodes"]
        med[shape] = m
    return dict(runs=res, median=med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child_b", type=int, default=0)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=("a", "b"), default=None)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child_b:
        return child_b(a.child_b, 4096, 10)
    out = {}
    if a.only != "b":
        out["recording"] = part_a(a.runs, a.parent, a.timeout)
    if a.only != "a":
        out["reanalysis"] = part_b(a.runs, a.timeout)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
