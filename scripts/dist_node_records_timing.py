#!/usr/bin/env python
"""What recording the harvested nodes of the distributional head costs and how many there are
(profiles/dist_node_records_timing.json); scripts/node_records_timing.py for DistValueSim.

    python scripts/dist_node_records_timing.py [--parent DIR] [--runs 3] [--out FILE] [-- play.py arguments]

Three things, on an MI355X:
  * ms per move of play.py with --save_dist_nodes, without it, and (with --parent) of the tree in DIR - a built checkout of the
    parent commit: every run is a fresh child process that calls play.main() with the arguments after `--` (default: DistValueSim's
    benchmark batch, --agent_type DistValueSim --mcts_sims 1000 --n_games 4096, over --max_moves 200: long enough for the pools of
    100 000 nodes to fill and collect) and stamps every game.play(); medians of `--runs` alternating runs;
  * rows harvested per move, the largest flush (the largest part file) and the rows lost, of the --save_dist_nodes runs;
  * tm_nodes_drain_dist per call against TreeStore.replay_dist() (the gather DistValueSim.harvested() uses) on the same buffers: a
    store of `--bench_store_games` games with `--bench_games` of them holding `--bench_tuples` harvested tuples each, device time
    of the drain by events, host time of replay_dist() and the clear around a synchronise.
Every step that opens the GPU is a child process under a time limit of its own; the first one that fails, or runs out of time,
ends the script: nothing else is started after it."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["--agent_type", "DistValueSim", "--mcts_sims", "1000", "--n_games", "4096", "--max_moves", "200", "--ngames", "100000000"]
ROW = 320


def child(repo, skip, argv):
    sys.path.insert(0, repo)
    os.chdir(repo)
    import play
    from tetris_mcts_amd.pyTetris import Tetris
    stamps, inner = [], Tetris.play

    def stamped(self, action):
        stamps.append(time.perf_counter())
        return inner(self, action)
    Tetris.play = stamped
    play.main(argv)
    d = [b - a for a, b in zip(stamps[skip:], stamps[skip + 1:])]
    print("TIMING " + json.dumps(dict(moves=len(stamps), timed=len(d), ms_per_move=1e3 * sum(d) / len(d),
                                      ms_median_move=1e3 * statistics.median(d), ms_max_move=1e3 * max(d))))


def _run(args, timeout):
    """one child under its time limit; anything but a clean exit ends the script (subprocess.run kills the child at the limit)"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("run failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return r


def one(repo, skip, argv, timeout):
    r = _run(["--child", repo, "--skip", str(skip), "--"] + argv, timeout)
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("TIMING ")][-1][7:])
    m = re.search(r"node rows written: (\d+) in (\d+) file\(s\), (\d+) lost", r.stdout)
    if m:
        res["node_rows"], res["node_files"], res["rows_lost"] = int(m.group(1)), int(m.group(2)), int(m.group(3))
        res["rows_per_move"] = res["node_rows"] / max(res["moves"], 1)
    res["warnings"] = [l for l in r.stderr.splitlines() if l.startswith("WARNING")][:4]
    return res


def drain_bench(games, tuples, G, cap, reps=20):
    """tm_nodes_drain_dist (device time, events) against TreeStore.replay_dist() + the clear (host time around a synchronise)"""
    import ctypes as C
    import torch
    sys.path.insert(0, HERE)
    from tetris_mcts_amd.store import KIND_DIST, TreeStore
    store = TreeStore(G, max_nodes=64, max_trace=64, kind=KIND_DIST, online=True, min_visits_to_store=3, replay_cap=cap)
    store.t["replay_obs"].random_(0, 1 << 30)
    store.t["replay_stat"].uniform_(1, 100)
    store.t["replay_dist"].uniform_(0, 1)
    count = torch.zeros(G, dtype=torch.int32, device="cuda")
    count[torch.randperm(G, device="cuda")[:games]] = tuples
    rows = games * tuples
    ring = torch.zeros((rows + 1) * ROW, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(4, dtype=torch.int32, device="cuda")
    offsets = torch.zeros(G + 1, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    drain_ms, replay_ms = [], []
    for i in range(reps + 3):
        store.t["replay_count"].copy_(count)
        counters.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = store.L.tm_nodes_drain_dist(C.byref(store.s), p(ring), rows + 1, p(counters), p(offsets),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0 and counters.tolist()[:2] == [rows, 0]
        store.t["replay_count"].copy_(count)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keys, dists, visits = store.replay_dist()
        store.t["replay_count"].zero_()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        assert keys.shape[0] == rows
        if i >= 3:
            drain_ms.append(e0.elapsed_time(e1))
            replay_ms.append(1e3 * (t1 - t0))
    print("DRAIN " + json.dumps(dict(games=G, replay_cap=cap, games_with_tuples=games, tuples_each=tuples, rows=rows,
                                     bytes_moved=2 * rows * ROW, reps=reps, drain_ms_median=statistics.median(drain_ms),
                                     drain_ms_min=min(drain_ms), replay_dist_ms_median=statistics.median(replay_ms),
                                     replay_dist_ms_min=min(replay_ms))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--drain_child", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--min_visit", type=int, default=50, help="DistValueSim's default min_visits_to_store")
    ap.add_argument("--bench_store_games", type=int, default=1024)
    ap.add_argument("--bench_cap", type=int, default=4096)
    ap.add_argument("--bench_games", type=int, default=64)
    ap.add_argument("--bench_tuples", type=int, default=2048)
    ap.add_argument("--out", default=None)
    ap.add_argument("rest", nargs="*")
    a = ap.parse_args()
    argv = a.rest or DEFAULT
    if a.child:
        return child(a.child, a.skip, argv)
    if a.drain_child:
        return drain_bench(a.bench_games, a.bench_tuples, a.bench_store_games, a.bench_cap)
    variants = [("save_dist_nodes", HERE, True), ("plain", HERE, False)] + ([("parent", os.path.abspath(a.parent), False)] if a.parent else [])
    runs = {name: [] for name, _, _ in variants}
    for i in range(a.runs):
        for name, repo, save in variants:
            tmp = tempfile.mkdtemp(prefix="distnodes_") if save else None
            try:
                extra = ["--save_dist_nodes", "--min_visit", str(a.min_visit), "--save_dir", tmp + "/"] if save else []
                res = one(repo, a.skip, argv + extra, a.timeout)
                if save:
                    sizes = [os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp) if ".part" in f]
                    res["bytes_written"], res["largest_flush_rows"] = sum(sizes), max(sizes, default=0) // ROW
            finally:
                if tmp:
                    shutil.rmtree(tmp, ignore_errors=True)
            runs[name].append(res)
            print(name, i, json.dumps(res), flush=True)
    base = "parent" if a.parent else "plain"
    med = {name: statistics.median(r["ms_per_move"] for r in rs) for name, rs in runs.items()}
    spread = max(r["ms_per_move"] for r in runs[base]) - min(r["ms_per_move"] for r in runs[base])
    r = _run(["--drain_child", "--bench_store_games", str(a.bench_store_games), "--bench_cap", str(a.bench_cap),
              "--bench_games", str(a.bench_games), "--bench_tuples", str(a.bench_tuples)], a.timeout)
    bench = json.loads([l for l in r.stdout.splitlines() if l.startswith("DRAIN ")][-1][6:])
    print("drain", json.dumps(bench), flush=True)
    saved = runs["save_dist_nodes"]
    out = dict(command="play.py " + " ".join(argv), min_visit=a.min_visit, skip_moves=a.skip, runs=runs, median_ms_per_move=med,
               baseline=base, baseline_spread_ms=spread, save_dist_nodes_minus_baseline_ms=med["save_dist_nodes"] - med[base],
               plain_minus_baseline_ms=med["plain"] - med[base],
               rows_per_move_median=statistics.median(r.get("rows_per_move", 0.0) for r in saved),
               largest_flush_rows=max(r.get("largest_flush_rows", 0) for r in saved),
               rows_lost=sum(r.get("rows_lost", 0) for r in saved), drain_against_replay_dist=bench)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
