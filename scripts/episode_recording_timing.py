#!/usr/bin/env python
"""ms per move of play.py with and without --save (profiles/episode_recording_timing.json).

    python scripts/episode_recording_timing.py [--parent DIR] [--runs 3] [--out FILE] [-- play.py arguments]

Every run is a fresh child process that calls play.main() with the arguments after `--` (default: the issue's command,
--agent_type ValueSim --mcts_sims 100 --n_games 4096 --max_moves 200) and takes a host time stamp at every game.play(): the agent
reads its actions back every move, so the stamps are a move apart in device time as well.  ms per move = the mean interval after
the first `--skip` moves.  Three variants, alternating: `save` (this tree with --save, into a temporary directory), `plain` (this
tree without it) and, with --parent, `parent` (the tree in DIR - a built checkout of the parent commit - without it).  Reported:
the median of each, and the parent's (without --parent: plain's) spread max - min as the margin."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["--agent_type", "ValueSim", "--mcts_sims", "100", "--n_games", "4096", "--max_moves", "200"]


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


def one(repo, skip, argv, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", repo, "--skip", str(skip), "--"] + argv,
                       capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("run failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("TIMING ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    ap.add_argument("rest", nargs="*")
    a = ap.parse_args()
    argv = a.rest or DEFAULT
    if a.child:
        return child(a.child, a.skip, argv)
    variants = [("save", HERE, True), ("plain", HERE, False)] + ([("parent", os.path.abspath(a.parent), False)] if a.parent else [])
    runs = {name: [] for name, _, _ in variants}
    for i in range(a.runs):
        for name, repo, save in variants:
            tmp = tempfile.mkdtemp(prefix="episodes_") if save else None
            try:
                extra = ["--save", "--save_dir", tmp + "/"] if save else []
                res = one(repo, a.skip, argv + extra, a.timeout)
                if save:
                    res["bytes_written"] = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))
            finally:
                if tmp:
                    shutil.rmtree(tmp, ignore_errors=True)
            runs[name].append(res)
            print(name, i, json.dumps(res), flush=True)
    base = "parent" if a.parent else "plain"
    med = {name: statistics.median(r["ms_per_move"] for r in rs) for name, rs in runs.items()}
    spread = max(r["ms_per_move"] for r in runs[base]) - min(r["ms_per_move"] for r in runs[base])
    out = dict(command="play.py " + " ".join(argv), skip_moves=a.skip, runs=runs, median_ms_per_move=med, baseline=base,
               margin_ms=spread, save_minus_baseline_ms=med["save"] - med[base], plain_minus_baseline_ms=med["plain"] - med[base])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
