#!/usr/bin/env python
"""Learning evidence for the offline targets' discount and net bootstrap: one recorded set, three fits from
the same checkpoint with the same iteration budget, each result played for the same number of moves.

    python scripts/offline_discount_evidence.py [--out profiles/offline_discount_evidence.jsonl] [--checkpoint F]
           [--record-moves 300] [--iters 3000] [--play-minutes 1.0]

1. `play.py --agent_type ValueSimLP --n_games 512 --mcts_sims 200 --save` under the checkpoint for --record-moves moves.
2. `train.py --td --td_lambda 0.9` on that set three ways: the defaults; `--target_gamma 0.999`; that plus `--bootstrap net
   --bootstrap_rounds 4`.  The largest target a fit saw is the `out_ubound[0]` of the checkpoint it wrote (Model_VV.train_data).
3. `scripts/selfplay_online.py --no-train --load` under the starting checkpoint and under each result for --play-minutes; the
   rounds of 250 moves that ALL of them completed are compared: lines cleared per 1000 moves by all games.
Every step is a fresh process with a time limit, one after the other; the first that fails ends the run.  One JSON line per
checkpoint played.  Needs a GPU."""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FITS = (("defaults", []), ("gamma_0.999", ["--target_gamma", "0.999"]),
        ("gamma_0.999_bootstrap_net_4", ["--target_gamma", "0.999", "--bootstrap", "net", "--bootstrap_rounds", "4"]))


def run(cmd, cwd, limit, log):
    with open(log, "w") as f:
        r = subprocess.run(cmd, cwd=cwd, stdout=f, stderr=subprocess.STDOUT, timeout=limit)
    if r.returncode != 0:
        sys.exit("%s failed with status %d: see %s" % (" ".join(cmd[:3]), r.returncode, log))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="offline_discount_evidence.jsonl")
    ap.add_argument("--checkpoint", default=os.path.join(ROOT, "tetris_mcts_amd", "checkpoints", "value_net_online_r06.pt"))
    ap.add_argument("--record-moves", type=int, default=300)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--play-minutes", type=float, default=1.0)
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--sims", type=int, default=200)
    a = ap.parse_args()
    import torch
    out = os.path.abspath(a.out)
    logs = os.path.splitext(out)[0] + "_logs"
    os.makedirs(logs, exist_ok=True)
    work = tempfile.mkdtemp(prefix="tm_evidence_")

    def seat(name):
        d = os.path.join(work, name)
        os.makedirs(os.path.join(d, "pytorch_model"))
        shutil.copy(a.checkpoint, os.path.join(d, "pytorch_model", "model_checkpoint"))
        return d
    rec = seat("rec")
    run([sys.executable, os.path.join(ROOT, "play.py"), "--agent_type", "ValueSimLP", "--n_games", str(a.games), "--mcts_sims",
         str(a.sims), "--save", "--save_dir", os.path.join(rec, "data") + "/", "--max_moves", str(a.record_moves), "--ngames",
         "100000000"], rec, 600, os.path.join(logs, "record.log"))
    assert "Loading model..." in open(os.path.join(logs, "record.log")).read() and glob.glob(os.path.join(rec, "data", "data*"))
    played = [dict(name="start", checkpoint=a.checkpoint, flags=None)]
    for name, flags in FITS:
        d = seat(name)
        cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--data_paths", os.path.join(rec, "data", "data*"), "--td", "--td_lambda",
               "0.9", "--batch_size", "1024", "--epochs", "1000", "--max_iters", str(a.iters)] + flags
        run(cmd, d, 900, os.path.join(logs, "fit_%s.log" % name))
        ck = os.path.join(d, "pytorch_model", "model_checkpoint")
        bound = torch.load(ck, map_location="cpu")["model_state_dict"]["out_ubound"]
        played.append(dict(name=name, checkpoint=ck, flags=" ".join(cmd[3:]).replace(rec, "REC"), largest_target=float(bound[0]),
                           fit_log_tail=open(os.path.join(logs, "fit_%s.log" % name)).read().strip().splitlines()[-2:]))
    for p in played:
        p["rounds_file"] = os.path.join(logs, "play_%s.jsonl" % p["name"])
        run([sys.executable, os.path.join(ROOT, "scripts", "selfplay_online.py"), "--load", p["checkpoint"], "--no-train", "--minutes",
             str(a.play_minutes), "--max-nodes", "100000", "--games", str(a.games), "--sims", str(a.sims), "--train-every", "250",
             "--out", p["rounds_file"]], ROOT, int(a.play_minutes * 60) + 300, os.path.join(logs, "play_%s.log" % p["name"]))
        p["rounds"] = [json.loads(line) for line in open(p["rounds_file"])]
    common = min(len(p["rounds"]) for p in played)
    with open(out, "w") as f:
        for p in played:
            r = p.pop("rounds")[:common]
            line = dict(name=p["name"], flags=p["flags"], largest_target=p.get("largest_target"), recorded_moves=a.record_moves,
                        games=a.games, sims=a.sims, fit_iters=a.iters, moves_per_game_compared=250 * common,
                        lines_per_1000_moves=sum(x["lines_per_1000_moves"] for x in r) / max(common, 1),
                        lines_per_1000_moves_by_round=[round(x["lines_per_1000_moves"], 2) for x in r],
                        episodes_ended=sum(x["episodes"] for x in r), fit_log_tail=p.get("fit_log_tail"))
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
