#!/usr/bin/env python
"""The split-precision value-net backend ("hip_bf16x3") against the fp32 one ("hip"), on one GPU.  Two modes, one JSON line each:

  kernels  per-launch time of the value net (dense states, k_vn_conv[_x3] + k_vn_fc1) at the headline's and ValueSimLP's mean
           requests per launch (1 867 and 7 169 states), both backends, with TFLOP/s against each backend's own peak (fp32
           matrix 157.3 TF; bf16x3 = the bf16 matrix peak / 6 products); and max |dv|, |dvar| of bf16x3 against fp32 over the
           states a short real search asked for (render_eval), with the r06 checkpoint; --fc1 bf16x3 adds the third
           configuration, "hip_bf16x3" with the split fc1 (k_vn_fc1_x3), and --repeats N times every configuration N times in
           turn and reports the median and the range of the N;
  head     the distributional head (DistValueSim's leaf evaluator, Model_Dist(seed 0) as bench.py runs it): per-launch time on
           4096 dense states (k_dn_conv[_x3] + k_dn_fc), both backends alternated in blocks of 20 launches after 20 warm-up
           launches each, with TFLOP/s against each backend's own peak; and max |dp| of bf16x3 against fp32 over the leaves a
           short real DistValueSim search asked for (render_eval);
  search   ms per move of the native search loop, moves warmup+1 .. warmup+steps, for ONE agent and ONE backend (two stores of
           4096 x 100 000 nodes do not fit one GPU: one process per backend).

    python scripts/bench_split_precision.py kernels [--out profiles/FILE.json]
    python scripts/bench_split_precision.py head [--out ...]
    python scripts/bench_split_precision.py kernels --fc1 bf16x3 --repeats 3 [--out ...]
    python scripts/bench_split_precision.py search --agent ValueSim --backend hip_bf16x3 [--fc1 bf16x3] [--out ...]
    python scripts/bench_split_precision.py search --agent DistValueSim --sims 1000 --warmup 5 --steps 5 --backend hip_bf16x3
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CKPT = os.path.join(ROOT, "tetris_mcts_amd", "checkpoints", "value_net_online_r06.pt")
# useful FLOP per state: conv1 144x32x9, conv2 96x32x288, conv3 56x32x288, fc1 1792x256, out 256x2 multiply-adds
FLOP_STATE = 2 * (144 * 32 * 9 + 96 * 32 * 288 + 56 * 32 * 288 + 1792 * 256 + 256 * 2)
PEAK_TF = {"hip": 157.3, "hip_bf16x3": 2516.6 / 6}      # MI355X: fp32 matrix = fp32 vector rate; bf16 matrix dense
# the distributional head: conv1 133x32x16, conv2 64x32x512, fc1 2048x128, fc_v 128x50 multiply-adds per state
FLOP_STATE_DIST = 2 * (133 * 32 * 16 + 64 * 32 * 512 + 2048 * 128 + 128 * 50)


FC1X3 = "hip_bf16x3+fc1_bf16x3"      # the third configuration's name in the output


def _model(backend, fc1="fp32"):
    from tetris_mcts_amd.model import Model_VV
    m = Model_VV(backend=backend, fc1=fc1)
    m.load(CKPT, verbose=False)
    return m


def _searched_states(n_games=512, sims=16, moves=6):
    """int8 [n, 200]: every leaf state a ValueSimLP search with the fp32 net asked for (render_eval of every launch)"""
    import torch
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.pyTetris import Tetris
    m = _model("hip")
    seen = []

    def ev(states):
        seen.append(states.clone())
        return m.inference_device(states)
    env_args = ((20, 10), 1, 0, 0)
    game = Tetris(*env_args, seed=20261016, n_games=n_games)
    agent = agents.ValueSimLP(sims=sims, env=Tetris, env_args=env_args, n_games=n_games, max_nodes=20000, evaluator=ev,
                              online=False)
    agent.update_root(game)
    for _ in range(moves):
        act = agent.play()
        game.play(act)
        agent.update_root(game)
    s = torch.cat(seen)
    return s[(s != 0).any(dim=1)].contiguous()


def kernels(args):
    import torch
    states = _searched_states()
    models = {b: _model(b) for b in ("hip", "hip_bf16x3")}
    if args.fc1 == "bf16x3":
        models[FC1X3] = _model("hip_bf16x3", "bf16x3")
    out = dict(mode="kernels", searched_states=int(states.shape[0]), flop_per_state=FLOP_STATE, launches={}, repeats=args.repeats)
    v32, r32 = [t.clone() for t in models["hip"].inference_device(states)]
    vx, rx = [t.clone() for t in models["hip_bf16x3"].inference_device(states)]
    out["max_abs_dv"] = float((vx - v32).abs().max().item())
    out["max_abs_dvar"] = float((rx - r32).abs().max().item())
    out["max_abs_v"], out["max_abs_var"] = float(v32.abs().max().item()), float(r32.abs().max().item())
    if FC1X3 in models:
        vf, rf = models[FC1X3].inference_device(states)
        out["max_abs_dv_fc1_x3"], out["max_abs_dvar_fc1_x3"] = float((vf - v32).abs().max().item()), float((rf - r32).abs().max().item())
    for n in (1867, 7169):
        batch = states[torch.arange(n, device=states.device) % states.shape[0]].contiguous()
        times = {b: [] for b in models}
        for _ in range(args.repeats):       # the configurations in turn, so that a drift of the clocks meets them all
            for b, m in models.items():
                v, r = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
                for _ in range(20):
                    m.inference_device(batch, v, r)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    m.inference_device(batch, v, r)
                e1.record()
                torch.cuda.synchronize()
                times[b].append(1e3 * e0.elapsed_time(e1) / args.launches)
        row = {}
        for b in models:
            us = sorted(times[b])[len(times[b]) // 2]       # the median
            peak = PEAK_TF["hip" if b == "hip" else "hip_bf16x3"]
            tf = FLOP_STATE * n / (us * 1e-6) / 1e12
            row[b] = dict(us_per_launch=round(us, 2), us_range=[round(min(times[b]), 2), round(max(times[b]), 2)],
                          tflops=round(tf, 2), peak_tflops=round(peak, 1), of_peak=round(tf / peak, 4))
        row["speedup"] = round(row["hip"]["us_per_launch"] / row["hip_bf16x3"]["us_per_launch"], 3)
        if FC1X3 in models:
            row["speedup_fc1_x3_over_hip_bf16x3"] = round(row["hip_bf16x3"]["us_per_launch"] / row[FC1X3]["us_per_launch"], 3)
        out["launches"][str(n)] = row
    return out


def _dist_model(backend):
    from tetris_mcts_amd.model_distributional import Model_Dist
    return Model_Dist(atoms=50, seed=0, backend=backend)       # bench.py's DistValueSim head


def _dist_searched_states(n_games=512, sims=32, moves=6):
    """int8 [n, 200]: every leaf state a DistValueSim search with the fp32 head asked for (render_eval of every launch)"""
    import torch
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.pyTetris import Tetris
    m = _dist_model("hip")
    seen = []

    def ev(states):
        st = torch.from_numpy(states.reshape(-1, 200)).cuda()
        seen.append(st)
        return m.inference_device(st)[:, :50].cpu().numpy()
    env_args = ((20, 10), 1, 0, 0)
    game = Tetris(*env_args, seed=20261016, n_games=n_games)
    agent = agents.DistValueSim(sims=sims, env=Tetris, env_args=env_args, n_games=n_games, max_nodes=20000, evaluator=ev)
    agent.update_root(game)
    for _ in range(moves):
        act = agent.play()
        game.play(act)
        agent.update_root(game)
    s = torch.cat(seen)
    return s[(s != 0).any(dim=1)].contiguous()


def head(args):
    import torch
    states = _dist_searched_states()
    models = {b: _dist_model(b) for b in ("hip", "hip_bf16x3")}
    p32 = models["hip"].inference_device(states)[:, :50].clone()
    px3 = models["hip_bf16x3"].inference_device(states)[:, :50].clone()
    out = dict(mode="head", searched_states=int(states.shape[0]), flop_per_state=FLOP_STATE_DIST,
               max_abs_dp=float((px3 - p32).abs().max().item()), max_rel_dp=float(((px3 - p32).abs() / p32).max().item()))
    n = args.states
    batch = states[torch.arange(n, device=states.device) % states.shape[0]].contiguous()
    dist = {b: torch.empty(n, 64, device="cuda") for b in models}
    for b, m in models.items():
        for _ in range(20):
            m.inference_device(batch, dist[b])
    torch.cuda.synchronize()
    ms = {b: 0.0 for b in models}
    block = 20
    for _ in range(args.launches // block):
        for b, m in models.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                m.inference_device(batch, dist[b])
            e1.record()
            torch.cuda.synchronize()
            ms[b] += e0.elapsed_time(e1)
    row = {}
    for b in models:
        us = 1e3 * ms[b] / (block * (args.launches // block))
        tf = FLOP_STATE_DIST * n / (us * 1e-6) / 1e12
        row[b] = dict(us_per_launch=round(us, 2), tflops=round(tf, 2), peak_tflops=round(PEAK_TF[b], 1),
                      of_peak=round(tf / PEAK_TF[b], 4))
    row["speedup"] = round(row["hip"]["us_per_launch"] / row["hip_bf16x3"]["us_per_launch"], 3)
    out["launches"] = {str(n): row}
    return out


def search(args):
    import numpy as np
    import torch
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.pyTetris import Tetris
    if args.fc1 != "fp32" and (args.agent == "DistValueSim" or args.backend != "hip_bf16x3"):
        sys.exit("--fc1 bf16x3 belongs to the value net's hip_bf16x3 backend")
    model = _dist_model(args.backend) if args.agent == "DistValueSim" else _model(args.backend, args.fc1)
    env_args = ((20, 10), 1, 0, 0)
    G = args.games
    game = Tetris(*env_args, seed=20260925, n_games=G)
    agent = getattr(agents, args.agent)(sims=args.sims, env=Tetris, env_args=env_args, n_games=G, max_nodes=args.max_nodes,
                                        model=model, online=False, ev_every=16)
    assert agent.search_model() is model
    agent.update_root(game)
    torch.cuda.synchronize()

    def move():
        act = agent.play()
        game.play(act)
        agent.update_root(game)
        ended = np.atleast_1d(game.end)
        if ended.any():
            game.reset("ended")
            agent.update_root(game)
    for _ in range(args.warmup):
        move()
    torch.cuda.synchronize()
    agent.store.search_stats(agent.n_sub, agent.ev_every, reset=True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        move()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / args.steps
    st = agent.store.search_stats(agent.n_sub, agent.ev_every, reset=True) or {}
    return dict(mode="search", agent=args.agent, backend=args.backend, fc1=args.fc1, games=G, sims=args.sims, max_nodes=args.max_nodes,
                moves="%d-%d" % (args.warmup + 1, args.warmup + args.steps), ms_per_move=round(ms, 2), search_stats=st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "head", "search"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--states", type=int, default=4096, help="head: states per launch")
    ap.add_argument("--agent", default="ValueSim", choices=("ValueSim", "ValueSimLP", "DistValueSim"))
    ap.add_argument("--backend", default="hip", choices=("hip", "hip_bf16x3"))
    ap.add_argument("--fc1", default="fp32", choices=("fp32", "bf16x3"), help="kernels: also time hip_bf16x3 with the split fc1; "
                    "search: fc1 of the hip_bf16x3 model")
    ap.add_argument("--repeats", type=int, default=1, help="kernels: timed blocks per configuration (median and range reported)")
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=500)
    ap.add_argument("--max-nodes", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    res = {"kernels": kernels, "head": head, "search": search}[args.mode](args)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
