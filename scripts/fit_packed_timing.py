"""What feeding a HIP fit packed observations costs and saves (one MI355X): train_data(state_format="dense") against
state_format="packed" on the same rows and from the same weights, in one process, alternated, `--repeats` times each.
    python scripts/fit_packed_timing.py [--head] [--json OUT]      (the value net, or with --head the distributional head)
Per head it records
  ms_per_iter   a graph-replayed iteration at --batch over --tuples training rows: one train_data call of --iters iterations minus
                the same call cut short after its set-up (max_iters=4), over the iterations between them (validation_fraction 0)
  setup_ms      from "the gathered tuples are on the device" to "the first iteration is launched", at each of --setup-rows:
                dense = dist.render_observations (the agent's _dense_set) + the per-fit state (HipFit / HipDistFit: the checks, the
                int8 copy); packed = the per-fit state alone
  peak_bytes    torch.cuda.max_memory_allocated() across one train_data call (rendering included for dense, as in the agent) at
                each of --setup-rows, after reset_peak_memory_stats, less what was allocated before the call
The rows are random boards with a falling piece of four cells; the dense route's code is the one the option leaves untouched."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tetris_mcts_amd import dist as tdist, model as M, train as T  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("--head", action="store_true", help="the distributional head (Model_Dist, 50 atoms) instead of the value net")
ap.add_argument("--tuples", type=int, default=250000)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--setup-rows", default="250000,500000")
ap.add_argument("--json", default=None)
args = ap.parse_args()
out_json = os.path.abspath(args.json) if args.json else None
os.environ["TM_TRAIN_GRAPH"] = "1"
os.chdir("/tmp")
rng = np.random.default_rng(0)
FORMATS = ("dense", "packed")


def observations(n):
    """n packed observations on the device: rows locked at random below a random height, a horizontal piece of four cells above"""
    h = rng.integers(0, 14, n)
    rows = rng.integers(0, 1024, size=(n, 20)).astype(np.uint32) * (np.arange(20)[None, :] >= (20 - h)[:, None])
    k = np.zeros((n, 12), np.uint32)
    k[:, :10] = rows[:, 0::2] | (rows[:, 1::2] << np.uint32(16))
    c = (rng.integers(0, np.maximum(1, 18 - h)) * 10 + rng.integers(0, 7, n)).astype(np.uint32)
    k[:, 10] = c | ((c + 1) << np.uint32(8)) | ((c + 2) << np.uint32(16)) | ((c + 3) << np.uint32(24))
    return torch.from_numpy(k.view(np.int32)).cuda()


def targets(n):
    w = torch.from_numpy(rng.integers(10, 200, size=(n, 1)).astype(np.float32)).cuda()
    if args.head:
        centre = torch.from_numpy(rng.uniform(2, 47, (n, 1)).astype(np.float32)).cuda()
        t = torch.softmax(-0.5 * (torch.arange(50, device="cuda").reshape(1, -1) - centre) ** 2 / 4.0, 1)
        return [t, w]
    v = torch.from_numpy(rng.uniform(5, 60, (n, 1)).astype(np.float32)).cuda()
    return [v, torch.full((n, 1), 4.0, device="cuda"), w]


def dense_states(keys):
    """what the agents' _dense_set makes of the gathered keys"""
    s = tdist.render_observations(keys)
    if not args.head:
        return s
    x = torch.zeros(keys.shape[0], 1, 22, 10, dtype=torch.float32, device=keys.device)
    x[:, :, 2:, :] = s
    return x


def new_model():
    if args.head:
        from tetris_mcts_amd.model_distributional import Model_Dist
        return Model_Dist(atoms=50, seed=0, backend="torch")
    return M.Model_VV(backend="torch", seed=0)


fit_backend = "hip_dist" if args.head else "hip"


def fit(mdl, states, rest, fmt, iters, val=0.0):
    return mdl.train_data([states] + rest, state_format=fmt, fit_backend=fit_backend, validation_backend="hip", validation_fraction=val,
                          iters_per_val=10 ** 9, batch_size=args.batch, max_iters=iters, log=False, early_stopping=False)


def stats(xs):
    return dict(min=min(xs), max=max(xs), median=float(np.median(xs)), all=list(xs))


summary = dict(head="model_distributional.Net" if args.head else "model.Net", tuples=args.tuples, batch=args.batch, iters=args.iters,
               repeats=args.repeats)
# ---- a replayed iteration ----
keys, rest = observations(args.tuples), targets(args.tuples)
dense = dense_states(keys)
models = {f: new_model() for f in FORMATS}
ms = {f: [] for f in FORMATS}
for rep in range(-1, args.repeats):          # repeat -1 warms both up and is not reported
    for f in FORMATS:
        st = dense if f == "dense" else keys
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = fit(models[f], st, rest, f, args.iters)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        t1 = time.perf_counter()
        short = fit(models[f], st, rest, f, 4)
        torch.cuda.synchronize(); ds = time.perf_counter() - t1
        assert res["graph_replay"] and short["graph_replay"]
        if rep >= 0:
            ms[f].append(1e3 * (dt - ds) / (res["iters"] - short["iters"]))
            print(dict(repeat=rep, state_format=f, ms_per_iter=ms[f][-1], short_call_ms=1e3 * ds), flush=True)
summary["ms_per_iter"] = {f: stats(ms[f]) for f in FORMATS}
summary["packed_over_dense_ms_per_iter"] = summary["ms_per_iter"]["packed"]["median"] / summary["ms_per_iter"]["dense"]["median"]
del dense, models
# ---- set-up time and peak memory ----
Fit = T.HipDistFit if args.head else T.HipFit
summary["setup_ms"], summary["peak_bytes"] = {}, {}
for n in [int(x) for x in args.setup_rows.split(",")]:
    keys, rest = observations(n), targets(n)
    rest[-1] = rest[-1] / rest[-1].mean()
    setup, peak = {f: [] for f in FORMATS}, {f: [] for f in FORMATS}
    for rep in range(-1, args.repeats):
        for f in FORMATS:
            mdl = new_model()
            opt = mdl._fused_optimizer() if args.head else mdl._optimizer()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            st = dense_states(keys) if f == "dense" else keys
            hip = Fit(mdl.model, opt, [st] + rest, args.batch, state_format=f)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            del hip, st, opt, mdl
            torch.cuda.empty_cache()
            mdl = new_model()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            st = dense_states(keys) if f == "dense" else keys
            fit(mdl, st, rest, f, 8, val=0.1)
            torch.cuda.synchronize()
            pk = torch.cuda.max_memory_allocated() - base
            del st, mdl
            torch.cuda.empty_cache()
            if rep >= 0:
                setup[f].append(1e3 * dt)
                peak[f].append(int(pk))
                print(dict(rows=n, repeat=rep, state_format=f, setup_ms=1e3 * dt, peak_bytes=int(pk)), flush=True)
    summary["setup_ms"][str(n)] = {f: stats(setup[f]) for f in FORMATS}
    summary["peak_bytes"][str(n)] = {f: stats(peak[f]) for f in FORMATS}
    del keys, rest
    torch.cuda.empty_cache()
print(json.dumps(summary), flush=True)
if out_json:
    os.makedirs(os.path.dirname(out_json), exist_ok=True)
    with open(out_json, "w") as fh:
        json.dump(summary, fh, indent=1)
