"""Where a fit's time goes (one MI355X): train_data on a synthetic replay set of the online run's size, eager and replayed from
the graph, and its parts on their own (a validation pass, a checkpoint save).
    python scripts/fit_timing.py [tuples] [--fit_backend {torch,hip}]
    python scripts/fit_timing.py [tuples] --blocks 3 --json OUT      the two fit backends alternated in blocks of graph-replayed
                                                                     iterations (no validation inside), one JSON file"""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tetris_mcts_amd import model as M, train as T  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("tuples", nargs="?", type=int, default=250000)
ap.add_argument("--fit_backend", default="torch", choices=("torch", "hip"))
ap.add_argument("--blocks", type=int, default=0, help="alternate torch / hip in this many blocks each and stop")
ap.add_argument("--block-iters", type=int, default=1000)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--json", default=None)
args = ap.parse_args()
n = args.tuples
out_json = os.path.abspath(args.json) if args.json else None
rng = np.random.default_rng(0)
states = torch.from_numpy(rng.integers(-1, 2, size=(n, 1, 20, 10)).astype(np.float32)).cuda()
values = (states.sum(dim=(1, 2, 3)) * 0.5 + 20).reshape(-1, 1)
variances = torch.full((n, 1), 4.0, device="cuda")
weights = torch.from_numpy(rng.integers(10, 200, size=(n, 1)).astype(np.float32)).cuda()
os.chdir("/tmp")
if os.environ.get("TM_FIT_BENCHMARK") == "1":      # MIOpen's search for the convolutions' kernels instead of its default pick
    torch.backends.cudnn.benchmark = True
print("cudnn.benchmark (MIOpen find)", torch.backends.cudnn.benchmark, flush=True)
if args.blocks > 0:
    os.environ["TM_TRAIN_GRAPH"] = "1"
    models = {b: M.Model_VV(backend="torch", seed=0) for b in ("torch", "hip")}
    rows = []
    for blk in range(-1, args.blocks):          # block -1 warms both up (MIOpen's kernel choice, allocations) and is not reported
        for b in ("torch", "hip"):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = models[b].train_data([states, values, variances, weights], iters_per_val=10 ** 9, batch_size=args.batch,
                                       max_iters=args.block_iters, log=False, early_stopping=False, fit_backend=b)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if blk >= 0:
                rows.append(dict(block=blk, fit_backend=b, iters=res["iters"], graph_replay=res["graph_replay"],
                                 ms_per_iter=1e3 * dt / res["iters"]))
                print(rows[-1], flush=True)
    ms = {b: [r["ms_per_iter"] for r in rows if r["fit_backend"] == b] for b in ("torch", "hip")}
    summary = dict(tuples=n, batch=args.batch, block_iters=args.block_iters, blocks=rows,
                   torch_ms=dict(min=min(ms["torch"]), max=max(ms["torch"]), median=float(np.median(ms["torch"]))),
                   hip_ms=dict(min=min(ms["hip"]), max=max(ms["hip"]), median=float(np.median(ms["hip"]))),
                   torch_over_hip=float(np.median(ms["torch"]) / np.median(ms["hip"])),
                   note="a block = one train_data call: 3 eager iterations, the capture, the rest replayed from the HIP graph; the "
                        "call's setup (the int8 copy of the states for hip, the data slices) is inside the time")
    print(json.dumps(summary["torch_ms"]), json.dumps(summary["hip_ms"]), "torch / hip = %.3f" % summary["torch_over_hip"], flush=True)
    if out_json:
        os.makedirs(os.path.dirname(out_json), exist_ok=True)
        with open(out_json, "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(0)
for mode in ("0", "1"):
    os.environ["TM_TRAIN_GRAPH"] = mode
    mdl = M.Model_VV(backend="torch", seed=0)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = mdl.train_data([states, values, variances, weights], iters_per_val=100, batch_size=1024, max_iters=1300, log=False,
                         early_stopping=False, fit_backend=args.fit_backend)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print("graph=%s: %d iterations in %.3f s = %.3f ms per iteration (13 validations of %d rows and the saves included) %s" % (mode, res["iters"], dt, 1e3 * dt / res["iters"], n // 10, res), flush=True)
    val = [d[-n // 10:] for d in (states, values, variances, weights / weights.mean())]
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(5): T.validation_loss(mdl.model, val, True)
    torch.cuda.synchronize(); print("   one validation pass: %.1f ms" % (1e3 * (time.perf_counter() - t0) / 5))
    t0 = time.perf_counter()
    for _ in range(5): mdl.save(verbose=False)
    print("   one checkpoint save: %.1f ms" % (1e3 * (time.perf_counter() - t0) / 5))
    # the iterations alone
    os.environ["TM_TRAIN_GRAPH"] = mode
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = mdl.train_data([states, values, variances, weights], iters_per_val=10 ** 9, batch_size=1024, max_iters=1000, log=False, early_stopping=False,
                         fit_backend=args.fit_backend)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print("   1000 iterations without validation: %.3f ms per iteration" % (1e3 * dt / 1000), flush=True)
