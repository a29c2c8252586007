"""What elastic weight consolidation costs for the distributional head (one MI355X): the Fisher pass and the penalty inside a
replayed iteration.  scripts/fisher_timing.py is the value net's.
    python scripts/dist_fisher_timing.py [--rows 65536] [--slab 1024] [--atoms 50] [--reps 5] [--block-iters 1000]
                                         [--json profiles/dist_fisher_timing.json] [--baseline-json FILE ...]
    python scripts/dist_fisher_timing.py --plain-only --package-root <a checkout of the parent commit, built> --json FILE
    python scripts/dist_fisher_timing.py --merge FILE --baseline-json FILE ... --json FILE      (no GPU: one summary of several runs)

The pass: tm_distnet_fit_fisher over `rows` fresh rows (from a seed) at `slab`, against rows / 1024 calls of tm_distnet_fit_grad
at batch 1 024 over the same rows in the same process - by count the same matrix work plus the squaring, so the ratio is what is
reported.  Device events, every shape warmed up, the legs alternated `reps` times, minimum / median / maximum reported.

The penalty: train_data(fit_backend="hip_dist") at batch 1 024 replayed from the graph, with and without `ewc_dist`, alternated
in blocks of --block-iters iterations; a block's time is the call's minus the same call cut short after its setup
(fit_timing.py's rule).  --plain-only times the blocks without `ewc_dist` alone and needs nothing this change adds: with
--package-root it is the baseline of the parent commit (a process of its own: run it before and after this commit's legs, in the
same session); --baseline-json puts such results into this run's summary with the ratio of the two plain legs."""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--slab", type=int, default=1024)
ap.add_argument("--atoms", type=int, default=50)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--block-iters", type=int, default=1000)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--package-root", default=ROOT)
ap.add_argument("--baseline-json", nargs="*", default=[])
ap.add_argument("--merge", default=None)
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "dist_fisher_timing.json"))
args = ap.parse_args()
out_json = os.path.abspath(args.json)
baseline = [json.load(open(f)) for f in args.baseline_json]


def spread(v):
    return dict(min=min(v), median=float(np.median(v)), max=max(v), reps=len(v))


def with_baseline(it):
    """the parent commit's plain blocks (--baseline-json, in the order given) beside this commit's"""
    if baseline:
        pb = [dict(b, run=k) for k, base in enumerate(baseline) for b in base["iteration"]["blocks"]]
        pm = [b["ms_per_iter"] for b in pb]
        it.update(parent_plain_ms=spread(pm), parent_blocks=pb, plain_over_parent_plain=float(it["plain_ms"]["median"] / np.median(pm)),
                  parent_note="the parent commit's blocks ran in processes of their own (run 0, 1, ...: in the order given), around this one")
    return it


if args.merge:
    summary = json.load(open(args.merge))
    with_baseline(summary["iteration"])
    with open(out_json, "w") as f:
        json.dump(summary, f, indent=1)
    sys.exit(0)
sys.path.insert(0, os.path.abspath(args.package_root))
from tetris_mcts_amd import _lib, model_distributional as MD  # noqa: E402
os.chdir("/tmp")      # nothing a fit writes lands in the repository
os.environ["TM_TRAIN_GRAPH"] = "1"
n, atoms, dev = args.rows, args.atoms, torch.device("cuda")
assert n % 1024 == 0
rng = np.random.default_rng(args.seed)
states = torch.zeros(n, 1, 22, 10, device=dev)
states[:, :, 2:, :] = torch.from_numpy(rng.integers(-1, 2, size=(n, 1, 20, 10)).astype(np.float32)).to(dev)
centre = (states.sum(dim=(1, 2, 3)) * 0.5 + atoms / 2).clamp(3, atoms - 3).reshape(-1, 1)
targets = torch.exp(-0.5 * ((torch.arange(atoms, device=dev).reshape(1, -1) - centre) / 2.0) ** 2)
targets[:, :2] = 0.0
targets = (targets / targets.sum(1, keepdim=True)).contiguous()
weights = torch.from_numpy(rng.integers(10, 200, size=(n, 1)).astype(np.float32)).to(dev)
weights = weights / weights.mean()
summary = dict(rows=n, slab=args.slab, atoms=atoms, seed=args.seed, parent_commit=args.package_root != ROOT)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


ewc = None
if not args.plain_only:
    lib = _lib.lib()
    mdl = MD.Model_Dist(atoms=atoms, seed=0, backend="hip")
    P = mdl.flat_params().clone()
    s8 = states[:, 0, 2:].reshape(n, 200).to(torch.int8).contiguous()
    w = weights.reshape(n).contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    ws_f = torch.empty(lib.tm_distnet_fit_fisher_workspace(args.slab, atoms), device=dev)
    ws_g = torch.empty(lib.tm_distnet_fit_workspace(1024, atoms), device=dev)
    fisher, grad, loss = torch.empty(P.numel(), device=dev), torch.empty(P.numel(), device=dev), torch.empty(2, device=dev)
    idx = torch.arange(n, dtype=torch.int64, device=dev)

    def fisher_pass():
        _lib.check(lib.tm_distnet_fit_fisher(P.data_ptr(), s8.data_ptr(), targets.data_ptr(), atoms, w.data_ptr(), None, n, args.slab,
                                             atoms, 1, fisher.data_ptr(), ws_f.data_ptr(), stream), "tm_distnet_fit_fisher")

    def grad_calls():
        for k in range(n // 1024):
            _lib.check(lib.tm_distnet_fit_grad(P.data_ptr(), s8.data_ptr(), targets.data_ptr(), atoms, w.data_ptr(),
                                               idx.data_ptr() + 8 * 1024 * k, 1024, atoms, 1, grad.data_ptr(), loss.data_ptr(),
                                               ws_g.data_ptr(), stream), "tm_distnet_fit_grad")

    # warm-up of every shape, then the legs alternated
    fisher_pass(); grad_calls(); torch.cuda.synchronize()
    t_f, t_g = [], []
    for _ in range(args.reps):
        t_f.append(event_ms(fisher_pass))
        t_g.append(event_ms(grad_calls))
    assert bool(torch.isfinite(fisher).all()) and float(fisher.max()) > 0
    summary.update(fisher_pass_ms=spread(t_f), grad_calls_ms=dict(spread(t_g), calls=n // 1024, batch=1024),
                   fisher_over_grad=float(np.median(t_f) / np.median(t_g)), value_net_fisher_over_grad=1.014)
    print(json.dumps(summary), flush=True)
    g = torch.Generator().manual_seed(1)
    ewc = dict(fisher=fisher.clone(), anchor=(P.cpu() + 0.01 * torch.randn(P.numel(), generator=g)).to(dev), lam=1.0)

# ---- the penalty inside a replayed iteration ----
data = [states, targets, weights]
legs = ("plain",) if args.plain_only else ("plain", "ewc_dist")
models = {leg: MD.Model_Dist(atoms=atoms, seed=0, backend="hip") for leg in legs}
rows = []
for blk in range(-1, args.blocks):      # block -1 warms the legs up and is not reported
    for leg in legs:
        kw = dict(iters_per_val=10 ** 9, batch_size=1024, log=False, early_stopping=False, fit_backend="hip_dist",
                  **(dict(ewc_dist=ewc) if leg == "ewc_dist" else {}))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = models[leg].train_data(data, max_iters=args.block_iters, **kw)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        t1 = time.perf_counter()
        short = models[leg].train_data(data, max_iters=4, **kw)
        torch.cuda.synchronize(); ds = time.perf_counter() - t1
        if blk >= 0:
            rows.append(dict(block=blk, leg=leg, iters=res["iters"], graph_replay=res["graph_replay"],
                             ms_per_iter=1e3 * (dt - ds) / (res["iters"] - short["iters"]), setup_ms=1e3 * ds))
            print(rows[-1], flush=True)
ms = {leg: [r["ms_per_iter"] for r in rows if r["leg"] == leg] for leg in legs}
it = dict(batch=1024, block_iters=args.block_iters, blocks=rows, plain_ms=spread(ms["plain"]),
          note="a block = one train_data call of block_iters iterations followed by the same call with max_iters=4; "
               "ms_per_iter is the difference over the iterations between them")
if not args.plain_only:
    it.update(ewc_dist_ms=spread(ms["ewc_dist"]), penalty_ms=float(np.median(ms["ewc_dist"]) - np.median(ms["plain"])),
              value_net_penalty_ms=0.0089)
summary["iteration"] = with_baseline(it)
print(json.dumps({k: v for k, v in it.items() if k not in ("blocks", "parent_blocks")}), flush=True)
os.makedirs(os.path.dirname(out_json), exist_ok=True)
with open(out_json, "w") as f:
    json.dump(summary, f, indent=1)
