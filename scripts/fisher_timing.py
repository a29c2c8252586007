"""What elastic weight consolidation costs (one MI355X): the Fisher pass and the penalty inside a replayed iteration.
    python scripts/fisher_timing.py [--rows 65536] [--slab 1024] [--reps 5] [--block-iters 1000] [--json profiles/fisher_timing.json]

The pass: tm_valuenet_fit_fisher over `rows` fresh rows (from a seed) at `slab`, against rows / 1024 calls of tm_valuenet_fit_grad
at batch 1 024 over the same rows in the same process - by count the same matrix work plus the squaring, so the ratio is what is
reported - and against torch per-sample gradients on the GPU (torch.func.vmap of grad over chunks of 256 rows where it runs on
this net, else a one-row autograd loop; either over --torch-rows rows and SCALED to `rows`, and marked as scaled).  Device
events, every shape warmed up, the legs alternated `reps` times, minimum / median / maximum reported.

The penalty: train_data(fit_backend="hip") at batch 1 024 replayed from the graph, with and without `ewc`, alternated in blocks of
--block-iters iterations; a block's time is the call's minus the same call cut short after its setup (fit_timing.py's rule)."""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tetris_mcts_amd import _lib, model as M, train as T  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--slab", type=int, default=1024)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--torch-rows", type=int, default=1024)
ap.add_argument("--block-iters", type=int, default=1000)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "fisher_timing.json"))
args = ap.parse_args()
out_json = os.path.abspath(args.json)
os.chdir("/tmp")      # nothing a fit writes lands in the repository
os.environ["TM_TRAIN_GRAPH"] = "1"
n, dev = args.rows, torch.device("cuda")
assert n % 1024 == 0
rng = np.random.default_rng(args.seed)
states = torch.from_numpy(rng.integers(-1, 2, size=(n, 1, 20, 10)).astype(np.float32)).to(dev)
values = (states.sum(dim=(1, 2, 3)) * 0.5 + 20).reshape(-1, 1)
variances = torch.full((n, 1), 4.0, device=dev)
weights = torch.from_numpy(rng.integers(10, 200, size=(n, 1)).astype(np.float32)).to(dev)
weights = weights / weights.mean()
mdl = M.Model_VV(backend="torch", seed=0)
with torch.no_grad():
    mdl.model.out_ubound.copy_(torch.stack([values.max(), variances.max()]))
lib = _lib.lib()
P = mdl._flat_learnable()
bounds = torch.cat([mdl.model.out_ubound.detach().reshape(2), mdl.model.out_lbound.detach().reshape(2)]).float().contiguous()
s8 = states.reshape(n, 200).to(torch.int8).contiguous()
val, var, w = (t.reshape(n).contiguous() for t in (values, variances, weights))
stream = torch.cuda.current_stream().cuda_stream
ws_f = torch.empty(lib.tm_valuenet_fit_fisher_workspace(args.slab), device=dev)
ws_g = torch.empty(lib.tm_valuenet_fit_workspace(1024), device=dev)
fisher, grad, loss = torch.empty(P.numel(), device=dev), torch.empty(P.numel(), device=dev), torch.empty(2, device=dev)
idx = torch.arange(n, dtype=torch.int64, device=dev)


def fisher_pass():
    _lib.check(lib.tm_valuenet_fit_fisher(P.data_ptr(), bounds.data_ptr(), s8.data_ptr(), val.data_ptr(), var.data_ptr(), w.data_ptr(), None,
                                          n, args.slab, 1, 0.1, fisher.data_ptr(), ws_f.data_ptr(), stream), "tm_valuenet_fit_fisher")


def grad_calls():
    for k in range(n // 1024):
        _lib.check(lib.tm_valuenet_fit_grad(P.data_ptr(), bounds.data_ptr(), s8.data_ptr(), val.data_ptr(), var.data_ptr(), w.data_ptr(),
                                            idx.data_ptr() + 8 * 1024 * k, 1024, 1, 0.1, grad.data_ptr(), loss.data_ptr(), ws_g.data_ptr(),
                                            stream), "tm_valuenet_fit_grad")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(v):
    return dict(min=min(v), median=float(np.median(v)), max=max(v), reps=len(v))


# ---- torch per-sample gradients on the GPU ----
tr = min(args.torch_rows, n)
params = {k: v.detach() for k, v in mdl.model.named_parameters()}


def row_loss(p, s, v, va, wt):
    out = torch.func.functional_call(mdl.model, p, (s.unsqueeze(0),))
    return (wt * T.gaussian_kl(out[:, 1:2], out[:, 0:1], va.clamp(min=0.1).reshape(1, 1), v.reshape(1, 1))).sum()


def torch_vmap():
    acc = {k: torch.zeros_like(v) for k, v in params.items() if v.requires_grad}
    learn = {k: v for k, v in params.items() if k in acc}
    rest = {k: v for k, v in params.items() if k not in acc}
    f = torch.func.vmap(torch.func.grad(lambda p, s, v, va, wt: row_loss({**p, **rest}, s, v, va, wt)), in_dims=(None, 0, 0, 0, 0))
    for a in range(0, tr, 256):
        g = f(learn, states[a:a + 256], val[a:a + 256], var[a:a + 256], w[a:a + 256])
        for k in acc:
            acc[k] += (g[k] ** 2).sum(0) / tr
    return acc


def torch_loop():
    acc = [torch.zeros_like(p) for p in mdl.model.parameters() if p.requires_grad]
    learn = [p for p in mdl.model.parameters() if p.requires_grad]
    for r in range(min(tr, 256)):
        for p in learn:
            p.grad = None
        mean, _ = T.batch_loss(mdl.model, [states[r:r + 1], values[r:r + 1], variances[r:r + 1], weights[r:r + 1]], True)
        mean.backward()
        with torch.no_grad():
            for a, p in zip(acc, learn):
                a += p.grad * p.grad / min(tr, 256)
    return acc


mdl.model.eval()
try:
    torch_vmap()
    torch_leg, torch_fn, torch_n = "torch.func.vmap(grad), chunks of 256 rows", torch_vmap, tr
except Exception as e:      # noqa: BLE001 - whatever vmap refuses on this net: the loop is the reference's own form
    print("vmap(grad) does not run here (%s: %s): the one-row loop" % (type(e).__name__, str(e).splitlines()[0][:120]), flush=True)
    torch_leg, torch_fn, torch_n = "one-row autograd loop", torch_loop, min(tr, 256)
# warm-up of every shape, then the legs alternated
fisher_pass(); grad_calls(); torch_fn(); torch.cuda.synchronize()
t_f, t_g, t_t = [], [], []
for _ in range(args.reps):
    t_f.append(event_ms(fisher_pass))
    t_g.append(event_ms(grad_calls))
    t_t.append(event_ms(torch_fn))
assert bool(torch.isfinite(fisher).all()) and float(fisher.max()) > 0
summary = dict(rows=n, slab=args.slab, seed=args.seed,
               fisher_pass_ms=spread(t_f), grad_calls_ms=dict(spread(t_g), calls=n // 1024, batch=1024),
               fisher_over_grad=float(np.median(t_f) / np.median(t_g)),
               torch_per_sample=dict(leg=torch_leg, rows_timed=torch_n, ms=spread(t_t), scaled=True,
                                     ms_scaled_to_rows=float(np.median(t_t)) * n / torch_n),
               torch_scaled_over_fisher=float(np.median(t_t)) * n / torch_n / float(np.median(t_f)))
print(json.dumps(summary), flush=True)

# ---- the penalty inside a replayed iteration ----
data = [states, values, variances, weights]
g = torch.Generator().manual_seed(1)
ewc = dict(fisher=fisher.clone(), anchor=(P.cpu() + 0.01 * torch.randn(P.numel(), generator=g)).to(dev), lam=1.0)
models = {leg: M.Model_VV(backend="torch", seed=0) for leg in ("plain", "ewc")}
rows = []
for blk in range(-1, args.blocks):      # block -1 warms both legs up and is not reported
    for leg in ("plain", "ewc"):
        kw = dict(iters_per_val=10 ** 9, batch_size=1024, log=False, early_stopping=False, fit_backend="hip",
                  **(dict(ewc=ewc) if leg == "ewc" else {}))
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
ms = {leg: [r["ms_per_iter"] for r in rows if r["leg"] == leg] for leg in ("plain", "ewc")}
summary["iteration"] = dict(batch=1024, block_iters=args.block_iters, blocks=rows, plain_ms=spread(ms["plain"]), ewc_ms=spread(ms["ewc"]),
                            penalty_ms=float(np.median(ms["ewc"]) - np.median(ms["plain"])),
                            note="a block = one train_data call of block_iters iterations followed by the same call with max_iters=4; "
                                 "ms_per_iter is the difference over the iterations between them")
print(json.dumps({k: v for k, v in summary["iteration"].items() if k != "blocks"}), flush=True)
os.makedirs(os.path.dirname(out_json), exist_ok=True)
with open(out_json, "w") as f:
    json.dump(summary, f, indent=1)
