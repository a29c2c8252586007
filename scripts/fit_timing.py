"""Where a fit's time goes (one MI355X): train_data on a synthetic replay set of the online run's size, eager and replayed from
the graph, and its parts on their own (a validation pass, a checkpoint save).
    python scripts/fit_timing.py [tuples] [--fit_backend {torch,hip}]
    python scripts/fit_timing.py [tuples] --blocks 3 --json OUT      the two fit backends alternated in blocks of graph-replayed
                                                                     iterations (no validation inside), one JSON file
    python scripts/fit_timing.py [tuples] --head --blocks 3 --json OUT   the distributional head (50 atoms), three legs alternated:
                                                                     torch autograd + torch.optim.Adam, eager (the default path);
                                                                     torch autograd + FusedAdam, replayed; hip_dist, replayed
    python scripts/fit_timing.py [tuples] --head --eager-iters 30 --fit_backend B    eager iterations of one leg alone (for a
                                                                     kernel trace)
    python scripts/fit_timing.py --validation [--head] --rows 25000,50000 --blocks 3 --json OUT
                                                                     one validation pass of that many held-out rows, torch
                                                                     (train.validation_loss) and hip (HipFit.validate: the C call
                                                                     and its one .cpu()) alternated in blocks; the hip pass at
                                                                     each of --slabs; and whole fits of 10 x rows tuples (1 300
                                                                     iterations, iters_per_val=100) under either backend
    python scripts/fit_timing.py [tuples] --fit_backend hip --validation_backend hip     the default mode's fits, validated on HIP"""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tetris_mcts_amd import model as M, train as T  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("tuples", nargs="?", type=int, default=250000)
ap.add_argument("--fit_backend", default="torch", choices=("torch", "hip", "hip_dist"))
ap.add_argument("--head", action="store_true", help="time the distributional head's fit (Model_Dist, 50 atoms) instead of the value net's")
ap.add_argument("--eager-iters", type=int, default=0, help="with --head: run this many eager iterations of --fit_backend and stop")
ap.add_argument("--blocks", type=int, default=0, help="alternate torch / hip in this many blocks each and stop")
ap.add_argument("--block-iters", type=int, default=1000)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--json", default=None)
ap.add_argument("--validation_backend", default="torch", choices=("torch", "hip"), help="how the default mode's fits validate (hip needs --fit_backend hip)")
ap.add_argument("--validation", action="store_true", help="time validation passes and whole fits under both validation backends and stop")
ap.add_argument("--rows", default="25000,50000", help="with --validation: held-out rows of a pass (the fits hold ten times as many tuples)")
ap.add_argument("--slabs", default="1024,2048,4096,8192", help="with --validation: the slabs the hip pass is also timed at")
ap.add_argument("--passes", type=int, default=5, help="with --validation: passes per block")
ap.add_argument("--fit-iters", type=int, default=1300, help="with --validation: iterations of a whole fit (0: no whole fits)")
args = ap.parse_args()
if args.validation_backend == "hip" and args.fit_backend == "torch":
    ap.error("--validation_backend hip needs --fit_backend hip (or hip_dist with --head)")
if args.fit_backend == "hip_dist" and not args.head:
    ap.error("--fit_backend hip_dist is the distributional head's: it needs --head")
n = args.tuples
out_json = os.path.abspath(args.json) if args.json else None
rng = np.random.default_rng(0)


def synthetic(n, head):
    """the synthetic replay set of the modes below: a learnable target that follows the board"""
    if head:
        x = torch.zeros(n, 1, 22, 10, device="cuda")
        x[:, :, 2:, :] = torch.from_numpy(rng.integers(-1, 2, size=(n, 1, 20, 10)).astype(np.float32)).cuda()
        centre = (x.sum(dim=(1, 2, 3)) * 0.5 + 25).clamp(2, 47).reshape(-1, 1)
        t = torch.softmax(-0.5 * (torch.arange(50, device="cuda").reshape(1, -1) - centre) ** 2 / 4.0, 1)
        t[:, :2] = 0.0
        return [x, t, torch.from_numpy(rng.integers(10, 200, size=(n, 1)).astype(np.float32)).cuda()]
    s = torch.from_numpy(rng.integers(-1, 2, size=(n, 1, 20, 10)).astype(np.float32)).cuda()
    return [s, (s.sum(dim=(1, 2, 3)) * 0.5 + 20).reshape(-1, 1), torch.full((n, 1), 4.0, device="cuda"),
            torch.from_numpy(rng.integers(10, 200, size=(n, 1)).astype(np.float32)).cuda()]


if args.validation:
    from tetris_mcts_amd.model_distributional import Model_Dist
    os.chdir("/tmp")
    os.environ["TM_TRAIN_GRAPH"] = "1"
    fit_backend = "hip_dist" if args.head else "hip"
    new_model = (lambda: Model_Dist(atoms=50, seed=0)) if args.head else (lambda: M.Model_VV(backend="torch", seed=0))
    loss_fn = T.dist_batch_loss if args.head else T.batch_loss

    def timed(fn, reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / reps
    summary = dict(head="model_distributional.Net" if args.head else "model.Net", fit_backend=fit_backend, passes_per_block=args.passes,
                   default_slab=T.VALIDATION_SLAB, chunk=T.VALIDATION_CHUNK, sizes=[],
                   note="a pass = one validation of `rows` held-out rows at fixed weights: torch is train.validation_loss (eager "
                        "forwards of 1 024 rows and one .cpu()), hip is HipFit.validate / HipDistFit.validate (one C call and one "
                        ".cpu()); a block times `passes_per_block` passes of each, torch first; block -1 warms both up and is not "
                        "reported.  whole_fit: one train_data call of fit_iters iterations on 10 x rows tuples with iters_per_val=100, "
                        "setup, validations and saves inside the time, the two validation backends alternated")
    for rows in [int(r) for r in args.rows.split(",")]:
        data = synthetic(10 * rows, args.head)
        norm = list(data)
        norm[-1] = norm[-1] / norm[-1].mean()
        val, train = [d[-rows:] for d in norm], [d[:4096] for d in norm]
        mdl = new_model()
        opt = mdl._fused_optimizer() if args.head else mdl._optimizer()
        Fit = T.HipDistFit if args.head else T.HipFit
        fits = {s: Fit(mdl.model, opt, train, 1024, val=val, val_slab=s) for s in sorted({int(s) for s in args.slabs.split(",")} | {T.VALIDATION_SLAB})}
        hip = fits[T.VALIDATION_SLAB]
        got_t = T.validation_loss(mdl.model, val, True, loss_fn=loss_fn)
        got_h = T.combine_chunk_rows(hip.validate(True))
        size = dict(rows=rows, torch_loss=got_t, hip_loss=got_h, blocks=[], slabs=[])
        for blk in range(-1, max(args.blocks, 3)):
            row = dict(block=blk, torch_ms=timed(lambda: T.validation_loss(mdl.model, val, True, loss_fn=loss_fn), args.passes),
                       hip_ms=timed(lambda: hip.validate(True), args.passes))
            if blk >= 0:
                size["blocks"].append(row)
                print(rows, row, flush=True)
        for s, f in fits.items():
            f.validate(True)
            size["slabs"].append(dict(slab=f.val_slab, hip_ms=min(timed(lambda: f.validate(True), args.passes) for _ in range(3))))
            print(rows, size["slabs"][-1], flush=True)
        for k in ("torch_ms", "hip_ms"):
            v = [b[k] for b in size["blocks"]]
            size[k] = dict(min=min(v), max=max(v), median=float(np.median(v)))
        size["torch_over_hip"] = size["torch_ms"]["median"] / size["hip_ms"]["median"]
        del fits, hip
        if args.fit_iters > 0:
            models = {vb: new_model() for vb in ("torch", "hip")}
            size["whole_fit"] = []
            for blk in range(-1, max(args.blocks, 3)):
                for vb in ("torch", "hip"):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    res = models[vb].train_data(list(data), iters_per_val=100, batch_size=args.batch, max_iters=args.fit_iters, log=False,
                                                early_stopping=False, fit_backend=fit_backend, validation_backend=vb)
                    torch.cuda.synchronize(); dt = time.perf_counter() - t0
                    if blk >= 0:
                        size["whole_fit"].append(dict(block=blk, validation_backend=vb, iters=res["iters"], graph_replay=res["graph_replay"],
                                                      ms_per_iter=1e3 * dt / res["iters"]))
                        print(rows, size["whole_fit"][-1], flush=True)
            med = {vb: float(np.median([r["ms_per_iter"] for r in size["whole_fit"] if r["validation_backend"] == vb])) for vb in ("torch", "hip")}
            size["whole_fit_ms_per_iter"] = med
            size["whole_fit_torch_over_hip"] = med["torch"] / med["hip"]
            del models
        summary["sizes"].append(size)
        print(json.dumps({k: v for k, v in size.items() if k not in ("blocks", "whole_fit")}), flush=True)
        del data, norm, val, train
        torch.cuda.empty_cache()
    if out_json:
        os.makedirs(os.path.dirname(out_json), exist_ok=True)
        with open(out_json, "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(0)
if args.head:
    from tetris_mcts_amd.model_distributional import Model_Dist
    os.chdir("/tmp")      # (as the value net's mode below: nothing a fit writes lands in the repository)
    atoms = 50
    x = torch.zeros(n, 1, 22, 10, device="cuda")
    x[:, :, 2:, :] = torch.from_numpy(rng.integers(-1, 2, size=(n, 1, 20, 10)).astype(np.float32)).cuda()
    centre = (x.sum(dim=(1, 2, 3)) * 0.5 + 25).clamp(2, 47).reshape(-1, 1)      # a learnable target: a bump whose place follows the board
    targets = torch.softmax(-0.5 * (torch.arange(atoms, device="cuda").reshape(1, -1) - centre) ** 2 / 4.0, 1)
    targets[:, :2] = 0.0                                                           # empty low bins, rows that do not sum to 1
    w = torch.from_numpy(rng.integers(10, 200, size=(n, 1)).astype(np.float32)).cuda()
    data = [x, targets, w]
    if args.eager_iters > 0:
        os.environ["TM_TRAIN_GRAPH"] = "0"
        mdl = Model_Dist(atoms=atoms, seed=0)
        res = mdl.train_data(data, iters_per_val=10 ** 9, batch_size=args.batch, max_iters=args.eager_iters, log=False,
                             early_stopping=False, fit_backend=args.fit_backend)
        torch.cuda.synchronize()
        print(res, flush=True)
        sys.exit(0)
    legs = ("torch_adam_eager", "torch_fusedadam_replayed", "hip_dist_replayed")
    models = {leg: Model_Dist(atoms=atoms, seed=0) for leg in legs}
    models["torch_fusedadam_replayed"]._fused_optimizer()
    rows = []
    for blk in range(-1, max(args.blocks, 1)):      # block -1 warms every leg up and is not reported
        for leg in legs:
            os.environ["TM_TRAIN_GRAPH"] = "0" if leg == "torch_adam_eager" else "1"
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = models[leg].train_data(data, iters_per_val=10 ** 9, batch_size=args.batch, max_iters=args.block_iters, log=False,
                                         early_stopping=False, fit_backend="hip_dist" if leg == "hip_dist_replayed" else "torch")
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            # the same call cut short after its setup (the per-fit checks, the int8 copy, three eager iterations, the capture and
            # one replay): the difference is the time of the iterations alone
            t1 = time.perf_counter()
            short = models[leg].train_data(data, iters_per_val=10 ** 9, batch_size=args.batch, max_iters=4, log=False,
                                           early_stopping=False, fit_backend="hip_dist" if leg == "hip_dist_replayed" else "torch")
            torch.cuda.synchronize(); ds = time.perf_counter() - t1
            if blk >= 0:
                rows.append(dict(block=blk, leg=leg, iters=res["iters"], graph_replay=res["graph_replay"],
                                 ms_per_iter=1e3 * (dt - ds) / (res["iters"] - short["iters"]),
                                 ms_per_iter_whole_call=1e3 * dt / res["iters"], setup_ms=1e3 * ds))
                print(rows[-1], flush=True)
    ms = {leg: [r["ms_per_iter"] for r in rows if r["leg"] == leg] for leg in legs}
    med = {leg: float(np.median(ms[leg])) for leg in legs}
    summary = dict(head="model_distributional.Net", atoms=atoms, tuples=n, batch=args.batch, block_iters=args.block_iters, blocks=rows,
                   **{leg + "_ms": dict(min=min(ms[leg]), max=max(ms[leg]), median=med[leg]) for leg in legs},
                   torch_adam_eager_over_hip_dist=med[legs[0]] / med[legs[2]], torch_fusedadam_replayed_over_hip_dist=med[legs[1]] / med[legs[2]],
                   note="a block = one train_data call of block_iters iterations followed by the same call with max_iters=4; "
                        "ms_per_iter is the difference over the iterations between them (the per-fit checks, the int8 copy, the three "
                        "eager iterations and the capture fall out), ms_per_iter_whole_call the first call over all of its iterations, "
                        "setup_ms the short call")
    print(json.dumps({k: v for k, v in summary.items() if k != "blocks"}), flush=True)
    if out_json:
        os.makedirs(os.path.dirname(out_json), exist_ok=True)
        with open(out_json, "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(0)
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
                         early_stopping=False, fit_backend=args.fit_backend, validation_backend=args.validation_backend)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print("graph=%s: %d iterations in %.3f s = %.3f ms per iteration (13 validations of %d rows and the saves included) %s" % (mode, res["iters"], dt, 1e3 * dt / res["iters"], n // 10, res), flush=True)
    val = [d[-n // 10:] for d in (states, values, variances, weights / weights.mean())]
    if args.validation_backend == "hip":      # the C call and its one .cpu(), at the weights the fit left in the flat buffer
        hip = T.HipFit(mdl.model, mdl._optimizer(), [d[:4096] for d in val], 1024, val=val)
        one_pass = lambda: hip.validate(True)      # noqa: E731
    else:
        one_pass = lambda: T.validation_loss(mdl.model, val, True)      # noqa: E731
    one_pass()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(5): one_pass()
    torch.cuda.synchronize(); print("   one validation pass (%s): %.1f ms" % (args.validation_backend, 1e3 * (time.perf_counter() - t0) / 5))
    t0 = time.perf_counter()
    for _ in range(5): mdl.save(verbose=False)
    print("   one checkpoint save: %.1f ms" % (1e3 * (time.perf_counter() - t0) / 5))
    # the iterations alone
    os.environ["TM_TRAIN_GRAPH"] = mode
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = mdl.train_data([states, values, variances, weights], iters_per_val=10 ** 9, batch_size=1024, max_iters=1000, log=False, early_stopping=False,
                         fit_backend=args.fit_backend, validation_backend=args.validation_backend)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print("   1000 iterations without validation: %.3f ms per iteration" % (1e3 * dt / 1000), flush=True)
