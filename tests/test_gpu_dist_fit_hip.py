"""The HIP gradient step of the distributional head's fit on the GPU (csrc/distnet_fit.hip, tm_adam_step,
train_data(fit_backend="hip_dist")).

Accuracy is measure B of DESIGN.md section 6 applied to gradients (tests/dist_fit_cases.py): per parameter tensor, and for the loss
mean and std,  max|g_hip - g64| <= 8 max|g_torch_fp32 - g64| + 4 u max|g64|  with torch's CPU autograd of Net.log_prob +
Model_Dist.loss in fp64 and fp32 as g64 and g_torch_fp32.  Every figure is printed before it is asserted (pytest -s shows them)."""
import hashlib
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import dist_fit_cases as DC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the kernels' blocking constants along the batch (csrc/distnet_fit.hip): SPW = 4 (and k_df_head's four samples a workgroup), the
# 32-sample tile / HEAD_CHUNK / K chunk, FC_KC = 256, and the 16 groups of k_fit_reduce over B and over ceil(B / 4) partials;
# DC.BATCHES holds one batch at, below and above each, next to 1, 2 and 65 (the cases themselves are built at the first use)
assert ({1, 2, 31, 32, 33, 65, 256} | {DC.SPW + d for d in (-1, 0, 1)} | {DC.FC_KC + d for d in (-1, 0, 1)}
        | {DC.RED_G + d for d in (-1, 0, 1)} | {60, 64, 65}) <= set(DC.BATCHES)
assert (DC.SPW, DC.TILE, DC.FC_KC, DC.RED_G, DC.RED_G_FC) == (4, 32, 256, 16, 4)
# DC.LARGE_BATCHES: the ceil(B / 32) partials of the FC bias sums below, at and above the 16 groups (15 / 16 / 17 partials), and
# the ceil(B / 256) splits of the FC weight gradients at 3 (a split of one sample), 4 (ragged and full) and 5 > the 4 groups of
# k_fit_reduce<4> (a last split of one sample); 1 024 is the batch of every DistValueSim fit
assert set(DC.LARGE_BATCHES) == {480, 512, 513, 1000, 1024, 1025} and not set(DC.LARGE_BATCHES) & set(DC.BATCHES)
assert [-(-b // DC.TILE) for b in (480, 512, 513)] == [DC.RED_G - 1, DC.RED_G, DC.RED_G + 1]
assert [-(-b // DC.FC_KC) for b in (513, 1000, 1024, 1025)] == [3, DC.RED_G_FC, DC.RED_G_FC, DC.RED_G_FC + 1]
assert (513 % DC.FC_KC, 1000 % DC.FC_KC, 1025 % DC.FC_KC) == (1, 7 * DC.TILE + 8, 1)
assert max(-(-b // DC.FC_KC) for b in DC.BATCHES) == 2 and max(-(-b // DC.TILE) for b in DC.BATCHES) == 9          # what BATCHES reaches
assert DC.case_names()[-len(DC.large_cases(names_only=True)):] == list(DC.large_cases(names_only=True))
assert {"fixture, batch %d" % b for b in DC.LARGE_BATCHES} | {"seed7, batch 513, stride 64", "seed64, batch 513",
                                                               "fitted, batch 1024, unweighted, idx NULL"} == set(DC.large_cases(names_only=True))


@pytest.mark.parametrize("name", DC.case_names())
def test_gradients_and_loss_within_measure_b(name):
    case = DC.cases()[name]
    torch.set_num_threads(16)
    g64, l64 = DC.reference(name, case, torch.float64)
    g32, l32 = DC.reference(name, case, torch.float32)
    got, loss = DC.hip_grad(case)
    assert np.isfinite(got).all() and np.isfinite(loss[0])
    bad = []
    for t, a, b32, b64 in zip(DC.TENSORS, DC.split(got, case["atoms"]), g32, g64):
        if case["atoms"] == 1:          # log p = 0: the gradient is identically zero, in both precisions and here
            assert np.abs(b64).max() == 0 and np.abs(b32).max() == 0 and (a == 0).all(), (name, t, np.abs(a).max())
            continue
        assert np.abs(b64).max() > 0 and np.abs(b32 - b64).max() > 0, (name, t, "the rule's denominator")
        err, bound, need = DC.measure(a, b32, b64)
        print("%-44s %-13s err %.3e  bound %.3e  torch fp32 %.3e  needs M = %.2f" % (name, t, err, bound, np.abs(b32 - b64).max(), need))
        if not err <= bound:
            bad.append((t, err, bound, need))
    for k, what in enumerate(("loss mean", "loss std")):
        if case["batch"] == 1 and k == 1:
            assert math.isnan(loss[1]) and math.isnan(l64[1])          # one sample: torch.std_mean's n - 1 gives NaN
            continue
        err, bound, need = DC.measure([loss[k]], [l32[k]], [l64[k]])
        print("%-44s %-13s err %.3e  bound %.3e  needs M = %.2f" % (name, what, err, bound, need))
        if not err <= bound:
            bad.append((what, err, bound, need))
    assert not bad, (name, bad)


def test_gradient_is_overwritten_not_accumulated():
    case = DC.digest_case()
    a, _ = DC.hip_grad(case, grad_fill=123.0)
    b, _ = DC.hip_grad(case, grad_fill=-7.0)
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all()


def test_same_bits_from_call_to_call_and_from_process_to_process():
    case = DC.digest_case()
    g1, l1 = DC.hip_grad(case)
    g2, l2 = DC.hip_grad(case)
    assert g1.tobytes() == g2.tobytes() and l1.tobytes() == l2.tobytes()
    for big in ("fixture, batch 257", "fixture, batch 1025"):               # 1 025: groups of the second stages with two terms
        b1, b2 = DC.hip_grad(DC.cases()[big]), DC.hip_grad(DC.cases()[big])
        assert b1[0].tobytes() == b2[0].tobytes() and b1[1].tobytes() == b2[1].tobytes(), big
    mine = hashlib.sha256(g1.tobytes() + l1.tobytes()).hexdigest()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dist_fit_cases.py"), "digest"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)                                 # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    theirs = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
    assert theirs == [mine]


@pytest.mark.parametrize("name,tstride", [("fixture, batch 1", None), ("fixture, batch 33", None), ("seed7, batch 33, stride 64", 7),
                                          ("fixture, batch 257", None), ("fixture, batch 1025", None)])
def test_the_call_writes_only_where_it_says(name, tstride):
    """workspace (exactly tm_distnet_fit_workspace(batch, atoms) floats), grad (the parameter count) and loss (2) carved out of one
    device tensor, each on a 16-byte boundary with 64 KiB of guard before, between and after (fit_hip_cases.Arena): after the call
    every guard byte holds its pattern, every input (params, states, targets, weight, idx) is bit-identical to its copy from before
    the call, and grad and loss are bit for bit what the call gives with buffers of the allocator's choosing.  50 atoms, and 7
    atoms with a target stride of 7 (no padding between the rows).  Reads past an input cannot be seen this way."""
    case = DC.cases()[name]
    if tstride is not None:
        case = dict(case, tstride=tstride)
        assert case["atoms"] == tstride == 7
    arena = DC.FC.Arena()
    got, loss = DC.hip_grad(case, place=arena)
    arena.check()
    assert set(arena.inputs) == {"params", "states", "targets", "weight", "idx"}
    print("%-28s arena of %d floats, segments (offset, floats) %s" % (name, arena.arena.numel(), arena.segments))
    plain, plain_loss = DC.hip_grad(case)
    assert np.isfinite(got).all() and got.tobytes() == plain.tobytes()
    assert loss.tobytes() == plain_loss.tobytes() and np.isfinite(loss[0]) and np.isfinite(loss[1]) == (case["batch"] > 1)


def test_refused_arguments_launch_nothing():
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda")
    B, atoms = 8, 50
    n = DC.n_params(atoms)
    P = torch.zeros(n, device=dev)
    s8 = torch.zeros(B, 200, dtype=torch.int8, device=dev)
    t = torch.full((B, atoms), 1.0 / atoms, device=dev)
    w = torch.ones(B, device=dev)
    grad = torch.full((n,), 5.0, device=dev)
    loss = torch.full((2,), 5.0, device=dev)
    ws = torch.zeros(lib.tm_distnet_fit_workspace(B, atoms), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    full = [P.data_ptr(), s8.data_ptr(), t.data_ptr(), atoms, w.data_ptr(), None, B, atoms, 1, grad.data_ptr(), loss.data_ptr(),
            ws.data_ptr(), st]
    for k in (0, 1, 2, 4, 9, 10, 11):
        args = list(full)
        args[k] = None
        assert lib.tm_distnet_fit_grad(*args) == 1, k           # hipErrorInvalidValue
    for k, bad in ((6, 0), (6, -1), (7, 0), (7, 65), (7, -2)):
        args = list(full)
        args[k] = bad
        assert lib.tm_distnet_fit_grad(*args) == 1, (k, bad)
    torch.cuda.synchronize()
    assert bool((grad == 5.0).all()) and bool((loss == 5.0).all())
    assert lib.tm_distnet_fit_grad(*full) == 0                  # ... and the same arguments complete are accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()) and not bool((grad == 5.0).any())


@pytest.mark.parametrize("kw", [dict(lr=1e-4, eps=1e-5, amsgrad=True), dict(lr=1e-3, eps=1e-8, amsgrad=False, weight_decay=1e-2)])
def test_adam_kernel_within_eight_times_torchs_fp32_error(kw):
    """tm_adam_step (through FusedAdam on GPU tensors): 6 steps on fixed random gradients against fp64 Adam; the bound is 8x the
    error of torch.optim.Adam in fp32 on the CPU against the same fp64 run, plus 4 ulp of the parameter"""
    from tetris_mcts_amd.train import FusedAdam
    rng = np.random.default_rng(3)
    shapes = [(300, 7), (1000,), (5,)]
    p0 = [rng.normal(0, 1, s) for s in shapes]
    grads = [[rng.normal(0, 1, s) * 10.0 ** rng.integers(-4, 1) for s in shapes] for _ in range(6)]
    p64 = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in p0]
    p32 = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float32)) for p in p0]
    pg = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float32, device="cuda")) for p in p0]
    o64, o32, og = torch.optim.Adam(p64, **kw), torch.optim.Adam(p32, **kw), FusedAdam(pg, **kw)
    assert og.fused() and og.flat_grad() is not None
    for gs in grads:
        for a, b, c, g in zip(p64, p32, pg, gs):
            g32 = torch.tensor(g, dtype=torch.float32)
            a.grad, b.grad = g32.double(), g32.clone()
            c.grad.copy_(g32.cuda())
        o64.step()
        o32.step()
        og.step()
    torch.cuda.synchronize()
    for a, b, c in zip(p64, p32, pg):
        ref, own, got = a.detach().numpy(), b.detach().double().numpy(), c.detach().cpu().double().numpy()
        err, torch_err, floor = np.abs(got - ref).max(), np.abs(own - ref).max(), 4 * DC.U * np.abs(ref).max()
        print("adam %s: err %.3e, torch fp32 %.3e, floor %.3e" % (tuple(a.shape), err, torch_err, floor))
        assert err <= 8 * torch_err + floor, (tuple(a.shape), err, torch_err, floor)
    assert np.abs(p64[0].detach().numpy() - p0[0]).max() > 1e-4           # ... and the parameters moved
    sd = og.state_dict()
    assert all(float(s["step"]) == 6.0 for s in sd["state"].values()) and og._flat["t"] == 6
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    # the state goes back into torch.optim.Adam and both take the same next step (to rounding)
    o2 = torch.optim.Adam(p32, **kw)
    with torch.no_grad():
        for b, c in zip(p32, pg):
            b.copy_(c.cpu())
    import copy
    o2.load_state_dict(copy.deepcopy({"state": {k: {kk: vv.cpu() for kk, vv in v.items()} for k, v in sd["state"].items()},
                                      "param_groups": sd["param_groups"]}))
    before = [c.detach().cpu().clone() for c in pg]
    for b, c, g in zip(p32, pg, grads[0]):
        g32 = torch.tensor(g, dtype=torch.float32)
        b.grad = g32.clone()
        c.grad.copy_(g32.cuda())
    o2.step()
    og.step()
    for b, c, p_before in zip(p32, pg, before):
        step = (b.detach() - p_before).abs().max()
        assert float((b.detach() - c.detach().cpu()).abs().max()) <= 1e-3 * float(step) + 4 * DC.U * float(b.detach().abs().max())


def _fit_set(n, atoms=50, seed=0):
    """a learnable set: the target is a bump whose place follows the number of filled cells; low bins empty, rows not renormalised"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 1, 22, 10), np.float32)
    x[:, :, 2:, :] = rng.integers(-1, 2, size=(n, 1, 20, 10))
    centre = np.clip(x.sum(axis=(1, 2, 3)) * 0.5 + atoms / 2, 3, atoms - 3).reshape(-1, 1)
    t = np.exp(-0.5 * ((np.arange(atoms).reshape(1, -1) - centre) / 2.0) ** 2)
    t[:, :2] = 0.0
    t = (t / t.sum(1, keepdims=True) * rng.uniform(0.9, 1.1, (n, 1))).astype(np.float32)
    w = rng.integers(1, 20, size=(n, 1)).astype(np.float32)
    return [x, t, w]


def test_eager_hip_dist_and_torch_fits_draw_the_same_batches_and_agree(monkeypatch):
    """TM_TRAIN_GRAPH=0, the same seed: 20 iterations of either backend draw the same indices and end on parameters that differ by
    no more than 2 % of the mean distance moved (the form of test_gpu_fit_hip's eager test)"""
    from tetris_mcts_amd.model_distributional import Model_Dist
    monkeypatch.setenv("TM_TRAIN_GRAPH", "0")
    data = _fit_set(3000)
    real_randint = torch.randint
    out = {}
    for backend in ("torch", "hip_dist"):
        draws = []

        def recording(*a, **k):
            r = real_randint(*a, **k)
            draws.append(r.detach().cpu().numpy().copy())
            return r
        torch.manual_seed(5)
        mdl = Model_Dist(atoms=50, seed=0, backend="torch")
        start = mdl.flat_params().cpu().numpy().astype(np.float64)
        monkeypatch.setattr(torch, "randint", recording)
        res = mdl.train_data(list(data), iters_per_val=1000, batch_size=256, max_iters=20, log=False, fit_backend=backend)
        monkeypatch.setattr(torch, "randint", real_randint)
        assert res["iters"] == 20 and res["graph_replay"] is False
        out[backend] = (draws, mdl.flat_params().cpu().numpy().astype(np.float64), start)
    d_t, d_h = out["torch"][0], out["hip_dist"][0]
    assert len(d_t) == len(d_h) == 20 and all(a.shape == (256,) and (a == b).all() for a, b in zip(d_t, d_h))
    moved = np.abs(out["torch"][1] - out["torch"][2])
    diff = np.abs(out["hip_dist"][1] - out["torch"][1])
    print("eager fits: diff max %.3e mean %.3e, moved max %.3e mean %.3e" % (diff.max(), diff.mean(), moved.max(), moved.mean()))
    assert moved.max() > 1e-3 and diff.max() <= 8e-3 and float(np.mean(diff)) <= 2e-2 * float(np.mean(moved))


def test_the_hip_dist_fit_replayed_from_a_hip_graph(monkeypatch):
    from tetris_mcts_amd import train as T
    from tetris_mcts_amd.model_distributional import Model_Dist
    monkeypatch.setenv("TM_TRAIN_GRAPH", "1")
    data = _fit_set(2000)
    torch.manual_seed(5)
    mdl = Model_Dist(atoms=50, seed=0, backend="hip")
    val = [torch.from_numpy(d[-200:]).cuda() for d in data]
    val[2] = val[2] / torch.from_numpy(data[2]).mean()
    with torch.no_grad():
        before = float(mdl.loss(*val)[0])
    r = mdl.train_data(data, iters_per_val=50, batch_size=256, max_iters=300, log=False, fit_backend="hip_dist")
    with torch.no_grad():
        after = float(mdl.loss(*val)[0])
    print("replayed hip_dist fit:", r, "validation loss", before, "->", after)
    assert r["graph_replay"] is True and (r["iters"] == 300 or r["iters"] % 50 == 0)
    assert isinstance(mdl.optimizer, T.FusedAdam) and mdl.optimizer._flat["t"] == r["iters"]
    assert float(mdl.optimizer.state_dict()["state"][0]["step"]) == r["iters"]
    assert after < before and r["best_validation"] < before, (before, after, r)          # the validation loss falls
    # the operand streams of the HIP head were dropped with the old weights: inference sees the fitted net
    d = mdl.inference_device(torch.zeros(4, 200, dtype=torch.int8, device="cuda"))[:, :50]
    x0 = torch.zeros(4, 1, 22, 10, device="cuda")
    assert torch.allclose(d, mdl.model(x0), atol=1e-5)
    # it stays fused: a later torch fit lands its autograd gradients in the flat buffer and is replayed too
    r2 = mdl.train_data(data, iters_per_val=50, batch_size=256, max_iters=20, log=False)
    assert r2["graph_replay"] is True and mdl.optimizer._flat["t"] == r["iters"] + 20


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q):
    import tempfile
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)                          # both ranks on the one device
    os.chdir(tempfile.mkdtemp())
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tetris_mcts_amd.model_distributional import Model_Dist
    mdl = Model_Dist(atoms=50, seed=0, backend="torch")
    start = mdl.flat_params().cpu().numpy().copy()
    gen = torch.Generator(device="cuda").manual_seed(99)
    res = mdl.train_data(_fit_set(2000), batch_size=256, iters_per_val=4, max_iters=8, generator=gen, log=False, fit_backend="hip_dist")
    q.put((rank, res["iters"], start, mdl.flat_params().cpu().numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_leave_bit_identical_weights():
    """two gloo ranks on the one GPU (two processes, as tests/test_gpu_two_ranks.py): a data-parallel hip_dist fit, 128 rows a rank"""
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res[0][1] == res[1][1] == 8
    assert res[0][3].tobytes() == res[1][3].tobytes()
    assert np.abs(res[0][3] - res[0][2]).max() > 1e-4          # ... and they moved


def test_an_index_outside_the_training_rows_is_refused_before_anything_is_launched():
    from tetris_mcts_amd import train as T
    from tetris_mcts_amd.model_distributional import Model_Dist
    dev = torch.device("cuda")
    mdl = Model_Dist(atoms=50, seed=0, backend="torch")
    batch = [torch.from_numpy(d).to(dev) for d in _fit_set(48)]
    n = 48
    fit = T.HipDistFit(mdl.model, mdl._fused_optimizer(), batch, n)
    fit.F["g"].fill_(3.0)
    for bad in (n, -1):
        idx = torch.arange(n, device=dev)
        idx[5] = bad
        with pytest.raises(ValueError, match="training rows"):
            fit.grad(idx, True)
    torch.cuda.synchronize()
    assert bool((fit.F["g"] == 3.0).all())
    fit.grad(torch.arange(n, device=dev), True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(fit.F["g"]).all()) and not bool((fit.F["g"] == 3.0).any())


def test_hip_dist_refusals_that_need_a_device():
    """what tests/test_dist_fit_hip.py cannot reach without a GPU: the agents' keyword with a store behind it, and the checks behind
    the CUDA one"""
    from tetris_mcts_amd import agents, train as T
    from tetris_mcts_amd.model_distributional import Model_Dist
    from tetris_mcts_amd.pyTetris import Tetris
    env_args = ((20, 10), 1, 0, 0)
    a = agents.DistValueSim(sims=8, env=Tetris, env_args=env_args, n_games=2, max_nodes=256, fit_backend="hip_dist")
    assert a.fit_backend == "hip_dist"
    with pytest.raises(ValueError, match="fit_backend"):
        agents.DistValueSim(sims=8, env=Tetris, env_args=env_args, n_games=2, max_nodes=256, fit_backend="hip")
    mdl = Model_Dist(atoms=50, seed=0, backend="torch")
    batch = [torch.from_numpy(d).cuda() for d in _fit_set(48)]
    with pytest.raises(ValueError, match="fused"):                       # a FusedAdam told not to fuse has no flat step
        T.HipDistFit(mdl.model, T.FusedAdam(mdl.model.parameters(), lr=1e-4, fused=False), batch, 16)
    with pytest.raises(ValueError, match="CUDA"):                        # the states in another precision
        T.HipDistFit(mdl.model, mdl._fused_optimizer(), [batch[0].double()] + batch[1:], 16)


def test_dist_online_training_round_with_the_hip_gradient_step():
    """one short DistValueSim run that reaches train_nodes(fit_backend="hip_dist", max_iters=8) on harvested tuples; the search then
    goes on with the refreshed operand streams"""
    from tetris_mcts_amd import agents, train as T
    from tetris_mcts_amd.model_distributional import Model_Dist
    from tetris_mcts_amd.pyTetris import Tetris
    G, sims = 16, 60
    env_args = ((20, 10), 1, 0, 0)
    game = Tetris(*env_args, seed=5, n_games=G)
    model = Model_Dist(atoms=50, seed=0, backend="hip")
    agent = agents.DistValueSim(sims=sims, env=Tetris, env_args=env_args, n_games=G, max_nodes=1500, model=model, online=True,
                                min_visits_to_store=4, memory_growth_rate=50, fit_backend="hip_dist")
    agent.update_root(game)
    before = model.flat_params().clone()
    for m in range(80):
        act = agent.play()
        game.play(act)
        agent.update_root(game)
        if game.end.any():
            game.reset("ended")
            agent.update_root(game)
        agent.train_if_collected(max_iters=8, iters_per_val=4, batch_size=64, log=False)
        if agent.n_trains >= 2:
            break
    assert agent.n_trains >= 2 and (agent.store.errors() == 0).all()
    assert isinstance(model.optimizer, T.FusedAdam) and model.optimizer._flat["t"] >= 8
    assert not torch.equal(before, model.flat_params())
    for _ in range(3):                                                  # the search continues on the new weights
        act = agent.play()
        game.play(act)
        agent.update_root(game)
    assert (agent.store.errors() == 0).all()
    d = model.inference_device(torch.zeros(4, 200, dtype=torch.int8, device="cuda"))[:, :50]
    assert torch.isfinite(d).all() and torch.allclose(d.sum(1), torch.ones(4, device="cuda"), atol=1e-5)
