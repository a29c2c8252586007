"""The HIP gradient step of the fit on the GPU (csrc/valuenet_fit.hip, train_data(fit_backend="hip")).

Accuracy is measure B of DESIGN.md section 6 applied to gradients (tests/fit_hip_cases.py): per parameter tensor, and for the loss
mean and std,  max|g_hip - g64| <= 8 max|g_torch_fp32 - g64| + 4 u max|g64|  with torch's CPU autograd of model.Net +
train.batch_loss in fp64 and fp32 as g64 and g_torch_fp32.  Every figure is printed before it is asserted (pytest -s shows them)."""
import hashlib
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import fit_hip_cases as FC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = FC.cases()
# the kernels' blocking constants along the batch (csrc/valuenet_fit.hip) and the batches past them: a split of fc1's weight
# gradient with one sample, and s1 = 5 splits for the 4 groups of k_fit_reduce<4> (with 33 > 16 partials of the FC bias sums)
assert (FC.FC_KC, FC.HEAD_CHUNK, FC.SPW, FC.RED_G_FC, FC.RED_G) == (256, 32, 4, 4, 16) and FC.LARGE_BATCHES == (257, 1025)
assert -(-1025 // FC.FC_KC) == 5 > FC.RED_G_FC and -(-1025 // FC.HEAD_CHUNK) == 33 > FC.RED_G and -(-1025 // FC.SPW) == 257
assert list(CASES)[-4:] == ["fresh net, batch 257", "fresh net, batch 1025", "fresh net, batch 1025, unweighted, idx NULL",
                            "value_net_online_r06.pt, weighted, batch 1025"]          # after every earlier case


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_and_loss_within_measure_b(name):
    case = CASES[name]
    torch.set_num_threads(16)
    g64, l64 = FC.reference(case, torch.float64)
    g32, l32 = FC.reference(case, torch.float32)
    got, loss = FC.hip_grad(case)
    assert np.isfinite(got).all() and np.isfinite(loss).all()
    bad = []
    for t, a, b32, b64 in zip(FC.TENSORS, FC.split(got), g32, g64):
        assert np.abs(b64).max() > 0 and np.abs(b32 - b64).max() > 0, (name, t, "the rule's denominator")
        err, bound, need = FC.measure(a, b32, b64)
        print("%-40s %-14s err %.3e  bound %.3e  torch fp32 %.3e  needs M = %.2f" % (name, t, err, bound, np.abs(b32 - b64).max(), need))
        if not err <= bound:
            bad.append((t, err, bound, need))
    for k, what in enumerate(("loss mean", "loss std")):
        if case["batch"] == 1 and k == 1:
            assert loss[1] == 0.0          # one sample: the population std is 0
            continue
        err, bound, need = FC.measure([loss[k]], [l32[k]], [l64[k]])
        print("%-40s %-14s err %.3e  bound %.3e  needs M = %.2f" % (name, what, err, bound, need))
        if not err <= bound:
            bad.append((what, err, bound, need))
    assert not bad, (name, bad)


def test_dead_relu_gives_exact_zeros_upstream():
    case = FC.dead_relu_case()
    g64, _ = FC.reference(case, torch.float64)
    g32, _ = FC.reference(case, torch.float32)
    got, loss = FC.hip_grad(case)
    for t, a, b32, b64 in zip(FC.TENSORS, FC.split(got), g32, g64):
        if np.abs(b64).max() == 0:
            assert t in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias", "fc1.weight")
            assert (a == 0).all(), (t, np.abs(a).max())
        else:
            err, bound, need = FC.measure(a, b32, b64)
            print("dead ReLU %-14s err %.3e bound %.3e needs M = %.2f" % (t, err, bound, need))
            assert err <= bound, (t, err, bound)
    assert np.isfinite(loss).all()


def test_gradient_is_overwritten_not_accumulated():
    case = FC.digest_case()
    a, _ = FC.hip_grad(case, grad_fill=123.0)
    b, _ = FC.hip_grad(case, grad_fill=-7.0)
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all()


def test_same_bits_from_call_to_call_and_from_process_to_process():
    case = FC.digest_case()
    g1, l1 = FC.hip_grad(case)
    g2, l2 = FC.hip_grad(case)
    assert g1.tobytes() == g2.tobytes() and l1.tobytes() == l2.tobytes()
    for big in ("fresh net, batch 1024", "fresh net, batch 1025"):          # 1 025: groups of the second stages with two terms
        b1, b2 = FC.hip_grad(CASES[big]), FC.hip_grad(CASES[big])
        assert b1[0].tobytes() == b2[0].tobytes() and b1[1].tobytes() == b2[1].tobytes(), big
    mine = hashlib.sha256(g1.tobytes() + l1.tobytes()).hexdigest()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fit_hip_cases.py"), "digest"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)                                 # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    theirs = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
    assert theirs == [mine]


@pytest.mark.parametrize("name", ["fresh net, batch 1", "fresh net, batch 33", "fresh net, batch 257", "fresh net, batch 1025"])
def test_the_call_writes_only_where_it_says(name):
    """workspace (exactly tm_valuenet_fit_workspace(batch) floats), grad (478 338) and loss (2) carved out of one device tensor,
    each on a 16-byte boundary with 64 KiB of guard before, between and after (FC.Arena): after the call every guard byte holds
    its pattern, every input (params, bounds, states, value, variance, weight, idx) is bit-identical to its copy from before the
    call, and grad and loss are bit for bit what the call gives with buffers of the allocator's choosing.  Reads past an input
    cannot be seen this way."""
    case = CASES[name]
    arena = FC.Arena()
    got, loss = FC.hip_grad(case, place=arena)
    arena.check()
    assert set(arena.inputs) == {"params", "bounds", "states", "value", "variance", "weight", "idx"}
    print("%-28s arena of %d floats, segments (offset, floats) %s" % (name, arena.arena.numel(), arena.segments))
    plain, plain_loss = FC.hip_grad(case)
    assert np.isfinite(got).all() and got.tobytes() == plain.tobytes() and loss.tobytes() == plain_loss.tobytes()


def test_refused_arguments_launch_nothing():
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda")
    B = 8
    P = torch.zeros(FC.N_LEARN, device=dev)
    bounds = torch.tensor([100.0, 1000.0, 0.0, 0.1], device=dev)
    s8 = torch.zeros(B, 200, dtype=torch.int8, device=dev)
    v = torch.ones(B, device=dev)
    grad = torch.full((FC.N_LEARN,), 5.0, device=dev)
    loss = torch.full((2,), 5.0, device=dev)
    ws = torch.zeros(lib.tm_valuenet_fit_workspace(B), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    full = [P.data_ptr(), bounds.data_ptr(), s8.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), None, B, 1, 0.1, grad.data_ptr(),
            loss.data_ptr(), ws.data_ptr(), st]
    for k in (0, 1, 2, 3, 4, 5, 10, 11, 12):
        args = list(full)
        args[k] = None
        assert lib.tm_valuenet_fit_grad(*args) == 1, k          # hipErrorInvalidValue
    for b in (0, -1):
        args = list(full)
        args[7] = b
        assert lib.tm_valuenet_fit_grad(*args) == 1, b
    torch.cuda.synchronize()
    assert bool((grad == 5.0).all()) and bool((loss == 5.0).all())
    assert lib.tm_valuenet_fit_grad(*full) == 0                 # ... and the same arguments complete are accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()) and not bool((grad == 5.0).any())


def test_four_reference_steps_with_the_hip_gradient():
    """the four training steps of tests/golden/ref_training.npz, the gradient from tm_valuenet_fit_grad: the three assertions and
    the tolerances of test_gpu_train_dist.test_training_steps_on_the_gpu_match_the_reference_within_tolerance"""
    from tetris_mcts_amd import model as M
    from tetris_mcts_amd import train as T
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_training.npz"))
    dev = torch.device("cuda")
    mdl = M.Model_VV(backend="torch", seed=0)
    mdl.set_flat_params(g["tr_params0"])
    mdl.model.train()
    opt = mdl._optimizer()
    batch = [torch.from_numpy(g[k].copy()).to(dev) for k in ("tr_states", "tr_values", "tr_variances", "tr_weights")]
    n = batch[0].shape[0]
    fit = T.HipFit(mdl.model, opt, batch, n)
    idx = torch.arange(n, device=dev)
    for i in range(4):
        loss = fit.grad(idx, True)
        gn = math.sqrt(sum(float(p.grad.norm(2)) ** 2 for p in mdl.model.parameters() if p.grad is not None))
        opt.step()
        print("step", i, float(loss), g["tr_losses"][i], gn, g["tr_gnorms"][i])
        assert abs(float(loss.detach()) - g["tr_losses"][i]) <= 1e-4 * abs(g["tr_losses"][i]), (i, float(loss.detach()), g["tr_losses"][i])
        assert abs(gn - g["tr_gnorms"][i]) <= 1e-4 * gn, (i, gn, g["tr_gnorms"][i])
    mdl._flat = None
    got = mdl.flat_params().cpu().numpy().astype(np.float64)
    moved = np.abs(g["tr_params4"].astype(np.float64) - g["tr_params0"].astype(np.float64))
    diff = np.abs(got - g["tr_params4"].astype(np.float64))
    print("diff max", diff.max(), "mean", np.mean(diff), "moved mean", np.mean(moved))
    assert moved.max() > 1e-3 and diff.max() <= 8e-3 and float(np.mean(diff)) <= 2e-2 * float(np.mean(moved)), (diff.max(), moved.max(), np.mean(diff), np.mean(moved))


def _fit_set(n=6000):
    rng = np.random.default_rng(0)
    states = rng.integers(-1, 2, size=(n, 1, 20, 10)).astype(np.float32)
    values = (states.sum(axis=(1, 2, 3)) * 0.5 + 20).astype(np.float32)[:, None]
    variances = np.full((n, 1), 4.0, np.float32)
    weights = rng.integers(1, 20, size=(n, 1)).astype(np.float32)
    return states, values, variances, weights


def test_eager_hip_and_torch_fits_draw_the_same_batches_and_agree(monkeypatch):
    """TM_TRAIN_GRAPH=0, the same seed: 20 iterations of either backend draw the same indices and end on parameters that differ by
    no more than 2 % of the mean distance moved (the form of the four-steps test)"""
    from tetris_mcts_amd import model as M
    monkeypatch.setenv("TM_TRAIN_GRAPH", "0")
    data = _fit_set(3000)
    real_randint = torch.randint
    out = {}
    for backend in ("torch", "hip"):
        draws = []

        def recording(*a, **k):
            r = real_randint(*a, **k)
            draws.append(r.detach().cpu().numpy().copy())
            return r
        torch.manual_seed(5)
        mdl = M.Model_VV(backend="torch", seed=0)
        start = mdl.flat_params().cpu().numpy().astype(np.float64)
        monkeypatch.setattr(torch, "randint", recording)
        res = mdl.train_data(list(data), iters_per_val=1000, batch_size=256, max_iters=20, log=False, fit_backend=backend)
        monkeypatch.setattr(torch, "randint", real_randint)
        assert res["iters"] == 20 and res["graph_replay"] is False
        out[backend] = (draws, mdl.flat_params().cpu().numpy().astype(np.float64), start)
    d_t, d_h = out["torch"][0], out["hip"][0]
    assert len(d_t) == len(d_h) == 20 and all(a.shape == (256,) and (a == b).all() for a, b in zip(d_t, d_h))
    moved = np.abs(out["torch"][1] - out["torch"][2])
    diff = np.abs(out["hip"][1] - out["torch"][1])
    print("eager fits: diff max %.3e mean %.3e, moved max %.3e mean %.3e" % (diff.max(), diff.mean(), moved.max(), moved.mean()))
    assert moved.max() > 1e-3 and diff.max() <= 8e-3 and float(np.mean(diff)) <= 2e-2 * float(np.mean(moved))


def test_the_hip_fit_replayed_from_a_hip_graph(monkeypatch):
    """test_gpu_train_dist.test_the_fit_replayed_from_a_hip_graph with fit_backend="hip": the same thresholds"""
    from tetris_mcts_amd import model as M
    res = {}
    states, values, variances, weights = _fit_set(6000)
    for mode in ("1", "0"):
        monkeypatch.setenv("TM_TRAIN_GRAPH", mode)
        torch.manual_seed(5)
        mdl = M.Model_VV(backend="torch", seed=0)
        with torch.no_grad():
            before = float(((mdl.model(torch.from_numpy(states[:512]).cuda())[:, 0:1].cpu() - torch.from_numpy(values[:512])) ** 2).mean())
        r = mdl.train_data([states, values, variances, weights], iters_per_val=50, batch_size=256, max_iters=300, log=False,
                           fit_backend="hip")
        with torch.no_grad():
            after = float(((mdl.model(torch.from_numpy(states[:512]).cuda())[:, 0:1].cpu() - torch.from_numpy(values[:512])) ** 2).mean())
        res[mode] = (r, before, after)
        print("graph", mode, r, before, after)
        assert r["iters"] == 300 or r["iters"] % 50 == 0
        assert after < 0.5 * before, (mode, before, after)
    assert res["1"][0]["graph_replay"] is True and res["0"][0]["graph_replay"] is False
    assert abs(res["1"][0]["best_validation"] - res["0"][0]["best_validation"]) < 0.35 * abs(res["0"][0]["best_validation"]) + 0.05


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
    os.chdir(tempfile.mkdtemp())                      # (rank 0's train_data writes ./pytorch_model/model_checkpoint)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tetris_mcts_amd import model as M
    mdl = M.Model_VV(backend="torch", seed=0)
    start = mdl.flat_params().cpu().numpy().copy()
    gen = torch.Generator(device="cuda").manual_seed(99)
    res = mdl.train_data(list(_fit_set(2000)), batch_size=256, iters_per_val=4, max_iters=8, generator=gen, log=False, fit_backend="hip")
    q.put((rank, res["iters"], start, mdl.flat_params().cpu().numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_leave_bit_identical_weights():
    """two gloo ranks on the one GPU (two processes, as tests/test_gpu_two_ranks.py): a data-parallel hip fit, 128 rows a rank"""
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
    from tetris_mcts_amd import model as M
    from tetris_mcts_amd import train as T
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_training.npz"))
    dev = torch.device("cuda")
    mdl = M.Model_VV(backend="torch", seed=0)
    batch = [torch.from_numpy(g[k].copy()).to(dev) for k in ("tr_states", "tr_values", "tr_variances", "tr_weights")]
    n = batch[0].shape[0]
    fit = T.HipFit(mdl.model, mdl._optimizer(), batch, n)
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

