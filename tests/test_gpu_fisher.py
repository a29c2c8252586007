"""Elastic weight consolidation on the GPU: the Fisher pass (csrc/valuenet_fit.hip: tm_valuenet_fit_fisher), the penalty
(csrc/yogi.hip: tm_ewc_penalty), the penalty inside a fit (train_data(ewc=)) and the route from recorded episodes to a checkpoint
that carries a Fisher (offline.fit_episodes(ewc_lambda=), train.py --ewc).

Accuracy of the Fisher is measure B of DESIGN.md section 6 (tests/fisher_cases.py): per parameter tensor
max|F_hip - F64| <= 8 max|F32 - F64| + 4 u max|F64| with per-sample CPU autograd in fp64 and fp32 as F64 and F32.  Every figure is
printed before it is asserted (pytest -s shows them)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fisher_cases as K
import fit_hip_cases as FC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.cases()
THREE_SLABS = "n 129, slab 64, weighted, repeats"


def _measure(name, case, got):
    f64, f32 = K.references(name, case)
    assert np.isfinite(got).all() and (got >= 0).all()
    bad = []
    for t, a, b32, b64 in zip(FC.TENSORS, FC.split(got), f32, f64):
        if not np.abs(b64).max() > 0:
            assert (a == 0).all(), (name, t, "F64 is identically zero: exact zeros")
            print("%-40s %-14s exactly zero" % (name, t))
            continue
        assert np.abs(b32 - b64).max() > 0, (name, t, "the rule's denominator")
        err, bound, need = FC.measure(a, b32, b64)
        print("%-40s %-14s err %.3e  bound %.3e  torch fp32 %.3e  needs M = %.2f" % (name, t, err, bound, np.abs(b32 - b64).max(), need))
        if not err <= bound:
            bad.append((t, err, bound, need))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", list(CASES))
def test_fisher_within_measure_b(name):
    _measure(name, CASES[name], K.hip_fisher(CASES[name]))


def test_dead_relu_gives_exact_zeros_upstream():
    case = K.dead_case()
    f64, _ = K.references("dead relu", case)
    zero = [t for t, b in zip(FC.TENSORS, f64) if not np.abs(b).max() > 0]
    assert {"conv1.weight", "conv2.weight", "conv3.weight", "fc1.weight"} <= set(zero), zero
    _measure("dead relu", case, K.hip_fisher(case))


def test_one_row_is_the_squared_gradient():
    """n = 1: F = g^2 with g tm_valuenet_fit_grad's batch-1 gradient of the same row.  Each route rounds at most three times
    (fl(fl(d^2) fl(a^2)) against fl(fl(d a)^2)): about 6 u, 8 u allowed; the absolute term covers squared operands flushed below
    the normal range."""
    case = CASES["n 1, weighted, idx"]
    g, _ = FC.hip_grad(case)
    f = K.hip_fisher(case).astype(np.float64)
    g2 = g.astype(np.float64) ** 2
    excess = np.abs(f - g2) - (2.0 ** -21 * g2 + 2.0 ** -100)
    rel = np.abs(f - g2)[g2 > 2.0 ** -80] / g2[g2 > 2.0 ** -80]
    print("n = 1: largest |F - g^2| / g^2 = %.3f u over %d elements" % (rel.max() * 2.0 ** 24, rel.size))
    assert (excess <= 0).all(), int((excess > 0).sum())
    assert g2.max() > 0


def test_a_slab_larger_than_n_changes_no_bit():
    case = CASES["n 33, weighted, idx NULL"]
    a, b = K.hip_fisher(case, slab=33), K.hip_fisher(case, slab=1024)
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all()


def test_same_bits_from_call_to_call_and_from_process_to_process_and_whatever_fisher_held():
    case = K.digest_case()
    a, b = K.hip_fisher(case), K.hip_fisher(case)
    assert a.tobytes() == b.tobytes()
    for fill in (123.0, -7.0):                                                  # fisher is overwritten, never read
        assert K.hip_fisher(case, fill=fill).tobytes() == a.tobytes()
    big = CASES[THREE_SLABS]
    c, d = K.hip_fisher(big, fill=1e30), K.hip_fisher(big, fill=-1.0)
    assert c.tobytes() == d.tobytes()
    mine = hashlib.sha256(a.tobytes()).hexdigest()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fisher_cases.py"), "digest"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)                                 # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    theirs = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
    assert theirs == [mine]


@pytest.mark.parametrize("name", ["n 5, weighted, repeats", THREE_SLABS])
def test_packed_rows_give_the_dense_bits(name):
    case = CASES[name]
    dense, packed = K.hip_fisher(case), K.hip_fisher(case, packed=True)
    assert dense.tobytes() == packed.tobytes() and dense.max() > 0


@pytest.mark.parametrize("name", ["n 1, weighted, idx", "n 257, unweighted, idx", THREE_SLABS])
def test_the_call_writes_only_where_it_says(name):
    """workspace (exactly tm_valuenet_fit_fisher_workspace(slab) floats) and fisher (478 338) carved out of one device tensor with
    64 KiB of guard before, between and after (FC.Arena): every guard byte and every input unchanged, the result the plain call's"""
    case = CASES[name]
    plain = K.hip_fisher(case)
    arena = FC.Arena()
    got = K.hip_fisher(case, place=arena)
    arena.check()
    assert got.tobytes() == plain.tobytes()


def test_refusals_launch_nothing():
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    case = CASES["n 3, unweighted, idx NULL"]
    inp = K.fisher_inputs(case)
    ws = torch.full((lib.tm_valuenet_fit_fisher_workspace(4) + 4,), 3.0, device="cuda")
    fisher = torch.full((K.N_LEARN,), 5.0, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(n=3, slab=4, w=ws, f=fisher, params=inp["params"], fn=lib.tm_valuenet_fit_fisher, states=inp["states"].data_ptr()):
        return fn(params.data_ptr() if params is not None else None, inp["bounds"].data_ptr(), states, inp["value"].data_ptr(),
                  inp["variance"].data_ptr(), inp["weight"].data_ptr(), None, n, slab, 0, K.CLIP, f.data_ptr() if f is not None else None,
                  w.data_ptr() if w is not None else None, s)
    assert call(n=0) == 1 and call(slab=0) == 1 and call(slab=(1 << 20) + 1) == 1 and call(w=ws[1:]) == 1 and call(f=None) == 1
    assert call(params=None) == 1 and call(w=None) == 1
    assert call(fn=lib.tm_valuenet_fit_fisher_packed, states=inp["states"].data_ptr() + 2) == 1
    g = torch.full((64,), 7.0, device="cuda")
    loss = torch.full((1,), 9.0, dtype=torch.float64, device="cuda")
    pw = torch.full((8,), 3.0, device="cuda")
    for lam in (-1.0, float("nan"), float("inf")):
        assert lib.tm_ewc_penalty(g.data_ptr(), g.data_ptr(), g.data_ptr(), 64, lam, g.data_ptr(), loss.data_ptr(), pw.data_ptr(), s) == 1
    assert lib.tm_ewc_penalty(g.data_ptr(), g.data_ptr(), g.data_ptr(), 0, 1.0, g.data_ptr(), loss.data_ptr(), pw.data_ptr(), s) == 1
    assert lib.tm_ewc_penalty(g.data_ptr(), g.data_ptr(), g.data_ptr(), 64, 1.0, g.data_ptr(), loss.data_ptr(), pw[1:].data_ptr(), s) == 1
    torch.cuda.synchronize()
    assert bool((ws == 3.0).all()) and bool((fisher == 5.0).all()) and bool((g == 7.0).all()) and float(loss) == 9.0 and bool((pw == 3.0).all())


# ---- tm_ewc_penalty ----
@pytest.mark.parametrize("n", [1, 255, 256, 257, K.N_LEARN])
def test_penalty_is_the_numpy_statement(n):
    p, anchor, fisher, grad = K.penalty_case(n, 40 + n % 7)
    lam = 0.37
    want, want_loss = K.penalty_numpy(p, anchor, fisher, grad, lam)
    got, loss = K.hip_penalty(p, anchor, fisher, grad, lam)
    assert got.tobytes() == want.tobytes()
    print("n %d: loss %.17g, numpy %.17g" % (n, loss, want_loss))
    assert abs(loss - want_loss) <= 1e-12 * abs(want_loss) and want_loss > 0
    again, loss2 = K.hip_penalty(p, anchor, fisher, grad, lam)
    assert again.tobytes() == got.tobytes() and loss2 == loss
    # guard bands around grad, loss and the workspace
    arena = FC.Arena()
    g3, loss3 = K.hip_penalty(p, anchor, fisher, grad, lam, place=arena)
    arena.check()
    assert g3.tobytes() == got.tobytes() and loss3 == loss


def test_no_penalty_leaves_the_gradient_equal_by_value():
    for kw in (dict(zero_fisher=True), dict(at_anchor=True)):
        p, anchor, fisher, grad = K.penalty_case(1000, 9, **kw)
        got, loss = K.hip_penalty(p, anchor, fisher, grad, 2.0)
        assert (got == grad).all() and loss == 0.0          # (by value: -0 + 0 is +0)


# ---- inside a fit ----
def _fit_data(n=600, seed=3):
    s, value, variance, weight = FC.dataset(n, seed)
    dev = torch.device("cuda")
    return [torch.from_numpy(s.reshape(n, 1, 20, 10).astype(np.float32)).to(dev)] + \
           [torch.from_numpy(a.reshape(n, 1)).to(dev) for a in (value, variance, weight)]


def _ewc_for(mdl, lam, seed=8):
    g = torch.Generator().manual_seed(seed)
    fisher = (torch.rand(K.N_LEARN, generator=g) ** 4 * 50).cuda()
    anchor = (mdl._flat_learnable().cpu() + 0.02 * torch.randn(K.N_LEARN, generator=g)).cuda()
    return dict(fisher=fisher, anchor=anchor, lam=lam)


def test_penalty_inside_a_fit_adds_the_numpy_statement(tmp_path, monkeypatch):
    from tetris_mcts_amd import train as T
    from tetris_mcts_amd.model import Model_VV
    monkeypatch.chdir(tmp_path)
    mdl = Model_VV(backend="torch", seed=0)
    data = _fit_data()
    with torch.no_grad():
        mdl.model.out_ubound.copy_(torch.stack([data[1].max(), data[2].max()]))
    ewc = _ewc_for(mdl, 0.6)
    hip = T.HipFit(mdl.model, mdl._optimizer(), data, 64, ewc=ewc)
    idx = torch.randint(0, 600, (64,), device="cuda")
    hip.grad(idx, True)
    torch.cuda.synchronize()
    before = hip.F["g"].cpu().numpy().copy()
    pen = hip.penalty()
    torch.cuda.synchronize()
    want, want_loss = K.penalty_numpy(hip.F["p"].cpu().numpy(), ewc["anchor"].cpu().numpy(), ewc["fisher"].cpu().numpy(), before, 0.6)
    assert hip.F["g"].cpu().numpy().tobytes() == want.tobytes() and np.abs(before).max() > 0
    assert abs(float(pen) - want_loss) <= 1e-12 * want_loss and want_loss > 0


def _fit(monkeypatch, graph, ewc_lam, iters=12):
    from tetris_mcts_amd.model import Model_VV
    monkeypatch.setenv("TM_TRAIN_GRAPH", graph)
    torch.manual_seed(5)
    mdl = Model_VV(backend="torch", seed=0)
    ewc = None if ewc_lam is None else _ewc_for(mdl, ewc_lam)
    torch.manual_seed(11)
    res = mdl.train_data(_fit_data(), fit_backend="hip", batch_size=64, max_iters=iters, iters_per_val=6, validation_fraction=0.0,
                         early_stopping=False, log=False, **({} if ewc is None else dict(ewc=ewc)))
    torch.cuda.synchronize()
    return res, mdl._flat_learnable().cpu().numpy()


def test_a_fit_with_the_penalty_replays_and_equals_the_eager_fit(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    r1, replayed = _fit(monkeypatch, "1", 0.6)
    r0, eager = _fit(monkeypatch, "0", 0.6)
    assert r1["graph_replay"] is True and r0["graph_replay"] is False and r1["iters"] == r0["iters"] == 12
    assert replayed.tobytes() == eager.tobytes() and np.isfinite(eager).all()
    # lam = 0: the fit without ewc, by value; lam > 0: another fit
    _, plain = _fit(monkeypatch, "1", None)
    _, zero = _fit(monkeypatch, "1", 0.0)
    assert np.array_equal(plain, zero)
    assert not np.array_equal(plain, replayed)


# ---- the route ----
def test_record_fit_fisher_checkpoint_and_command_line(tmp_path, monkeypatch):
    from test_gpu_offline import _record
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model import Model_VV, PARAM_ORDER
    stem = _record(str(tmp_path / "self1"))
    monkeypatch.chdir(tmp_path)
    path = os.path.join(str(tmp_path), "pytorch_model", "model_checkpoint")
    model = Model_VV(backend="hip", seed=0)
    # a model that never computed a Fisher saves exactly the two keys it always saved
    model.save(verbose=False)
    assert sorted(torch.load(path, map_location="cpu")) == ["model_state_dict", "optimizer_state_dict"]
    kw = dict(td=True, lam=0.9, fit_backend="hip", validation_backend="hip", max_iters=20, batch_size=64, validation=True,
              val_mode=1, val_episodes=5)
    res = O.fit_episodes(model, [stem], ewc_lambda=1.0, **kw)
    _, info = O.training_set([stem], td=True, lam=0.9, validation=True, val_mode=1, val_episodes=5, device="cpu")
    assert info["n_val"] > 0 and res["ewc"] == dict(penalised=False, fisher_rows=info["n_train"])
    assert model.fisher is not None and model.fisher.shape == (K.N_LEARN,) and model.fisher.is_cuda
    assert bool(torch.isfinite(model.fisher).all()) and bool((model.fisher >= 0).all()) and float(model.fisher.max()) > 0
    assert torch.equal(model.ewc_anchor, model._flat_learnable()) and model.ewc_anchor.data_ptr() != model._flat_learnable().data_ptr()
    ck = torch.load(path, map_location="cpu")
    sd = model.model.state_dict()
    for key in ("fisher", "ewc_anchor"):
        assert list(ck[key]) == PARAM_ORDER[:10] and all(ck[key][k].shape == sd[k].shape for k in PARAM_ORDER[:10])
    fresh = Model_VV(backend="hip", seed=1)
    fresh.load(verbose=False)
    assert torch.equal(fresh.fisher, model.fisher) and torch.equal(fresh.ewc_anchor, model.ewc_anchor)
    first = model.fisher.clone()
    res2 = O.fit_episodes(fresh, [stem], ewc_lambda=1.0, **kw)
    assert res2["ewc"]["penalised"] is True and res2["rounds"][0]["graph_replay"] is True
    assert not torch.equal(fresh.fisher, first), "the new Fisher replaces the old"
    # the command line on the same directory, in a fresh process
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--data_paths", str(tmp_path / "self1" / "data*"), "--td",
                        "--td_lambda", "0.9", "--validation", "--val_mode", "1", "--val_episodes", "5", "--max_iters", "20",
                        "--batch_size", "64", "--ewc", "--ewc_lambda", "1"],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Loading model..." in r.stdout and "Saving model..." in r.stdout and "EWC penalty" in r.stderr
    again = Model_VV(backend="hip", seed=2)
    again.load(verbose=False)
    assert again.fisher is not None and not torch.equal(again.fisher, fresh.fisher)
