"""Elastic weight consolidation for the distributional head on the GPU: the Fisher pass (csrc/distnet_fit.hip:
tm_distnet_fit_fisher), the penalty inside a hip_dist fit (train_data(ewc_dist=)) and the routes from recorded episodes and from
dist node shards to a checkpoint that carries a Fisher (offline.fit_episodes_dist / fit_dist_nodes(ewc_lambda=), train.py
--ewc_dist).

Accuracy of the Fisher is measure B of DESIGN.md section 6 (tests/dist_fisher_cases.py): per parameter tensor
max|F_hip - F64| <= 8 max|F32 - F64| + 4 u max|F64| with per-row CPU autograd in fp64 and fp32 as F64 and F32.  Every figure is
printed before it is asserted (pytest -s shows them)."""
import hashlib
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dist_fisher_cases as K
import dist_fit_cases as DC
import fisher_cases as VK          # penalty_numpy: the float32 statement of tm_ewc_penalty
import fit_hip_cases as FC         # Arena

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(name):
    return K.cases()[name]


def _measure(name, case, got):
    f64, f32 = K.references(name, case)
    assert got.shape == (DC.n_params(case["atoms"]),) and np.isfinite(got).all() and (got >= 0).all()
    bad = []
    for t, a, b32, b64 in zip(K.TENSORS, DC.split(got, case["atoms"]), f32, f64):
        if not np.abs(b64).max() > 0:
            assert (a == 0).all(), (name, t, "F64 is identically zero: exact zeros")
            print("%-46s %-14s exactly zero" % (name, t))
            continue
        assert np.abs(b32 - b64).max() > 0, (name, t, "the rule's denominator")
        err, bound, need = K.measure(a, b32, b64)
        print("%-46s %-14s err %.3e  bound %.3e  torch fp32 %.3e  needs M = %.2f" % (name, t, err, bound, np.abs(b32 - b64).max(), need))
        if not err <= bound:
            bad.append((t, err, bound, need))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", K.case_names())
def test_fisher_within_measure_b(name):
    _measure(name, _case(name), K.hip_fisher(_case(name)))


def test_one_atom_gives_exact_zeros_everywhere():
    case = _case(K.ZERO_CASE)
    got = K.hip_fisher(case)
    assert got.shape == (DC.n_params(1),) and (got == 0).all()


def test_one_row_is_the_squared_gradient():
    """n = 1: F = g^2 with g tm_distnet_fit_grad's batch-1 gradient of the same row (the divisor is 1 either way).  Each route rounds
    at most three times (fl(fl(d^2) fl(a^2)) against fl(fl(d a)^2)): about 6 u, 8 u allowed; the absolute term covers squared
    operands flushed below the normal range."""
    case = _case(K.ONE_ROW)
    g, _ = DC.hip_grad(case)
    f = K.hip_fisher(case).astype(np.float64)
    g2 = g.astype(np.float64) ** 2
    excess = np.abs(f - g2) - (2.0 ** -21 * g2 + 2.0 ** -100)
    rel = np.abs(f - g2)[g2 > 2.0 ** -80] / g2[g2 > 2.0 ** -80]
    print("n = 1: largest |F - g^2| / g^2 = %.3f u over %d elements" % (rel.max() * 2.0 ** 24, rel.size))
    assert (excess <= 0).all(), int((excess > 0).sum())
    assert g2.max() > 0


def test_a_slab_larger_than_n_changes_no_bit():
    case = _case(K.N33)
    a, b = K.hip_fisher(case, slab=33), K.hip_fisher(case, slab=1024)
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all() and a.max() > 0


def test_same_bits_from_call_to_call_and_from_process_to_process_and_whatever_fisher_held():
    case = K.digest_case()
    a, b = K.hip_fisher(case), K.hip_fisher(case)
    assert a.tobytes() == b.tobytes()
    for fill in (123.0, -7.0):                                                  # fisher is overwritten, never read
        assert K.hip_fisher(case, fill=fill).tobytes() == a.tobytes()
    big = _case(K.THREE_SLABS)
    c, d = K.hip_fisher(big, fill=1e30), K.hip_fisher(big, fill=-1.0)
    assert c.tobytes() == d.tobytes()
    mine = hashlib.sha256(a.tobytes()).hexdigest()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dist_fisher_cases.py"), "digest"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)                                 # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    theirs = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
    assert theirs == [mine]


@pytest.mark.parametrize("name", ["fixture, n 5, weighted, repeats", K.THREE_SLABS])
def test_packed_rows_give_the_dense_bits(name):
    case = _case(name)
    dense, packed = K.hip_fisher(case), K.hip_fisher(case, packed=True)
    assert dense.tobytes() == packed.tobytes() and dense.max() > 0


@pytest.mark.parametrize("name", [K.ONE_ROW, K.N257, K.THREE_SLABS])
def test_the_call_writes_only_where_it_says(name):
    """workspace (exactly tm_distnet_fit_fisher_workspace(slab, atoms) floats) and fisher carved out of one device tensor with
    64 KiB of guard before, between and after (FC.Arena): every guard byte and every input unchanged, the result the plain call's"""
    case = _case(name)
    plain = K.hip_fisher(case)
    arena = FC.Arena()
    got = K.hip_fisher(case, place=arena)
    arena.check()
    assert got.tobytes() == plain.tobytes()


def test_refusals_launch_nothing():
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    case = _case("fixture, n 3, unweighted, idx NULL")
    inp = K.fisher_inputs(case)
    ws = torch.full((lib.tm_distnet_fit_fisher_workspace(4, 50) + 4,), 3.0, device="cuda")
    fisher = torch.full((DC.n_params(50),), 5.0, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(n=3, slab=4, atoms=50, stride=50, w=ws, f=fisher, params=inp["params"].data_ptr(), fn=lib.tm_distnet_fit_fisher,
             states=inp["states"].data_ptr(), target=inp["targets"].data_ptr(), weight=inp["weight"].data_ptr()):
        return fn(params, states, target, stride, weight, None, n, slab, atoms, 0, f.data_ptr() if f is not None else None,
                  w.data_ptr() if w is not None else None, s)
    assert call(n=0) == 1 and call(slab=0) == 1 and call(slab=(1 << 20) + 1) == 1 and call(w=ws[1:]) == 1 and call(f=None) == 1
    assert call(params=None) == 1 and call(w=None) == 1 and call(states=None) == 1 and call(target=None) == 1 and call(weight=None) == 1
    assert call(atoms=0) == 1 and call(atoms=65, stride=65) == 1 and call(stride=49) == 1
    assert call(params=inp["params"].data_ptr() + 4) == 1
    assert call(fn=lib.tm_distnet_fit_fisher_packed, states=inp["states"].data_ptr() + 2) == 1
    torch.cuda.synchronize()
    assert bool((ws == 3.0).all()) and bool((fisher == 5.0).all())


# ---- inside a fit ----
N_FLAT = DC.n_params(50)


def _fit_data(n=600, seed=3):
    s, t, w = DC.dataset(n, 50, seed)
    states = torch.zeros(n, 1, 22, 10)
    states[:, 0, 2:] = torch.from_numpy(s.reshape(n, 20, 10).astype(np.float32))
    return [states.cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(w).reshape(n, 1).cuda()]


def _ewc_for(mdl, lam, seed=8):
    g = torch.Generator().manual_seed(seed)
    fisher = (torch.rand(N_FLAT, generator=g) ** 4 * 50).cuda()
    anchor = (mdl.flat_params().cpu() + 0.02 * torch.randn(N_FLAT, generator=g)).cuda()
    return dict(fisher=fisher, anchor=anchor, lam=lam)


def test_penalty_inside_a_fit_adds_the_numpy_statement():
    from tetris_mcts_amd import train as T
    from tetris_mcts_amd.model_distributional import Model_Dist
    mdl = Model_Dist(atoms=50, seed=0, backend="hip")
    data = _fit_data()
    ewc = _ewc_for(mdl, 0.6)
    hip = T.HipDistFit(mdl.model, mdl._fused_optimizer(), data, 64, ewc=ewc)
    assert hip.F["n"] == N_FLAT
    idx = torch.randint(0, 600, (64,), device="cuda")
    hip.grad(idx, True)
    torch.cuda.synchronize()
    before = hip.F["g"].cpu().numpy().copy()
    pen = hip.penalty()
    torch.cuda.synchronize()
    want, want_loss = VK.penalty_numpy(hip.F["p"].cpu().numpy(), ewc["anchor"].cpu().numpy(), ewc["fisher"].cpu().numpy(), before, 0.6)
    assert hip.F["g"].cpu().numpy().tobytes() == want.tobytes() and np.abs(before).max() > 0
    assert not np.array_equal(want, before)
    assert abs(float(pen) - want_loss) <= 1e-12 * want_loss and want_loss > 0
    # the value net's dict is not this fit's: refused by the same check as in train_data
    with pytest.raises(ValueError, match="fisher"):
        T.HipDistFit(mdl.model, mdl._fused_optimizer(), data, 64, ewc=dict(fisher=ewc["fisher"][:-1], anchor=ewc["anchor"], lam=1.0))


def _fit(monkeypatch, graph, ewc_lam, iters=12):
    from tetris_mcts_amd.model_distributional import Model_Dist
    monkeypatch.setenv("TM_TRAIN_GRAPH", graph)
    torch.manual_seed(5)
    mdl = Model_Dist(atoms=50, seed=0, backend="hip")
    ewc = None if ewc_lam is None else _ewc_for(mdl, ewc_lam)
    torch.manual_seed(11)
    res = mdl.train_data(_fit_data(), fit_backend="hip_dist", batch_size=64, max_iters=iters, iters_per_val=6, validation_fraction=0.0,
                         early_stopping=False, log=False, **({} if ewc is None else dict(ewc_dist=ewc)))
    torch.cuda.synchronize()
    return res, mdl.flat_params().cpu().numpy()


def test_a_fit_with_the_penalty_replays_and_equals_the_eager_fit(monkeypatch):
    r1, replayed = _fit(monkeypatch, "1", 0.6)
    r0, eager = _fit(monkeypatch, "0", 0.6)
    assert r1["graph_replay"] is True and r0["graph_replay"] is False and r1["iters"] == r0["iters"] == 12
    assert replayed.tobytes() == eager.tobytes() and np.isfinite(eager).all()
    # lam = 0: the fit without ewc_dist, by value; lam > 0: another fit
    _, plain = _fit(monkeypatch, "1", None)
    _, zero = _fit(monkeypatch, "1", 0.0)
    assert np.array_equal(plain, zero)
    assert not np.array_equal(plain, replayed)


# ---- the routes ----
def _cli():
    spec = importlib.util.spec_from_file_location("tm_train_cli_gpu_ewc_dist", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _spy_fisher(model, monkeypatch):
    seen, inner = [], model.compute_fisher

    def spy(data, **kw):
        seen.append(([d.clone() for d in data], kw))
        return inner(data, **kw)
    monkeypatch.setattr(model, "compute_fisher", spy)
    return seen


def _carries_a_fisher(model, path):
    from tetris_mcts_amd.model_distributional import PARAM_ORDER
    assert model.fisher is not None and model.fisher.shape == (N_FLAT,) and model.fisher.is_cuda
    assert bool(torch.isfinite(model.fisher).all()) and bool((model.fisher >= 0).all()) and float(model.fisher.max()) > 0
    assert torch.equal(model.ewc_anchor, model.flat_params()) and model.ewc_anchor.data_ptr() != model.flat_params().data_ptr()
    ck = torch.load(path, map_location="cpu")
    assert sorted(ck) == ["ewc_anchor", "fisher", "model_state_dict", "optimizer_state_dict"]
    sd = model.model.state_dict()
    for key in ("fisher", "ewc_anchor"):
        assert list(ck[key]) == PARAM_ORDER and all(ck[key][k].shape == sd[k].shape for k in PARAM_ORDER)


def test_record_fit_fisher_checkpoint_and_command_line(tmp_path, monkeypatch):
    from test_gpu_offline import _record
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model_distributional import Model_Dist
    stem = _record(str(tmp_path / "self1"))
    monkeypatch.chdir(tmp_path)
    path = os.path.join(str(tmp_path), "pytorch_model", "model_checkpoint_dist")
    model = Model_Dist(atoms=50, backend="hip", seed=0)
    # a model that never computed a Fisher saves exactly the two keys it always saved
    model.save(verbose=False)
    assert sorted(torch.load(path, map_location="cpu")) == ["model_state_dict", "optimizer_state_dict"]
    kw = dict(max_iters=20, batch_size=64, validation_backend="hip", validation=True, val_mode=1, val_episodes=3, weighted=True)
    handed, inner = [], model.train_data

    def spy(data, **k):
        handed.append(([d.clone() for d in data], k))
        return inner(data, **k)
    monkeypatch.setattr(model, "train_data", spy)
    seen = _spy_fisher(model, monkeypatch)
    res = O.fit_episodes_dist(model, [stem], ewc_lambda=1.0, **kw)
    (data, tk), (fdata, fk) = handed[0], seen[0]
    n = data[0].shape[0]
    n_train = n - int(n * tk["validation_fraction"])
    assert 0 < n_train < n and tk["ewc_lambda"] == 1.0 and res["ewc"] == dict(penalised=False, fisher_rows=n_train)
    # the Fisher's rows: the training rows, that round's targets, the weights as the fit used them
    assert fk == dict(weighted=True) and [d.shape[0] for d in fdata] == [n_train] * 3
    assert torch.equal(fdata[0], data[0][:n_train]) and torch.equal(fdata[1], data[1][:n_train])
    assert torch.equal(fdata[2], (data[2] / data[2].mean())[:n_train])
    print("weights handed to the fit: mean %.4g, std %.4g" % (float(data[2].mean()), float(data[2].std())))
    _carries_a_fisher(model, path)
    fresh = Model_Dist(atoms=50, backend="hip", seed=1)
    fresh.load(verbose=False)
    assert torch.equal(fresh.fisher, model.fisher) and torch.equal(fresh.ewc_anchor, model.ewc_anchor)
    first = model.fisher.clone()
    res2 = O.fit_episodes_dist(fresh, [stem], ewc_lambda=1.0, **kw)
    assert res2["ewc"] == dict(penalised=True, fisher_rows=n_train) and res2["rounds"][0]["graph_replay"] is True
    assert not torch.equal(fresh.fisher, first), "the new Fisher replaces the old"
    _carries_a_fisher(fresh, path)
    # the command line on the same directory, in a fresh process
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--head", "dist", "--data_paths", str(tmp_path / "self1" / "data*"),
                        "--validation", "--val_mode", "1", "--val_episodes", "3", "--max_iters", "20", "--batch_size", "64",
                        "--ewc_dist", "--ewc_lambda", "1"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Loading model..." in r.stdout and "Saving model..." in r.stdout and "EWC penalty" in r.stderr
    again = Model_Dist(atoms=50, backend="hip", seed=2)
    again.load(verbose=False)
    assert again.fisher is not None and not torch.equal(again.fisher, fresh.fisher)


def test_dist_node_shards_fit_fisher_checkpoint_and_command_line(tmp_path, monkeypatch):
    """the same through fit_dist_nodes: packed observations, the recorded distributions, the visits as weights"""
    import dist_node_cases as NK
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model_distributional import Model_Dist
    from tetris_mcts_amd.nodes import DistNodeShardWriter
    monkeypatch.chdir(tmp_path)
    rows = NK.synthetic_rows(400, 9, 50)
    DistNodeShardWriter(str(tmp_path / "data" / "self1") + "/", "distnodes", 0, 50, 0.0, 5000.0).write(rows)
    paths = [str(tmp_path / "data" / "self1" / "distnodes*")]
    path = os.path.join(str(tmp_path), "pytorch_model", "model_checkpoint_dist")
    model = Model_Dist(atoms=50, backend="hip", seed=0)
    seen = _spy_fisher(model, monkeypatch)
    kw = dict(max_iters=20, batch_size=64, weighted=True, weighted_mode=1, validation=True, val_set_size=0.1)
    res = O.fit_dist_nodes(model, paths, ewc_lambda=1.0, **kw)
    assert res["n_train"] == 360 and res["n_val"] == 40 and res["ewc"] == dict(penalised=False, fisher_rows=360)
    fdata, fk = seen[0]
    assert fk == dict(weighted=True, state_format="packed") and fdata[0].dtype == torch.int32 and fdata[0].shape == (360, 12)
    assert fdata[1].shape == (360, 50) and abs(float(fdata[2].mean()) - 1.0) < 0.2 and float(fdata[2].std()) > 0
    _carries_a_fisher(model, path)
    fresh = Model_Dist(atoms=50, backend="hip", seed=1)
    fresh.load(verbose=False)
    assert torch.equal(fresh.fisher, model.fisher) and torch.equal(fresh.ewc_anchor, model.ewc_anchor)
    first = model.fisher.clone()
    res2 = O.fit_dist_nodes(fresh, paths, ewc_lambda=1.0, **kw)
    assert res2["ewc"] == dict(penalised=True, fisher_rows=360) and res2["graph_replay"] is True
    assert not torch.equal(fresh.fisher, first)
    # without ewc_lambda the model's Fisher is neither used nor replaced, and the result carries no ewc entry
    held = fresh.fisher.clone()
    res3 = O.fit_dist_nodes(fresh, paths, **kw)
    assert "ewc" not in res3 and torch.equal(fresh.fisher, held)
    # the command line, in this process
    _cli().main(["--dist_nodes", "--data_paths"] + paths + ["--max_iters", "20", "--batch_size", "64", "--ewc_dist", "--ewc_lambda", "1"])
    again = Model_Dist(atoms=50, backend="hip", seed=2)
    again.load(verbose=False)
    assert again.fisher is not None and not torch.equal(again.fisher, held)
