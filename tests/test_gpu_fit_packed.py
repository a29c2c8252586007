"""The packed route of the HIP fits on the GPU: tm_*_fit_grad_packed and tm_*_fit_validate_packed against their int8 twins on the
rendered rows, train_data(state_format="packed") against the dense fit, and the agents' fit_states="packed".  The kernels are the
int8 route's with the cell read from the observation and every later statement unchanged, so every comparison here is of bytes."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import dist_fit_cases as DC  # noqa: E402
import fit_hip_cases as FC  # noqa: E402
import fit_packed_cases as PC  # noqa: E402
import fit_validation_cases as FV  # noqa: E402

pytestmark = pytest.mark.gpu

VALUE_CASES = ("fresh net, batch 1", "fresh net, batch 33", "fresh net, batch 257", "fresh net, batch 1025",
               "fresh net, batch 1025, unweighted, idx NULL", "value_net_online_r06.pt, weighted, batch 1025")
# batches 1, 33 and 257 at 50 atoms; batch 33 at 17 atoms with a target stride of 64, and at 7
DIST_CASES = ("fixture, batch 1", "seed50, batch 33, stride 50", "fixture, batch 257", "seed17, batch 33, stride 64",
              "seed7, batch 33, stride 64")


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ------------------------------------------------------------------------------------------------------------- 1. value net gradient
@pytest.mark.parametrize("name", VALUE_CASES + ("300 rows with ended rows and edge pieces, batch 33",))
def test_value_net_gradient_is_the_int8_routes_bits(name):
    case = PC.mixed_value_case() if name.startswith("300 rows") else PC.value_cases()[name]
    g8, l8 = FC.hip_grad(case)
    gp, lp, _, _ = PC.value_grad_packed(case)
    assert g8.shape == (FC.N_LEARN,) and np.isfinite(g8).all() and np.isfinite(l8).all()
    assert _same(gp, g8) and _same(lp, l8)


# ------------------------------------------------------------------------------------------------------------------ 2. head gradient
@pytest.mark.parametrize("name", DIST_CASES)
def test_head_gradient_is_the_int8_routes_bits(name):
    case = DC.cases()[name]
    assert case["tstride"] == int(name.split("stride ")[1]) if "stride" in name else case["atoms"] == 50
    g8, l8 = DC.hip_grad(case)
    gp, lp, _, _ = PC.dist_grad_packed(case)
    assert g8.shape == (DC.n_params(case["atoms"]),) and np.isfinite(g8).all()
    assert _same(gp, g8) and _same(lp, l8)


# ---------------------------------------------------------------------------------------------------------------------- 3. validation
_VAL = {}


def _val_case(head):
    if head not in _VAL:
        case = PC.validation_case(head, 2050)
        _VAL[head] = (case, torch.from_numpy(PC.pack(case["data"][0])).cuda())
    return _VAL[head]


@pytest.mark.parametrize("n", [1, 1025, 2050])
@pytest.mark.parametrize("head", ["value", "dist"])
def test_validation_rows_are_the_int8_routes_bits(head, n):
    """chunk 1 024, slab 2 048: a one-row chunk, a partial second chunk, a second slab"""
    from tetris_mcts_amd import _lib
    chunk, slab = 1024, 2048
    case, keys = _val_case(head)
    inp = FV.device_inputs(case, n)
    nch = (n + chunk - 1) // chunk
    ws = torch.empty(FV.workspace_floats(case, slab), dtype=torch.float32, device="cuda")
    out = []
    for packed in (False, True):
        rows = torch.full((nch, 3), float("nan"), dtype=torch.float64, device="cuda")
        ws.fill_(float("nan"))
        err = PC.validate_packed(case, inp, keys, n, chunk, slab, rows, ws) if packed else FV.call(case, inp, n, chunk, slab, rows, ws)
        _lib.check(err, "fit_validate")
        torch.cuda.synchronize()
        out.append(rows.cpu())
    dense, packed = out
    assert torch.isfinite(dense[:, :2]).all()
    if n == 1:
        assert torch.isnan(dense[0, 2]) if head == "dist" else dense[0, 2] == 0
    assert torch.equal(dense.view(torch.int64), packed.view(torch.int64))


# ---------------------------------------------------------------------------------------------------------------- 4. stores stay inside
@pytest.mark.parametrize("head", ["value", "dist"])
def test_the_packed_call_writes_only_where_it_says(head):
    arena = FC.Arena()
    if head == "value":
        g, l, keys, before = PC.value_grad_packed(PC.value_cases()["fresh net, batch 33"], place=arena)
    else:
        g, l, keys, before = PC.dist_grad_packed(DC.cases()["seed50, batch 33, stride 50"], place=arena)
    arena.check()
    assert np.isfinite(g).all() and np.isfinite(l).all()
    assert keys.cpu().numpy().tobytes() == before


# ------------------------------------------------------------------------------------------------------------------- 5. a whole fit
def _fit_rows(head, n=2000):
    boards = FC.boards(n, 5)[0]
    if head == "value":
        _, value, variance, weight = FC.dataset(n, 5)
        rest = [a.reshape(-1, 1) for a in (value, variance, weight * 10)]
        dense = boards.reshape(n, 1, 20, 10).astype(np.float32)
    else:
        _, target, weight = DC.dataset(n, 50, 5)
        rest = [target, (weight * 10).reshape(-1, 1)]
        dense = np.zeros((n, 1, 22, 10), np.float32)
        dense[:, 0, 2:] = boards.reshape(n, 20, 10)
    return dense, torch.from_numpy(PC.pack(boards)).cuda(), rest


def _new_model(head, tmp_path, monkeypatch):
    from tetris_mcts_amd import model as M
    from tetris_mcts_amd.model_distributional import Model_Dist
    monkeypatch.setattr(M, "EXP_PATH", str(tmp_path) + "/")
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(5)
    return Model_Dist(atoms=50, seed=0, backend="torch") if head == "dist" else M.Model_VV(backend="torch", seed=0)


def _flat(mdl):
    return torch.cat([p.detach().reshape(-1) for p in mdl.model.parameters()]).cpu().numpy().tobytes()


@pytest.mark.parametrize("head", ["value", "dist"])
def test_a_whole_fit_on_packed_rows_is_the_dense_fit_bit_for_bit(head, tmp_path, monkeypatch):
    from tetris_mcts_amd import train as T
    monkeypatch.setenv("TM_TRAIN_GRAPH", "1")
    dense, keys, rest = _fit_rows(head)
    Fit = T.HipDistFit if head == "dist" else T.HipFit
    made, real = [], Fit.__init__

    def recording(self, *a, **k):
        real(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(Fit, "__init__", recording)
    kw = dict(fit_backend="hip_dist" if head == "dist" else "hip", validation_backend="hip", batch_size=64, max_iters=30,
              iters_per_val=10, log=False)
    res, bits = {}, {}
    for fmt in ("dense", "packed"):
        mdl = _new_model(head, tmp_path, monkeypatch)
        start = _flat(mdl)
        res[fmt] = mdl.train_data([dense if fmt == "dense" else keys] + list(rest), state_format=fmt, **kw)
        bits[fmt] = _flat(mdl)
        assert bits[fmt] != start and res[fmt]["graph_replay"] is True and res[fmt]["iters"] == 30
    assert bits["packed"] == bits["dense"]
    assert res["packed"] == res["dense"]
    hip_d, hip_p = made
    assert hip_d.states.dtype == torch.int8 and not hip_d.packed and hip_p.packed
    assert hip_p.states.dtype == torch.int32 and tuple(hip_p.states.shape) == (hip_p.rows, 12) and hip_p.rows == 1800
    assert hip_p.states.data_ptr() == keys.data_ptr()                                # the caller's storage: no copy
    assert hip_p.val_states.dtype == torch.int32 and tuple(hip_p.val_states.shape) == (200, 12)
    assert hip_p.val_states.data_ptr() == keys.data_ptr() + 1800 * 48


# -------------------------------------------------------------------------------------------------------------------- 6. the agents
def _boom(*a, **k):
    raise AssertionError("dist.render_observations was called on the packed route")


def test_valuesim_fits_on_the_observations_it_harvests(tmp_path, monkeypatch):
    """the set-up of test_gpu_tree.test_online_training_loop with fit_states="packed": the fit runs with
    dist.render_observations out of reach, a dump renders, and the harvested tuples give the same weights in either format"""
    from tetris_mcts_amd import agents, dist as tdist, model as M
    from tetris_mcts_amd.pyTetris import Tetris
    monkeypatch.setattr(M, "EXP_PATH", str(tmp_path) + "/")
    monkeypatch.chdir(tmp_path)
    model = M.Model_VV(backend="hip", seed=0)
    env_args = ((20, 10), 1, 0, 0)
    game = Tetris(*env_args, seed=5, n_games=16)
    agent = agents.ValueSim(sims=40, env=Tetris, env_args=env_args, n_games=16, max_nodes=5000, model=model, online=True,
                            min_visits_to_store=3, replay_cap=8192, memory_growth_rate=1, fit_backend="hip",
                            validation_backend="hip", fit_states="packed")
    agent.update_root(game)
    before = model.flat_params().clone()
    for m in range(90):
        game.play(agent.play())
        agent.update_root(game)
        if game.end.any():
            game.reset("ended")
            agent.update_root(game)
    n_tuples = int(agent.store.t["replay_count"].sum().item())
    assert agent.store.counter("N_GC") >= 1 and n_tuples > 50
    held = tuple(t.clone() for t in agent.store.replay())
    with monkeypatch.context() as m:
        m.setattr(tdist, "render_observations", _boom)
        res = agent.train_nodes(max_iters=24, iters_per_val=8, batch_size=64, log=False)
    assert res is not None and res["iters"] == 24 and res["graph_replay"] is True
    assert not torch.equal(before, model.flat_params())
    assert int(agent.store.t["replay_count"].sum().item()) == 0
    act = agent.play()
    assert act.shape == (16,) and (agent.store.errors() == 0).all()
    # a dump renders (for the dump alone): the held rows again, through the rows the agent carries between two looks
    agent._memory = held
    res = agent.train_nodes(max_iters=8, iters_per_val=8, batch_size=64, log=False, dump_data=True, dump_path=str(tmp_path / "data" / "dump"))
    assert res is not None
    dump = np.load(str(tmp_path / "data" / "dump.npz"))
    assert sorted(dump.files) == ["states", "values", "variance", "weights"]
    assert dump["states"].shape == (n_tuples, 1, 20, 10) and dump["weights"].shape == (n_tuples, 1)
    assert set(np.unique(dump["states"])) <= {-1.0, 0.0, 1.0} and (dump["weights"] >= 3).all()
    # the harvested tuples, fitted in either format from the same weights
    keys, stats = held[0].view(torch.int32).reshape(-1, 12), held[1]
    bits = {}
    for fmt in ("dense", "packed"):
        torch.manual_seed(5)
        mdl = M.Model_VV(backend="torch", seed=0)
        data = list(tdist.training_arrays(keys, stats)) if fmt == "dense" else [keys] + list(tdist.training_targets(stats))
        r = mdl.train_data(data, state_format=fmt, fit_backend="hip", validation_backend="hip", max_iters=24, iters_per_val=8,
                           batch_size=64, log=False)
        assert r["iters"] == 24
        bits[fmt] = mdl.flat_params().cpu().numpy().tobytes()
    assert bits["dense"] == bits["packed"]


def test_distvaluesim_fits_on_the_observations_it_harvests(tmp_path, monkeypatch):
    """the short run of test_gpu_dist_fit_hip's online round with fit_states="packed" """
    from tetris_mcts_amd import agents, dist as tdist
    from tetris_mcts_amd.model_distributional import Model_Dist
    from tetris_mcts_amd.pyTetris import Tetris
    monkeypatch.chdir(tmp_path)
    G, sims = 16, 60
    env_args = ((20, 10), 1, 0, 0)
    game = Tetris(*env_args, seed=5, n_games=G)
    model = Model_Dist(atoms=50, seed=0, backend="hip")
    agent = agents.DistValueSim(sims=sims, env=Tetris, env_args=env_args, n_games=G, max_nodes=1500, model=model, online=True,
                                min_visits_to_store=4, memory_growth_rate=1, fit_backend="hip_dist", validation_backend="hip",
                                fit_states="packed")
    agent.update_root(game)
    before = model.flat_params().clone()
    for m in range(80):
        game.play(agent.play())
        agent.update_root(game)
        if game.end.any():
            game.reset("ended")
            agent.update_root(game)
        if int(agent.store.t["replay_count"].sum().item()) >= 64:
            break
    n_tuples = int(agent.store.t["replay_count"].sum().item())
    assert n_tuples >= 64
    held = tuple(t.clone() for t in agent.store.replay_dist())
    with monkeypatch.context() as m:
        m.setattr(tdist, "render_observations", _boom)
        res = agent.train_nodes(max_iters=8, iters_per_val=4, batch_size=64, log=False)
    assert res is not None and res["iters"] == 8
    assert not torch.equal(before, model.flat_params())
    assert int(agent.store.t["replay_count"].sum().item()) == 0
    agent.play()
    assert (agent.store.errors() == 0).all()
    agent._memory = held
    res = agent.train_nodes(max_iters=4, iters_per_val=4, batch_size=64, log=False, dump_data=True, dump_path=str(tmp_path / "data" / "memory_dump"))
    assert res is not None
    dump = np.load(str(tmp_path / "data" / "memory_dump.npz"))
    assert sorted(dump.files) == ["states", "values", "weights"]
    assert dump["states"].shape == (n_tuples, 1, 22, 10) and (dump["states"][:, :, :2] == 0).all()
    assert set(np.unique(dump["states"])) <= {-1.0, 0.0, 1.0}
