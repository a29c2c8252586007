"""Dist node records on the device (csrc/node_records.hip: tm_nodes_drain_dist, tm_node_dist_targets) against the byte statement
of the drain (tests/dist_node_cases.py), the numpy statement of the targets (nodes.node_dist_targets_numpy) and
TreeStore.replay_dist() inside a search; then the whole route at small scale: play.py --save_dist_nodes -> train.py --dist_nodes
-> checkpoint -> a DistValueSim that loads it.

The scan over the games is exercised at G = 1, 3, 70 and 4 097: one game, fewer games than a wave, more than a wave, more than a
workgroup has threads.  Every call writes into arrays carved out of one tensor of 0xA5 bytes, and the bytes around them are read
back (test_gpu_nodes.Guarded)."""
import contextlib
import ctypes as C
import importlib.util
import io
import os
from functools import partial

import numpy as np
import pytest
import torch

import dist_node_cases as K
from test_gpu_nodes import FILL, Guarded, _play, _stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 5          # replay_cap of the synthetic harvests


def _lib():
    from tetris_mcts_amd import _lib
    return _lib.lib()


def _small_store(G):
    from tetris_mcts_amd.store import KIND_DIST, TreeStore
    return TreeStore(G, max_nodes=64, max_trace=64, kind=KIND_DIST, online=True, min_visits_to_store=3, replay_cap=CAP)


def _drains(G, ring_cap, empties):
    """one drain per entry of `empties` (True: every game empty) into one guarded ring of ring_cap rows; checks the ring, the
    counters, replay_count, offsets and the guard bands against the statement"""
    store = _small_store(G)
    assert store.s.kind == K.KIND_DIST and store.t["replay_dist"].shape == (G, CAP, K.DIST_ROW)
    arena = Guarded([ring_cap * K.ROW, 16, 4 * (G + 1)])
    arena.zero(1)
    want, head, lost = [], 0, 0
    for i, empty in enumerate(empties):
        obs, stat, dist, count = K.harvest(G, CAP, 1000 * G + i, empty)
        store.t["replay_obs"].copy_(torch.from_numpy(obs.view(np.int32)))
        store.t["replay_stat"].copy_(torch.from_numpy(stat.view(np.float32)))
        store.t["replay_dist"].copy_(torch.from_numpy(dist.view(np.float32)))
        store.t["replay_count"].copy_(torch.from_numpy(count))
        rc = store.L.tm_nodes_drain_dist(C.byref(store.s), arena.ptr(0), ring_cap, arena.ptr(1), arena.ptr(2), _stream())
        assert rc == 0
        rows = K.drain_statement(obs, stat, dist, count, CAP)
        c = np.minimum(np.maximum(count, 0), CAP).astype(np.int64)
        first = np.minimum(head + np.concatenate([[0], np.cumsum(c)]), ring_cap)
        fits = min(head + len(rows), ring_cap) - head
        want.append(rows)
        head, lost = head + fits, lost + len(rows) - fits
        assert int(store.t["replay_count"].abs().sum().item()) == 0, "replay_count is cleared"
        assert arena.bytes(2).view(np.int32).tolist() == first.tolist(), ("offsets", i)
        # the sources are only read
        assert store.t["replay_dist"].cpu().numpy().view(np.uint32).tobytes() == dist.tobytes()
    arena.check()
    rows = np.concatenate(want)
    ring = arena.bytes(0).reshape(ring_cap, K.ROW)
    assert head == min(len(rows), ring_cap) and lost == len(rows) - head
    assert ring[:head].tobytes() == rows[:head].tobytes(), "the ring is the statement's rows, byte for byte"
    assert (ring[head:] == FILL).all(), "rows beyond head are not written"
    assert arena.bytes(1).view(np.int32).tolist() == [head, lost, len(empties), 0]
    return len(rows), head, lost


@pytest.mark.parametrize("G", [1, 3, 70, 4097])
def test_drain_on_synthetic_harvests(G):
    """random bytes in replay_obs / replay_stat / replay_dist, counts 0, 1, 5 and 9 (clamped to 5), some games empty; three drains
    in a row into one ring, the second with every game empty"""
    n, head, lost = _drains(G, 3 * CAP * G + 7, [False, True, False])
    assert n == head > 0 and lost == 0


@pytest.mark.parametrize("G", [1, 3, 70, 4097])
def test_drain_overflow(G):
    """a ring smaller than the total: the rows that fit are the statement's prefix, lost is the remainder, nothing beyond the ring
    is written and no error is raised; a ring that is full already takes nothing"""
    total, _, _ = _drains(G, 3 * CAP * G + 7, [False, False])
    cut = total // 2 + 1                                   # (inside a game's rows for G = 1: 5 + 1 rows, cut at 4)
    n, head, lost = _drains(G, cut, [False, False, False])
    assert head == cut and lost == n - cut > 0


def _searching(harvest):
    """the setting of test_dist_online_harvest_matches_the_oracle[1500-60-120] (tests/test_gpu_dist_agent.py), which harvests
    more than 50 tuples, with harvest=True in place of online=True"""
    import dist_regimes as R
    from test_gpu_dist_agent import hash_dist
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.pyTetris import Tetris
    G, r = 6, R.SUITE_SETTING
    env_args = R.env_args(r)
    game = Tetris(*env_args, seed=31337 + np.arange(G), n_games=G)
    kw = dict(harvest=True, min_visits_to_store=8, replay_cap=8192) if harvest else {}
    agent = agents.DistValueSim(atoms=r.atoms, vmin=r.vmin, vmax=r.vmax, sims=60, env=Tetris, env_args=env_args, n_games=G,
                                max_nodes=1500, evaluator=partial(hash_dist, bins=r.atoms), **kw)
    agent.update_root(game)
    return game, agent


def test_drain_inside_a_search():
    """120 moves: what every drain appends is TreeStore.replay_dist() taken just before it, bit for bit, with the game index (and
    the two zero words the harvest leaves in replay_stat); the actions are those of the same agent without harvest"""
    G, ring_cap = 6, 1 << 13
    game, agent = _searching(True)
    game0, plain = _searching(False)
    assert agent.store.s.online == 1 and plain.store.s.online == 0 and agent.online is False and agent.harvest is True
    assert agent.store.s.min_visits_to_store == 8 and agent.store.s.replay_cap == 8192 and plain.store.t["replay_dist"] is None
    store = agent.store
    arena = Guarded([ring_cap * K.ROW, 16, 4 * (G + 1)])
    arena.zero(1)
    want = []
    for m in range(120):
        a, b = _play(game, agent), _play(game0, plain)
        assert np.array_equal(a, b), ("actions", m)
        keys, dists, visits = store.replay_dist()
        cnt = store.t["replay_count"].clamp(min=0, max=store.s.replay_cap)
        slot = torch.repeat_interleave(torch.arange(G, device="cuda", dtype=torch.int32), cnt.long())
        zero = torch.zeros(keys.shape[0], 2, dtype=torch.int32, device="cuda")
        rows = torch.cat([keys.view(torch.int32), zero, visits.view(torch.int32)[:, None], slot[:, None], dists.view(torch.int32)], 1)
        want.append(rows.cpu().numpy())
        assert store.L.tm_nodes_drain_dist(C.byref(store.s), arena.ptr(0), ring_cap, arena.ptr(1), arena.ptr(2), _stream()) == 0
    arena.check()
    rows = np.concatenate(want)
    assert len(rows) >= 1, "no collection harvested: the test checks nothing"
    assert rows.shape[1] * 4 == K.ROW and len(rows) < ring_cap
    assert arena.bytes(1).view(np.int32).tolist() == [len(rows), 0, 120, 0]
    assert arena.bytes(0)[:len(rows) * K.ROW].tobytes() == rows.tobytes()
    assert int(store.t["replay_count"].sum().item()) == 0 and store.counter("N_DROPPED") == 0
    assert store.counter("N_GC") == plain.store.counter("N_GC") >= 1
    table = rows.view(np.uint8).reshape(-1).view(K.dist_dtype())
    assert (table["visit"] >= 8).all() and set(np.unique(table["slot"])) <= set(range(G))


def _targets_case(lib, rows, atoms, stride, wmode, shift=0):
    """one call of tm_node_dist_targets into guarded arrays (`shift`: bytes by which obs, target and weight are moved off their
    16-byte alignment), held to the numpy statement byte for byte"""
    from tetris_mcts_amd.nodes import node_dist_targets_numpy
    n = len(rows)
    rows_d = torch.from_numpy(rows.view(np.uint8).reshape(n, K.ROW).copy()).cuda()
    sizes = [n * 48, 4 * n * stride, 4 * n]
    arena = Guarded([s + shift for s in sizes] + [4])
    arena.zero(3)
    out = [C.c_void_p(arena.ptr(i).value + shift) for i in range(3)]
    rc = lib.tm_node_dist_targets(C.c_void_p(rows_d.data_ptr()), n, atoms, wmode, out[0], out[1], stride, out[2], arena.ptr(3), _stream())
    arena.check()
    obs, target, weight, fault = node_dist_targets_numpy(rows, atoms, wmode)
    assert rc == 0 and int(arena.bytes(3).view(np.int32)[0]) == fault
    got = [arena.bytes(i) for i in range(3)]
    assert all((g[:shift] == FILL).all() for g in got), "the bytes before a shifted array are not written"
    assert got[0][shift:].tobytes() == obs.tobytes() and got[2][shift:].tobytes() == weight.tobytes()
    full = np.full((n, stride), FILL * 0x01010101, np.uint32)
    full[:, :atoms] = target.view(np.uint32)
    assert got[1][shift:].tobytes() == full.tobytes(), "atoms copied bit for bit, the floats up to the stride keep the fill"
    return fault


@pytest.mark.parametrize("atoms", [7, 50, 64])
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_node_dist_targets_equal_the_numpy_statement(n, atoms):
    lib = _lib()
    for stride in sorted({atoms, 64}):
        for wmode in (0, 2):
            assert _targets_case(lib, K.synthetic_rows(n, n + atoms, atoms), atoms, stride, wmode) == 0
            for kind in K.FAULT_KINDS:
                rows = K.synthetic_rows(n, n + atoms, atoms)
                if not K.inject(rows, n // 2, kind, atoms):
                    continue
                assert _targets_case(lib, rows, atoms, stride, wmode) == 1, kind
    # arrays that are only 4-byte aligned, and faults in the first and the last row at once
    rows = K.synthetic_rows(n, n, atoms, faults=[(0, "visit_zero"), (n - 1, "atom_negative")])
    assert _targets_case(lib, rows, atoms, atoms, 2, shift=4) == 1
    assert _targets_case(lib, K.synthetic_rows(n, n, atoms), atoms, 64, 2, shift=12) == 0


def test_a_file_of_more_atoms_than_the_model_sets_the_fault_word():
    assert _targets_case(_lib(), K.synthetic_rows(100, 3, 50), 7, 7, 0) == 1


def test_refused_arguments_on_the_gpu():
    from tetris_mcts_amd import _lib
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    K.refused_dist_node_arguments(_lib, (t.data_ptr() + 15) // 16 * 16)
    torch.cuda.synchronize()
    assert not t.any()


def test_node_dist_targets_of_no_rows_launch_nothing():
    from tetris_mcts_amd import offline as O
    obs, target, weight = O.node_dist_targets(np.zeros(0, K.dist_dtype()), 50, device="cuda")
    assert obs.shape == (0, 12) and target.shape == (0, 50) and weight.shape == (0,)


def _cli():
    spec = importlib.util.spec_from_file_location("tm_train_cli_gpu_dist_nodes", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# the value net's route test runs 500 simulations a move; at that count this agent's pools collect too and the run below harvested
# 19 541 rows on an MI355X (33 660 at 1 000, 80 138 at 2 000), so the count stays where it started
ROUTE_SIMS = "500"


def test_route_play_save_dist_nodes_then_train_dist_nodes(tmp_path, monkeypatch):
    """play.py --save_dist_nodes at a size that still collects (the command line has no flag for the pool: a game's 100 000 nodes
    must fill), train.py --dist_nodes on what it wrote, the checkpoint; fit_dist_nodes against train_data on the same arrays; a
    DistValueSim that builds its own model loads the checkpoint and plays"""
    import play
    from tetris_mcts_amd import agents
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model_distributional import Model_Dist
    from tetris_mcts_amd.nodes import DistNodeLoader
    from tetris_mcts_amd.pyTetris import Tetris
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TM_TRAIN_GRAPH", "0")
    said = io.StringIO()
    with contextlib.redirect_stdout(said):      # (not capsys: a module first imported under it would keep its closed streams)
        play.main(["--agent_type", "DistValueSim", "--save_dist_nodes", "--min_visit", "3", "--n_games", "4", "--mcts_sims", ROUTE_SIMS,
                   "--max_moves", "120", "--endless", "--nodes_ring_rows", "65536", "--nodes_flush_moves", "2",
                   "--save_dir", "./data/self1/"])
    paths = [str(tmp_path / "data" / "self1" / "distnodes*")]
    ld = DistNodeLoader(O.choose_stems(paths))
    assert ld.length > 64, "no collection harvested enough: the route trains on nothing"
    assert "node rows written: %d in %d file(s), 0 lost" % (ld.length, len(ld.files)) in said.getvalue()
    assert (ld.atoms, ld.vmin, ld.vmax) == (50, 0.0, 5000.0)
    assert (ld.visit >= 3).all() and not ld.value.any() and not ld.variance.any() and set(np.unique(ld.slot)) <= set(range(4))
    assert np.isfinite(ld.dist).all() and (ld.dist >= 0).all() and not ld.dist[:, 50:].any()
    assert (ld.dist[:, :50] > 0).any(1).all()
    _cli().main(["--dist_nodes", "--data_paths"] + paths + ["--max_iters", "20", "--batch_size", "64", "--new"])
    assert os.path.isfile(os.path.join(str(tmp_path), "pytorch_model", "model_checkpoint_dist"))
    fresh = Model_Dist(atoms=50, backend="hip", seed=1)
    before = fresh.flat_params().clone()
    fresh.load(verbose=False)
    assert not torch.equal(before, fresh.flat_params()) and bool(torch.isfinite(fresh.flat_params()).all())
    assert not torch.equal(Model_Dist(atoms=50, backend="hip", seed=0).flat_params(), fresh.flat_params())
    # fit_dist_nodes = train_data(fit_backend="hip_dist", state_format="packed") on dist_node_training_set's arrays: the same bits
    a = Model_Dist(atoms=50, backend="hip", seed=0)
    torch.manual_seed(7)
    res = O.fit_dist_nodes(a, paths, max_iters=20, batch_size=64, weighted=True, weighted_mode=1)
    assert res["iters"] == 20 and res["n_train"] == ld.length and res["n_val"] == 0 and res["graph_replay"] is False
    assert (res["atoms"], res["vmin"], res["vmax"]) == (50, 0.0, 5000.0)
    b = Model_Dist(atoms=50, backend="hip", seed=0)
    data, info = O.dist_node_training_set(paths, weighted=True, weighted_mode=1, device=b.device)
    assert info["n"] == ld.length and data[0].cpu().numpy().tobytes() == ld.obs.tobytes()
    assert data[1].cpu().numpy().tobytes() == np.ascontiguousarray(ld.dist[:, :50]).tobytes()
    assert data[2].cpu().numpy().tobytes() == ld.visit.tobytes()
    torch.manual_seed(7)
    b.train_data(data, fit_backend="hip_dist", state_format="packed", shuffle=False, batch_size=64, max_iters=20,
                 validation_fraction=0.0, early_stopping=False, validation_backend="hip")
    assert torch.equal(a.flat_params(), b.flat_params())
    assert not torch.equal(a.flat_params(), Model_Dist(atoms=50, backend="hip", seed=0).flat_params())
    # held-out rows need the HIP validation, a model of other atoms is refused
    with pytest.raises(ValueError, match="validation_backend='hip'"):
        O.fit_dist_nodes(a, paths, max_iters=5, validation=True, val_set_size=0.1, validation_backend="torch")
    with pytest.raises(ValueError, match="50 atoms, the model has 64"):
        O.fit_dist_nodes(Model_Dist(atoms=64, backend="hip", seed=0), paths, max_iters=5)
    # the checkpoint is fit_dist_nodes' now: a DistValueSim that builds its own model loads it and plays
    game = Tetris((20, 10), 1, 0, 0, seed=5, n_games=2)
    agent = agents.DistValueSim(sims=20, env=Tetris, env_args=game.env_args, n_games=2, max_nodes=2000)
    assert torch.equal(agent.model.flat_params(), a.flat_params())
    agent.update_root(game)
    act = np.atleast_1d(agent.play())
    assert act.shape == (2,) and ((act >= 0) & (act < 7)).all() and (agent.store.errors() == 0).all()
    agent.close()
