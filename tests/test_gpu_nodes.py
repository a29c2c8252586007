"""Node records on the device (csrc/node_records.hip: tm_nodes_drain, tm_nodes_sweep, tm_node_targets) against numpy statements
of their definitions (tests/node_cases.py, nodes.node_targets_numpy) and against TreeStore.replay() inside a search; then the
whole route at small scale: play.py --save_nodes -> train.py --nodes -> checkpoint.

The scan over the games is exercised at G = 1, 3, 70 and 4 097: one game, fewer games than a wave, more than a wave, more than a
workgroup has threads.  Every call writes into arrays carved out of one tensor of 0xA5 bytes, and the bytes around them are read
back."""
import contextlib
import ctypes as C
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

import node_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL = 4096, 0xA5
CAP = 5          # replay_cap of the synthetic harvests
EPS = 0.001


class Guarded:
    """the arrays a call writes, carved out of one device tensor with guard bands of FILL before, between and after them"""

    def __init__(self, sizes):
        off, self.seg = GUARD, []
        for n in sizes:
            self.seg.append((off, n))
            off = (off + n + 15) // 16 * 16 + GUARD
        self.t = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")

    def ptr(self, i):
        return C.c_void_p(self.t.data_ptr() + self.seg[i][0])

    def zero(self, i):
        o, n = self.seg[i]
        self.t[o:o + n] = 0

    def bytes(self, i):
        o, n = self.seg[i]
        return self.t[o:o + n].cpu().numpy()

    def check(self):
        torch.cuda.synchronize()
        outside = torch.ones(self.t.numel(), dtype=torch.bool, device="cuda")
        for o, n in self.seg:
            outside[o:o + n] = False
        bad = torch.nonzero(outside & (self.t != FILL)).flatten()
        assert bad.numel() == 0, ("stores outside the arrays at byte offsets", bad[:8].tolist(), self.seg)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _small_store(G):
    from tetris_mcts_amd.store import TreeStore
    return TreeStore(G, max_nodes=64, max_trace=64, online=True, min_visits_to_store=3, replay_cap=CAP)


def _drains(G, ring_cap, empties):
    """one drain per entry of `empties` (True: every game empty) into one guarded ring of ring_cap rows; checks the ring, the
    counters, replay_count, offsets and the guard bands against the statement"""
    store = _small_store(G)
    arena = Guarded([ring_cap * K.ROW, 16, 4 * (G + 1)])
    arena.zero(1)
    want, head, lost = [], 0, 0
    for i, empty in enumerate(empties):
        obs, stat, count = K.harvest(G, CAP, 1000 * G + i, empty)
        store.t["replay_obs"].copy_(torch.from_numpy(obs.view(np.int32)))
        store.t["replay_stat"].copy_(torch.from_numpy(stat.view(np.float32)))
        store.t["replay_count"].copy_(torch.from_numpy(count))
        rc = store.L.tm_nodes_drain(C.byref(store.s), arena.ptr(0), ring_cap, arena.ptr(1), arena.ptr(2), _stream())
        assert rc == 0
        rows = K.drain_statement(obs, stat, count, CAP)
        c = np.minimum(np.maximum(count, 0), CAP).astype(np.int64)
        first = np.minimum(head + np.concatenate([[0], np.cumsum(c)]), ring_cap)
        fits = min(head + len(rows), ring_cap) - head
        want.append(rows)
        head, lost = head + fits, lost + len(rows) - fits
        assert int(store.t["replay_count"].abs().sum().item()) == 0, "replay_count is cleared"
        assert arena.bytes(2).view(np.int32).tolist() == first.tolist(), ("offsets", i)
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
    """random bytes in replay_obs / replay_stat, counts 0, 1, 5 and 9 (clamped to 5), some games empty; three drains in a row into
    one ring, the second with every game empty"""
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


def _play(game, agent):
    act = agent.play()
    game.play(act)
    agent.update_root(game)
    if np.atleast_1d(game.end).any():
        game.reset("ended")
        agent.update_root(game)
    return np.atleast_1d(act).copy()


class _Replayed:
    """hash_eval_torch replayed from a captured graph: the function's own kernels on the agent's one buffer of rendered states, as
    one launch where the eager call makes some 350 (the searches of this file are bound by those launches, not by their work)"""

    def __init__(self):
        self.graph = None

    def __call__(self, states):
        from gpu_helpers import hash_eval_torch
        if self.graph is None:
            self.ptr, self.shape = states.data_ptr(), tuple(states.shape)
            hash_eval_torch(states)                       # (warm-up, outside the capture)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.out = hash_eval_torch(states)
        assert states.data_ptr() == self.ptr and tuple(states.shape) == self.shape, "the agent renders into one buffer"
        self.graph.replay()
        return self.out


def _harvesting(G=3, sims=40, max_nodes=6000, seed=21, **kw):
    """the setting of test_replay_harvest_matches_oracle (tests/test_gpu_tree.py) with harvest=True in place of online=True"""
    from test_gpu_tree import _make
    return _make("ValueSim", G, sims, max_nodes, seed, evaluator=_Replayed(), min_visits_to_store=3, replay_cap=20000, **kw)


def test_drain_inside_a_search():
    """120 moves: what every drain appends is TreeStore.replay() taken just before it, bit for bit, with the game index; the
    actions are those of the same agent without harvest.
    The setting is test_replay_harvest_matches_oracle's (tests/test_gpu_tree.py) with one departure: both agents' evaluator is
    hash_eval_torch replayed from a captured graph (_Replayed) instead of called eagerly.  The values are the eager call's bit for
    bit - the same kernels on the same buffer - and the two searches of 120 moves take 6 s instead of 19, which the eager
    evaluator spends on some 350 launches an evaluation."""
    G, ring_cap = 3, 1 << 16
    game, agent = _harvesting(harvest=True)
    game0, plain = _harvesting()
    assert agent.store.s.online == 1 and plain.store.s.online == 0 and agent.online is False and agent.harvest is True
    store = agent.store
    arena = Guarded([ring_cap * K.ROW, 16, 4 * (G + 1)])
    arena.zero(1)
    want, harvested_moves = [], 0
    for m in range(120):
        a, b = _play(game, agent), _play(game0, plain)
        assert np.array_equal(a, b), ("actions", m)
        keys, stats = store.replay()
        cnt = store.t["replay_count"].clamp(min=0, max=store.s.replay_cap)
        slot = torch.repeat_interleave(torch.arange(G, device="cuda", dtype=torch.int32), cnt.long())
        rows = torch.cat([keys.view(torch.int32), stats.view(torch.int32)[:, :3], slot[:, None]], 1)
        want.append(rows.cpu().numpy())
        harvested_moves += int(len(want[-1]) > 0)
        assert store.L.tm_nodes_drain(C.byref(store.s), arena.ptr(0), ring_cap, arena.ptr(1), arena.ptr(2), _stream()) == 0
    arena.check()
    rows = np.concatenate(want)
    assert harvested_moves >= 1 and len(rows) > 0, "no collection harvested: the test checks nothing"
    assert len(rows) < ring_cap
    assert arena.bytes(1).view(np.int32).tolist() == [len(rows), 0, 120, 0]
    assert arena.bytes(0)[:len(rows) * K.ROW].tobytes() == rows.tobytes()
    assert int(store.t["replay_count"].sum().item()) == 0 and store.counter("N_DROPPED") == 0
    assert store.counter("N_GC") == plain.store.counter("N_GC") >= 1


def test_sweep_and_close_with_occupied(tmp_path):
    """after 30 moves: tm_nodes_sweep's rows equal the statement built from obs_stat, obs_key and gs, the predicate agrees with
    export_game's visits and end_obs, and the store is byte-identical afterwards; NodeRecorder.close(occupied=True) writes the
    drained rows and then the swept ones"""
    from tetris_mcts_amd.nodes import NodeLoader, NodeRecorder
    G = 3
    game, agent = _harvesting(harvest=True)
    for m in range(30):
        _play(game, agent)
    store = agent.store
    before = {k: v.clone() for k, v in store.t.items() if v is not None}
    ring_cap = G * store.max_nodes
    arena = Guarded([ring_cap * K.ROW, 16, 4 * (G + 1)])
    arena.zero(1)
    assert store.L.tm_nodes_sweep(C.byref(store.s), arena.ptr(0), ring_cap, arena.ptr(1), arena.ptr(2), _stream()) == 0
    arena.check()
    for k, v in before.items():
        assert torch.equal(store.t[k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), ("the sweep changed", k)
    stat = before["obs_stat"].cpu().numpy().view(np.uint32)
    key = before["obs_key"].cpu().numpy().view(np.uint32)
    gs = before["gs"].cpu().numpy()
    rows, per = K.sweep_statement(stat, key, gs, 3)
    assert len(rows) > 0 and all(len(o) > 0 for o in per)
    assert arena.bytes(1).view(np.int32).tolist() == [len(rows), 0, 1, 0]
    assert arena.bytes(0)[:len(rows) * K.ROW].tobytes() == rows.tobytes()
    assert (arena.bytes(0)[len(rows) * K.ROW:] == FILL).all()
    # the predicate, from the exported tree of one game: enough visits, not the observation of a finished game, allocated
    g = 1
    ex = store.export_game(g)
    o = np.arange(store.max_nodes)
    want = o[(o >= gs[g, K.GS_LOW_OBS]) & (ex["visit"] >= 3) & (ex["end_obs"] == 0)]
    assert np.array_equal(want, per[g])
    took = rows.view(K.node_dtype()).reshape(-1)
    mine = took[took["slot"] == g]
    assert np.array_equal(mine["visit"], ex["visit"][want].astype(np.float32))
    assert mine["value"].tobytes() == ex["value"][want].tobytes() and mine["variance"].tobytes() == ex["variance"][want].tobytes()
    # the recorder's close: what is still in the harvest buffers first, then the sweep
    keys, stats = store.replay()
    pending = int(keys.shape[0])
    rec = NodeRecorder(str(tmp_path) + "/", "nodes", 0, G, ring_rows=ring_cap)
    rec.close(agent, occupied=True)
    ld = NodeLoader(str(tmp_path) + "/nodes0")
    assert ld.length == pending + len(rows) == rec.rows_written and rec.lost == 0
    assert ld.rows[pending:].tobytes() == rows.tobytes()
    assert ld.rows[:pending]["obs"].tobytes() == keys.cpu().numpy().tobytes()
    # a ring too small for the sweep loses rows, and says so
    rec = NodeRecorder(str(tmp_path) + "/", "small", 0, G, ring_rows=len(rows) - 2)
    rec.close(agent, occupied=True)
    assert rec.lost == 2 and rec.rows_written == len(rows) - 2


@pytest.mark.parametrize("n", [1, 63, 1000])
def test_node_targets_equal_the_numpy_statement(n):
    from tetris_mcts_amd.nodes import node_targets_numpy
    lib = _lib()
    for faults in ((), ((n // 2, "value", np.float32("nan")),), ((0, "visit", 0.0), (n - 1, "variance", np.float32("inf")))):
        rows = K.synthetic_rows(n, n, faults=faults)
        rows_d = torch.from_numpy(rows.view(np.uint8).reshape(n, K.ROW).copy()).cuda()
        for wmode in range(4):
            arena = Guarded([n * 48, 4 * n, 4 * n, 4 * n, 4])
            arena.zero(4)
            rc = lib.tm_node_targets(C.c_void_p(rows_d.data_ptr()), n, wmode, EPS, *(arena.ptr(i) for i in range(5)), _stream())
            arena.check()
            obs, value, variance, weight, fault = node_targets_numpy(rows, wmode, EPS)
            assert rc == 0 and int(arena.bytes(4).view(np.int32)[0]) == fault == int(bool(faults))
            for i, w in enumerate((obs, value, variance, weight)):
                assert arena.bytes(i).tobytes() == w.tobytes(), (wmode, i)


def _lib():
    from tetris_mcts_amd import _lib
    return _lib.lib()


def test_refused_arguments_on_the_gpu():
    from tetris_mcts_amd import _lib
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    K.refused_node_arguments(_lib, (t.data_ptr() + 15) // 16 * 16)
    torch.cuda.synchronize()
    assert not t.any()


def _cli():
    spec = importlib.util.spec_from_file_location("tm_train_cli_gpu_nodes", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_route_play_save_nodes_then_train_nodes(tmp_path, monkeypatch):
    """play.py --save_nodes at a size that still collects (the command line has no flag for the pool: a game's 100 000 nodes must
    fill, which takes some tens of thousands of simulations), train.py --nodes on what it wrote, the checkpoint; fit_nodes
    against train_data on the same arrays"""
    import play
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.nodes import NodeLoader
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TM_TRAIN_GRAPH", "0")
    said = io.StringIO()
    with contextlib.redirect_stdout(said):      # (not capsys: a module first imported under it would keep its closed streams)
        play.main(["--agent_type", "ValueSim", "--save_nodes", "--min_visit", "3", "--n_games", "4", "--mcts_sims", "500",
                   "--max_moves", "120", "--endless", "--nodes_ring_rows", "65536", "--nodes_flush_moves", "2",
                   "--save_dir", "./data/self1/"])
    paths = [str(tmp_path / "data" / "self1" / "nodes*")]
    ld = NodeLoader(O.choose_stems(paths))
    assert ld.length > 64, "no collection harvested: the route trains on nothing"
    assert "node rows written: %d in %d file(s), 0 lost" % (ld.length, len(ld.files)) in said.getvalue()
    assert (ld.visit >= 3).all() and np.isfinite(ld.value).all() and np.isfinite(ld.variance).all()
    assert set(np.unique(ld.slot)) <= set(range(4))
    _cli().main(["--nodes", "--td", "--data_paths"] + paths + ["--max_iters", "20", "--batch_size", "64", "--new"])
    assert os.path.isfile(os.path.join(str(tmp_path), "pytorch_model", "model_checkpoint"))
    fresh = Model_VV(backend="hip", seed=1)
    before = fresh.flat_params().clone()
    fresh.load(verbose=False)
    assert not torch.equal(before, fresh.flat_params()) and bool(torch.isfinite(fresh.flat_params()).all())
    # fit_nodes = train_data(state_format="packed") on node_training_set's arrays: the same weights, bit for bit
    a = Model_VV(backend="hip", seed=0)
    torch.manual_seed(7)
    res = O.fit_nodes(a, paths, max_iters=20, batch_size=64, weighted=True, weighted_mode=1)
    assert res["iters"] == 20 and res["n_train"] == ld.length and res["n_val"] == 0 and res["graph_replay"] is False
    b = Model_VV(backend="hip", seed=0)
    data, info = O.node_training_set(paths, weighted=True, weighted_mode=1, device=b.device)
    assert info["n"] == ld.length and data[0].cpu().numpy().tobytes() == ld.obs.tobytes()
    assert data[3].cpu().numpy().tobytes() == ld.visit.tobytes()
    torch.manual_seed(7)
    b.train_data(data, batch_size=64, max_iters=20, validation_fraction=0.0, shuffle=False, early_stopping=False,
                 fit_backend="hip", validation_backend="hip", state_format="packed")
    assert torch.equal(a.flat_params(), b.flat_params())
    assert not torch.equal(a.flat_params(), Model_VV(backend="hip", seed=0).flat_params())
    # held-out rows need the HIP validation
    with pytest.raises(ValueError, match="validation_backend='hip'"):
        O.fit_nodes(a, paths, max_iters=5, validation=True, val_set_size=0.1, validation_backend="torch")
