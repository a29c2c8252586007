"""The dense request path for evaluators the engine does not own (csrc/eval_requests.hip; TreeAgent's dense_requests /
evaluator_pure): tm_eval_gather against the padded render byte for byte inside guard bands, the scatters, whole trajectories
against today's path, the CPU oracle and the native loop, and the number of rows an evaluator is handed."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_helpers import hash_eval_torch

pytestmark = pytest.mark.gpu
SHARE = 512                 # TM_EVAL_GATHER_SHARE: the slots a workgroup of the gather takes
PATTERN = 0x5A5A5A5A        # fit_hip_cases.Arena's fill


def _make(name, G, sims, max_nodes, seed, **kw):
    from test_gpu_tree import _make as make
    return make(name, G, sims, max_nodes, seed, **kw)


def _uniform_dist(boards):
    return np.full((len(boards), 50), 1.0 / 50, np.float32)


_stores = {}


def _stepped_store(name, G):
    """an agent whose store has been through update_root and four launches: eval_obs holds a launch's real requests"""
    if (name, G) not in _stores:
        from tetris_mcts_amd import store as st
        kw = dict(evaluator=_uniform_dist) if name == "DistValueSim" else dict(evaluator=hash_eval_torch)
        game, agent = _make(name, G, 8, 512, 300 + G, **kw)
        s = agent.store
        s.move_begin(8)
        s.sim_step(st.SIM_BACKUP | st.SIM_FRONT)
        for _ in range(3):
            agent.evaluate_requests()
            s.sim_step(st.SIM_BACKUP | st.SIM_FRONT)
        torch.cuda.synchronize()
        assert not bool(s.errors().any().item())
        _stores[(name, G)] = (agent, s.t["eval_obs"].clone())
    return _stores[(name, G)]


def _patterns(agent, real):
    """eval_obs contents: the launch's own, and patterns over valid indices (the game's root observation; TM_KIND_DIST: root node)"""
    from tetris_mcts_amd import store as st
    s = agent.store
    G, K = s.n_games, s.eval_slots
    g = torch.arange(G, device=s.device)
    root = s.t["gs"][:, st.GS["ROOT"]].long()
    ro = root if s.kind == st.KIND_DIST else s.t["node_rec"][g, root, 29].long()
    assert bool((ro > 0).all().item())
    every = ro.to(torch.int32).repeat_interleave(K)
    j = torch.arange(G * K, device=s.device)
    z = torch.zeros_like(every)
    return {"real": real, "zero": z, "every": every, "first": torch.where(j == 0, every, z),
            "last": torch.where(j == G * K - 1, every, z), "alternating": torch.where(j % 2 == 1, every, z)}


def _gather(s, cap, pad):
    """tm_eval_gather into buffers carved out of one tensor with guard bands; returns (arena, states, slots, count) after the
    guards were checked"""
    from fit_hip_cases import Arena
    arena = Arena()
    before = s.t["eval_obs"].clone()
    vs, vl, vc = arena(cap * 50, cap, {"eval_obs": s.t["eval_obs"]})
    rc = s.L.tm_eval_gather(C.byref(s.s), cap, pad, C.c_void_p(vs.data_ptr()), C.c_void_p(vl.data_ptr()),
                            C.c_void_p(vc.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    arena.check()                 # every guard byte, and eval_obs, unchanged
    assert torch.equal(before, s.t["eval_obs"])
    return arena, vs.view(torch.int8).view(cap, 200).cpu().numpy(), vl.view(torch.int32).cpu().numpy(), vc.view(torch.int32).cpu().numpy()


def _check_gather(s, ref, eo, cap, pad):
    idx = np.nonzero(eo)[0]
    R = len(idx)
    n = min(R, cap)
    m = min(cap, -(-n // pad) * pad)
    arena, states, slots, count = _gather(s, cap, pad)
    assert count.tolist() == [R, n], (count, R, n)
    assert np.array_equal(slots[:n], idx[:n])
    assert states[:n].tobytes() == ref[idx[:n]].tobytes()
    assert not states[n:m].any() and (slots[n:m] == -1).all()
    assert (states[m:] == 0x5A).all(), "a row at or beyond m was written"
    assert (slots[m:] == PATTERN).all()
    return arena, R


@pytest.mark.parametrize("name,G", [("ValueSimLP", 4), ("ValueSimLP", 12), ("ValueSimLP", 300), ("ValueSimLP", (6 * SHARE + 1) // 7),
                                    ("ValueSim", 68), ("DistValueSim", 12)])
def test_gather_is_the_padded_render_compacted(name, G):
    """28, 84 (across a wave), 2 100 and 3 073 (a whole number of workgroups' shares and one) leaf-parallel slots, 68 single-leaf
    ones and 12 of the distributional kind: slots = the ascending non-zero indices of eval_obs, rows = tm_eval_render's for those
    slots byte for byte, padding rows zero with slot -1, count, nothing written beyond row m or outside the buffers (cap = 5 < R
    included), and the same bytes from a second call."""
    agent, real = _stepped_store(name, G)
    s = agent.store
    total = s.n_games * s.eval_slots
    if name == "ValueSimLP" and G > 300:
        assert total % SHARE == 1
    seen_R = set()
    try:
        for pname, eo_dev in _patterns(agent, real).items():
            s.t["eval_obs"].copy_(eo_dev)
            ref = s.render_eval().cpu().numpy()
            eo = eo_dev.cpu().numpy()
            for pad in (1, 7, 256):
                arena, R = _check_gather(s, ref, eo, total, pad)
                seen_R.add(R)
            again, _ = _check_gather(s, ref, eo, total, 256)
            assert torch.equal(arena.arena, again.arena), pname
            if R > 5:
                _check_gather(s, ref, eo, 5, 7)
                _check_gather(s, ref, eo, 5, 2)
            if R > 1:
                _check_gather(s, ref, eo, R - 1, 256)
    finally:
        s.t["eval_obs"].copy_(real)
    assert 0 in seen_R and 1 in seen_R and total in seen_R and len(seen_R) >= 4


def test_gather_on_a_slice_counts_from_the_slice():
    """games [4, 12) of twelve as a store of their own (tm_store_slice): the requests of those games, slots relative to the slice"""
    from tetris_mcts_amd import _lib
    agent, real = _stepped_store("ValueSimLP", 12)
    s = agent.store
    sub = _lib.TmStore()
    assert s.L.tm_store_slice(C.byref(s.s), 4, 8, C.byref(sub)) == 0
    ref = s.render_eval().cpu().numpy()
    eo = real.cpu().numpy()
    idx = np.nonzero(eo[28:])[0]
    assert len(idx) > 0
    cap = 56
    states = torch.full((cap, 200), 0x5A, dtype=torch.int8, device=s.device)
    slots = torch.full((cap,), PATTERN, dtype=torch.int32, device=s.device)
    count = torch.zeros(2, dtype=torch.int32, device=s.device)
    rc = s.L.tm_eval_gather(C.byref(sub), cap, 1, C.c_void_p(states.data_ptr()), C.c_void_p(slots.data_ptr()),
                            C.c_void_p(count.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and count.tolist() == [len(idx), len(idx)]
    assert np.array_equal(slots.cpu().numpy()[:len(idx)], idx)
    assert states.cpu().numpy()[:len(idx)].tobytes() == ref[28 + idx].tobytes()
    assert bool((slots[len(idx):] == PATTERN).all().item())


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def test_scatter_writes_the_named_slots_only():
    agent, _ = _stepped_store("ValueSimLP", 12)
    s = agent.store
    total, dev = 84, s.device
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep_v, keep_var = s.t["eval_v"].clone(), s.t["eval_var"].clone()
    try:
        s.t["eval_v"].copy_(torch.arange(total, device=dev) * 0.25 + 1000)
        s.t["eval_var"].copy_(torch.arange(total, device=dev) * 0.5 + 2000)
        v0, var0 = s.t["eval_v"].clone(), s.t["eval_var"].clone()
        slots = torch.tensor([3, 83, -1, 5, 84, 10 ** 6, 0, 7], dtype=torch.int32, device=dev)       # 7: beyond count[1]
        v = torch.arange(8, device=dev, dtype=torch.float32) + 0.125
        var = torch.arange(8, device=dev, dtype=torch.float32) + 50.5
        count = torch.tensor([9, 0], dtype=torch.int32, device=dev)
        call = lambda: s.L.tm_eval_scatter(C.byref(s.s), C.c_void_p(slots.data_ptr()), C.c_void_p(count.data_ptr()),  # noqa: E731
                                           C.c_void_p(v.data_ptr()), C.c_void_p(var.data_ptr()), stream)
        assert call() == 0
        assert _bits(s.t["eval_v"]) == _bits(v0) and _bits(s.t["eval_var"]) == _bits(var0)          # count[1] = 0: nothing
        count[1] = 7
        assert call() == 0
        want_v, want_var = v0.clone(), var0.clone()
        for p, j in enumerate([3, 83, -1, 5, 84, 10 ** 6, 0]):
            if 0 <= j < total:
                want_v[j], want_var[j] = v[p], var[p]
        assert _bits(s.t["eval_v"]) == _bits(want_v) and _bits(s.t["eval_var"]) == _bits(want_var)
        assert s.t["eval_v"][7].item() == v0[7].item()
    finally:
        s.t["eval_v"].copy_(keep_v)
        s.t["eval_var"].copy_(keep_var)


def test_scatter_dist_writes_the_atoms_of_the_named_rows_only():
    agent, _ = _stepped_store("DistValueSim", 12)
    s = agent.store
    dev = s.device
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = s.t["eval_dist"].clone()
    try:
        s.t["eval_dist"].copy_(torch.arange(12 * 64, device=dev).reshape(12, 64) + 0.5)
        d0 = s.t["eval_dist"].clone()
        slots = torch.tensor([11, -1, 2, 12, 0, 4], dtype=torch.int32, device=dev)                  # 4: beyond count[1]
        dist = -(torch.arange(6 * 56, device=dev, dtype=torch.float32).reshape(6, 56) + 1)         # rows of 56 floats, 50 atoms
        count = torch.tensor([6, 0], dtype=torch.int32, device=dev)
        call = lambda stride: s.L.tm_eval_scatter_dist(C.byref(s.s), C.c_void_p(slots.data_ptr()), C.c_void_p(count.data_ptr()),  # noqa: E731
                                                       C.c_void_p(dist.data_ptr()), stride, stream)
        assert call(56) == 0
        assert _bits(s.t["eval_dist"]) == _bits(d0)
        assert call(49) == 1 and _bits(s.t["eval_dist"]) == _bits(d0)                              # hipErrorInvalidValue
        count[1] = 5
        assert call(56) == 0
        want = d0.clone()
        for p, j in enumerate([11, -1, 2, 12, 0]):
            if 0 <= j < 12:
                want[j, :50] = dist[p, :50]
        assert _bits(s.t["eval_dist"]) == _bits(want)
    finally:
        s.t["eval_dist"].copy_(keep)


# ---- whole trajectories ----
G_RUN, SIMS, MOVES, POOL = 6, 30, 40, 2500


class Switching:
    """hash_eval_torch, and from `switch()` on another function of the same hash (new weights)"""

    def __init__(self):
        self.mode = 0

    def __call__(self, states):
        v, var = hash_eval_torch(states)
        return (v, var) if self.mode == 0 else (v * np.float32(0.5) + np.float32(3.0), var + np.float32(1.0))


def _run(name, evaluator=hash_eval_torch, moves=MOVES, max_nodes=POOL, switch_at=None, model=None, seed=31, sims=SIMS, **kw):
    """(actions, the 84 statistics bytes per game) of every move, and the agent"""
    if model is not None:
        evaluator = None
    game, agent = _make(name, G_RUN, sims, max_nodes, seed, evaluator=evaluator, model=model, **kw)
    out = []
    for m in range(moves):
        if switch_at is not None and m == switch_at:
            evaluator.mode = 1
            agent.evaluator_changed()
        act = np.atleast_1d(agent.play())
        out.append((act.tolist(), agent.get_stats().reshape(G_RUN, -1).tobytes()))
        game.play(act)
        agent.update_root(game)
        if np.atleast_1d(game.end).any():
            game.reset("ended")
            agent.update_root(game)
    assert not bool(agent.store.errors().any().item())
    return out, agent


_padded = {}


def _padded_run(name):
    if name not in _padded:
        _padded[name], agent = _run(name)
        assert agent.store.counter("N_GC") >= 1, "the pool is meant to force collections"
    return _padded[name]


def _same(a, b, what):
    assert len(a) == len(b)
    for m, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0], (what, "actions of move", m, x[0], y[0])
        assert x[1] == y[1], (what, "statistics of move", m)


@pytest.mark.parametrize("pure", [False, True])
@pytest.mark.parametrize("name", ["ValueSim", "ValueSimLP", "ValueSimC"])
def test_dense_trajectories_are_todays(name, pure):
    """6 games x 30 simulations x 40 moves through collections, the hash evaluator as the callable: the dense path, and the dense
    path with TM_SIM_EVAL_NEEDED, play the padded path's actions with its statistics bytes"""
    got, agent = _run(name, dense_requests=True, evaluator_pure=pure, dense_pad=7)
    _same(got, _padded_run(name), (name, pure))
    if pure and name == "ValueSim":
        assert agent.store.counter("N_EVAL_CACHED") > 0          # leaves were answered from the per-observation cache


def test_dense_pure_leaf_parallel_against_the_oracle(oracle):
    from test_gpu_tree import _compare_run
    gcs = _compare_run(oracle, "ValueSimLP", G=G_RUN, sims=SIMS, max_nodes=POOL, seed=31, moves=MOVES, evaluator="hash",
                       dense_requests=True, evaluator_pure=True)
    assert gcs >= 1


def test_a_callable_that_changes_mid_run():
    """ValueSim, the callable's outputs switched before move 20 and evaluator_changed() told: dense + pure (whose cache must drop
    what the old function gave) matches the padded path given the same switch"""
    want, _ = _run("ValueSim", evaluator=Switching(), switch_at=20)
    got, agent = _run("ValueSim", evaluator=Switching(), switch_at=20, dense_requests=True, evaluator_pure=True)
    _same(got, want, "switch")
    assert agent.store.counter("N_EVAL_CACHED") > 0


@pytest.mark.parametrize("name", ["ValueSim", "ValueSimLP"])
def test_dense_pure_python_loop_is_the_native_loop(name, golden_dir):
    """the HIP value net wrapped as a callable through the dense + pure Python loop against the native loop of model="""
    import os
    from tetris_mcts_amd.model import Model_VV
    model = Model_VV(backend="hip")
    model.set_flat_params(np.load(os.path.join(golden_dir, "ref_valuenet.npz"))["params"])
    want, native = _run(name, model=model, moves=10, max_nodes=20000, sims=25)
    assert native.search_model() is model
    got, agent = _run(name, evaluator=lambda states: model.inference_device(states), moves=10, max_nodes=20000, sims=25,
                      dense_requests=True, evaluator_pure=True)
    assert agent.search_model() is False
    _same(got, want, name)
    for key in ("N_EVAL", "N_EVAL_CACHED", "N_EXPAND"):
        assert agent.store.counter(key) == native.store.counter(key), key


def _hash_dist(boards):
    """a softmax row per board from a hash of the board, each row a function of its own board alone"""
    b = np.asarray(boards).reshape(len(boards), 200).astype(np.int64)
    h = ((b + 2) * np.arange(1, 201, dtype=np.int64)).sum(1) % 1000003
    logits = np.sin((h[:, None] % 97) * 0.37 + np.arange(50)[None, :] * (0.11 + 0.01 * (h[:, None] % 7)))
    e = np.exp(2.0 * logits)
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def test_dist_agent_dense_is_padded():
    want, _ = _run("DistValueSim", evaluator=_hash_dist, moves=12, max_nodes=20000)
    seen = []

    def counting(boards):
        seen.append(boards.shape)
        return _hash_dist(boards)
    got, agent = _run("DistValueSim", evaluator=counting, moves=12, max_nodes=20000, dense_requests=True, dense_pad=4)
    _same(got, want, "DistValueSim")
    # the callable's contract is the padded path's, [rows, 20, 10] numpy; rows = the requests rounded up to dense_pad, at most every game
    assert seen and all(len(sh) == 3 and sh[1:] == (20, 10) and sh[0] in (4, G_RUN) for sh in seen)


def test_the_evaluator_is_handed_what_the_backup_will_use():
    """ValueSimLP, hash evaluator, dense + pure, dense_pad = 1: in every launch the rows handed over are the non-zero eval_obs slots
    counted before the call; over a move they are the requests the engine counts (TM_GS_N_EVAL), fewer than every slot of every
    launch; a launch without a request does not call the evaluator."""
    rows, calls = [], [0]

    def counting(states):
        calls[0] += 1
        rows.append(int(states.shape[0]))
        assert states.dtype == torch.int8 and states.is_cuda and states.shape[1] == 200
        return hash_eval_torch(states)
    game, agent = _make("ValueSimLP", G_RUN, SIMS, 20000, 31, evaluator=counting, dense_requests=True, evaluator_pure=True,
                        dense_pad=1)
    s = agent.store
    plain, launches, asked = agent.evaluate_requests, [0], []

    def watched():
        launches[0] += 1
        n = int((s.t["eval_obs"] != 0).sum().item())
        before = calls[0]
        plain()
        asked.append(n)
        assert calls[0] == before + (1 if n else 0)
        if n:
            assert rows[-1] == n
    agent.evaluate_requests = watched
    for m in range(6):
        n_eval, k0, l0 = s.counter("N_EVAL"), len(rows), launches[0]
        act = agent.play()
        total = sum(rows[k0:])
        assert total == s.counter("N_EVAL") - n_eval
        assert 0 < total < G_RUN * 7 * (launches[0] - l0)
        game.play(act)
        agent.update_root(game)
    assert s.counter("N_GC") == 0 and s.counter("N_EVAL_SKIP") > 0
    # a launch without a request: the evaluator is not called
    s.t["eval_obs"].zero_()
    before = calls[0]
    watched()
    assert calls[0] == before and asked[-1] == 0
