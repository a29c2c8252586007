"""One tree kernel per agent family (tree.hip: k_sim_step<false>, k_sim_step_capped, k_sim_step<true>, k_sim_step_dist, chosen by
tm_sim_step from the store's kind and cap): every kind the store knows against its CPU oracle, bit for bit - actions and root
statistics move by move, then the games' counters - at the smallest shape at which a dispatch or a specialisation can go wrong:
8 games (two simulation workgroups of four waves), 60 simulations, 3 moves, and a node pool so small that the collector workgroups
collect beside the simulations and at least one game's reachable tree outgrows its pool (the reference's MAX_NODES EXCEEDED,
agent.cpp:227-231: the device restarts that game's tree at the update_root of the very move, and the game is compared up to it).

The pools are chosen on the oracle: test_the_oracle_alone_meets_a_collection_and_a_restart needs no GPU and proves, with the
reference's arithmetic alone, that every case has a game that collects and plays on and a game that runs out of nodes.  The oracle's
moves are computed once per case and shared by both tests."""
import random
from concurrent.futures import ThreadPoolExecutor
from functools import partial

import numpy as np
import pytest

G, SIMS, MOVES, SEED = 8, 60, 3, 9100
ENV_ARGS = ((20, 10), 1, 0, 0)
# case -> (agent class, oracle kind, node pool)
CASES = {
    "ValueSim": ("ValueSim", 0, 700),
    "ValueSim-cap3": ("ValueSim", 0, 700),              # k_sim_step_capped beside the collections
    "ValueSimLP": ("ValueSimLP", 1, 720),
    "ValueSimC-LP": ("ValueSimC", 2, 800),              # the cppagent kinds: leaf-parallel ...
    "ValueSimC-single": ("ValueSimC", 3, 700),          # ... and single-leaf
    "Vanilla": ("Vanilla", 4, 500),
    "VanillaC": ("VanillaC", 5, 400),
    "DistValueSim": ("DistValueSim", 6, 520),           # the HIP head inside the native loop
    "DistValueSim-online": ("DistValueSim", 6, 480),    # the harvest at the collections (the hash evaluator, as the harvest's own tests)
}
MT_SEED = 3                  # the rollout kinds' CPython streams: game g draws from random.Random(MT_SEED + g)
HARVEST_MIN_VISITS = 2
_oracle_runs = {}


def _value_params():
    import torch
    from tetris_mcts_amd.model import Model_VV
    return Model_VV(backend="torch", device="cpu", seed=0).flat_params().numpy()


def _dist_params():
    from tetris_mcts_amd.model_distributional import Model_Dist
    return Model_Dist(atoms=50, device="cpu", seed=0, backend="torch").flat_params().numpy()


def _oracle_run(oracle, case):
    """The case's 8 games on the oracle alone: per game the (action, statistics bytes) of every move up to the one in which its
    pool is exhausted (`err_at`, -1: never), its counters and, in the online case, what it harvested."""
    _, kind, pool = CASES[case]
    key = (kind, pool, case if kind == 6 else "")       # (the cap is a change of schedule only: the same oracle run)
    if key in _oracle_runs:
        return _oracle_runs[key]
    kw = {}
    if kind < 4:
        kw = dict(evaluator="valuenet", params=_value_params())
    elif kind == 4:
        kw = dict(gamma=0.99, low=5)
    elif kind == 5:
        kw = dict(gamma=0.99, low=1)
    elif case == "DistValueSim":
        kw = dict(low=5, evaluator="distnet", params=_dist_params())
    else:
        kw = dict(low=5, online=True, min_visits_to_store=HARVEST_MIN_VISITS, memory_size=100000)

    def one(g):
        og = oracle.Game(*ENV_ARGS[1:], seed=SEED + g)
        oa = oracle.Agent(kind, max_nodes=pool, **kw)
        if kind in (4, 5):
            oa.set_python_random_state(random.Random(MT_SEED + g).getstate())
        oa.update_root(og)
        moves, err_at = [], -1
        for m in range(MOVES):
            a = oa.play(SIMS)
            if oa.error:
                err_at = m
                break
            moves.append((a, oa.stats().tobytes()))
            og.play(a)
            assert not og.end
            oa.update_root(og)
        return dict(moves=moves, err_at=err_at, n_gc=oa.n_gc, n_expand=oa.n_expand, n_sims=oa.n_sims,
                    harvest=oa.memory_dist() if case == "DistValueSim-online" else None)

    with ThreadPoolExecutor(max_workers=G) as pool_:          # (the oracle releases the GIL)
        games = list(pool_.map(one, range(G)))
    _oracle_runs[key] = games
    return games


@pytest.mark.parametrize("case", list(CASES))
def test_the_oracle_alone_meets_a_collection_and_a_restart(oracle, case):
    games = _oracle_run(oracle, case)
    assert any(r["err_at"] < 0 and r["n_gc"] > 0 for r in games), [(r["n_gc"], r["err_at"]) for r in games]   # collected, played on
    assert any(r["err_at"] >= 0 for r in games), [(r["n_gc"], r["err_at"]) for r in games]                      # MAX_NODES EXCEEDED
    assert all(len(r["moves"]) == (MOVES if r["err_at"] < 0 else r["err_at"]) for r in games)
    if case == "DistValueSim-online":
        assert sum(len(r["harvest"][2]) for r in games if r["err_at"] < 0) > 0


def _device_agent(case):
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.model_distributional import Model_Dist
    from tetris_mcts_amd.pyTetris import Tetris
    name, kind, pool = CASES[case]
    game = Tetris(*ENV_ARGS, seed=SEED, n_games=G)
    kw = dict(sims=SIMS, env=Tetris, env_args=ENV_ARGS, n_games=G, max_nodes=pool)
    if kind < 4:
        model = Model_VV(backend="hip", seed=0)
        assert np.array_equal(model.flat_params().cpu().numpy(), _value_params())
        kw.update(model=model, online=False)
        if name == "ValueSimC":
            kw.update(leaf_parallel=kind == 2)
    elif kind in (4, 5):
        kw.update(random_seed=MT_SEED)
    elif case == "DistValueSim":
        model = Model_Dist(atoms=50, seed=0, backend="hip")
        assert np.array_equal(model.flat_params().cpu().numpy(), _dist_params())
        kw.update(model=model)
    else:
        from test_gpu_dist_agent import hash_dist
        kw.update(atoms=50, vmin=0.0, vmax=5000.0, evaluator=partial(hash_dist, bins=50), online=True,
                  min_visits_to_store=HARVEST_MIN_VISITS, replay_cap=8192)
    agent = getattr(agents, name)(**kw)
    agent.update_root(game)
    if case == "ValueSim-cap3":
        agent.store.set_request_cap(3, n_sub=agent.n_sub, ev_every=agent.ev_every)
    return game, agent


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_every_kind_matches_its_oracle_through_collections_and_a_restart(oracle, case):
    from tetris_mcts_amd import dist as tdist, store as st
    ref = _oracle_run(oracle, case)
    game, agent = _device_agent(case)
    S = agent.store
    resets = np.zeros((MOVES, G), np.int64)         # TM_GS_N_POOL_RESET after the move's update_root
    for m in range(MOVES):
        act = np.atleast_1d(agent.play())
        stats = agent.get_stats().reshape(G, 3, 7)
        for g, r in enumerate(ref):
            if m < len(r["moves"]):
                a, sb = r["moves"][m]
                assert a == act[g], (case, "action", m, g, a, act[g])
                assert sb == stats[g].tobytes(), (case, "stats", m, g)
        game.play(act)
        agent.update_root(game)
        assert not np.atleast_1d(game.end).any()
        resets[m] = S.t["gs"][:, st.GS["N_POOL_RESET"]].cpu().numpy()
    gs = S.t["gs"].cpu().numpy()
    assert int((gs[:, st.GS["ERR"]] & ~1).sum()) == 0                    # no error flag but the pool one
    for g, r in enumerate(ref):
        e = r["err_at"]
        if e >= 0:
            # the tree was restarted at the update_root of the very move in which the reference runs out of nodes
            assert resets[e, g] >= 1 and (e == 0 or resets[e - 1, g] == 0), (case, g, e, resets[:, g])
            continue
        assert resets[MOVES - 1, g] == 0 and gs[g, st.GS["ERR"]] == 0, (case, g)
        assert (gs[g, st.GS["N_GC"]], gs[g, st.GS["N_EXPAND"]], gs[g, st.GS["N_SIMS"]]) == (r["n_gc"], r["n_expand"], r["n_sims"]), (case, g)
    if case == "ValueSim-cap3":
        assert int(gs[:, st.GS["N_EVAL_DEFERRED"]].sum()) > 0            # the cap left requests out: the capped kernel's own path ran
    if case == "DistValueSim-online":
        cnt = S.t["replay_count"].cpu().numpy()
        for g, r in enumerate(ref):
            if r["err_at"] >= 0:
                continue
            states, d, v = r["harvest"]
            assert cnt[g] == len(v), (g, cnt[g], len(v))
            if cnt[g]:
                dev_states = tdist.render_observations(S.t["replay_obs"][g, :cnt[g]]).reshape(-1, 200).cpu().numpy().astype(np.int8)
                assert np.array_equal(dev_states, states), g
                assert S.t["replay_dist"][g, :cnt[g], :50].cpu().numpy().tobytes() == d.tobytes(), g
                assert S.t["replay_stat"][g, :cnt[g], 2].cpu().numpy().tobytes() == v.tobytes(), g
