"""The request cap of the native loop (tm_search_set_request_cap; tree.hip TM_PENDING_POSTED, valuenet.hip ReqList::cap): the value
net serves the first `cap` requests of a launch, the games of the others post theirs again, do not back up and catch up at the
end of the move.  A change of schedule only - so a capped run is held, bit for bit, to the run without the cap: actions, root
statistics, the games, the counters.  Caps far below the requests a launch posts (3, 17, half the games) make every launch defer,
which the counter of re-posted requests proves; nothing is left owing when tm_search_run returns."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIMS, MOVES, POOL = 40, 6, 8000
COUNTERS = ("N_SIMS", "N_EXPAND", "N_EVAL", "N_EVAL_CACHED", "ERR")
_runs = {}


def _run(agent_name, G, cap, pool=POOL, moves=MOVES, bump_at=None):
    """`moves` moves of G games under `cap` (-1: off); what the moves handed the caller and the games' counters.  One run per
    argument tuple, shared by the tests (the runs without a cap are every capped run's reference)."""
    key = (agent_name, G, cap, pool, moves, bump_at)
    if key in _runs:
        return _runs[key]
    from tetris_mcts_amd import agents, store as st
    from tetris_mcts_amd.model import Model_VV, next_weights_epoch
    from tetris_mcts_amd.pyTetris import Tetris
    model = Model_VV(backend="hip", seed=0)
    game = Tetris((20, 10), 1, 0, 0, seed=7000, n_games=G)
    kw = dict(sims=SIMS, env=Tetris, env_args=game.env_args, n_games=G, max_nodes=pool, model=model, online=False)
    agent = agents.ValueSimC(leaf_parallel=False, **kw) if agent_name == "ValueSimC" else agents.ValueSim(**kw)
    agent.update_root(game)
    S = agent.store
    assert S.eval_slots == 1
    S.set_request_cap(cap, n_sub=agent.n_sub, ev_every=agent.ev_every)
    out = dict(actions=[], stats=[], games=[], owing=[])
    for m in range(moves):
        if bump_at is not None and m == bump_at:
            model.weights_epoch = next_weights_epoch()      # (what a fit does: outputs filed per observation are not used again)
        a = agent.play()
        gs = S.t["gs"].cpu().numpy()
        out["owing"].append(int(np.abs(gs[:, st.GS["SIM_TARGET"]] - gs[:, st.GS["SIM_STARTED"]]).sum() + (gs[:, st.GS["PENDING"]] != 0).sum()))
        out["actions"].append(np.array(a, copy=True))
        out["stats"].append(agent.get_stats())
        game.play(a)
        agent.update_root(game)
        if np.atleast_1d(game.end).any():
            game.reset("ended")
            agent.update_root(game)
        out["games"].append(game.packed().copy())
    torch.cuda.synchronize()
    gs = S.t["gs"].cpu().numpy()
    out["counters"] = {k: gs[:, st.GS[k]].copy() for k in COUNTERS}
    out["deferred"] = int(gs[:, st.GS["N_EVAL_DEFERRED"]].sum())
    out["collections"] = int(gs[:, st.GS["N_GC"]].sum())
    out["catchup_launches"] = S.search_stats(agent.n_sub, agent.ev_every, reset=False)["catchup_launches"]
    _runs[key] = out
    return out


def _same(ref, got):
    for m in range(len(ref["actions"])):
        assert np.array_equal(ref["actions"][m], got["actions"][m]), ("actions", m)
        assert ref["stats"][m].tobytes() == got["stats"][m].tobytes(), ("root statistics", m)
        assert np.array_equal(ref["games"][m], got["games"][m]), ("games", m)
    for k in COUNTERS:
        assert np.array_equal(ref["counters"][k], got["counters"][k]), k
    assert (got["counters"]["ERR"] == 0).all()


@pytest.mark.parametrize("agent_name", ["ValueSim", "ValueSimC"])
@pytest.mark.parametrize("G", [96, 100])
@pytest.mark.parametrize("cap", [3, 17, "half"])
def test_capped_search_is_the_uncapped_search(agent_name, G, cap):
    cap = G // 2 if cap == "half" else cap
    ref, got = _run(agent_name, G, -1), _run(agent_name, G, cap)
    print("%s G=%d cap=%d: requests %d, posted again %d, catch-up launches %d (uncapped %d)"
          % (agent_name, G, cap, int(got["counters"]["N_EVAL"].sum()), got["deferred"], got["catchup_launches"], ref["catchup_launches"]))
    assert ref["deferred"] == 0
    assert got["deferred"] > 0                 # the path ran
    _same(ref, got)
    assert got["owing"] == [0] * MOVES and ref["owing"] == [0] * MOVES


def test_a_deferred_game_meets_a_collecting_game():
    """pools that run dry within the moves played: collections and deferrals in the same launches"""
    G, pool, moves = 96, 700, 10
    ref, got = _run("ValueSim", G, -1, pool=pool, moves=moves), _run("ValueSim", G, 17, pool=pool, moves=moves)
    print("collections %d / %d, posted again %d" % (ref["collections"], got["collections"], got["deferred"]))
    assert ref["collections"] > 0 and got["collections"] == ref["collections"]
    assert got["deferred"] > 0
    _same(ref, got)
    assert got["owing"] == [0] * moves


def test_cap_across_a_change_of_weights_epoch():
    """the evaluator's epoch moves on between two moves (what was filed per observation is not used again): more requests a
    launch from then on, deferred and served like the others"""
    ref, got = _run("ValueSim", 100, -1, bump_at=3), _run("ValueSim", 100, 17, bump_at=3)
    assert got["deferred"] > 0
    _same(ref, got)
    assert got["owing"] == [0] * MOVES
    # (the bump is felt: without it the same games post fewer requests)
    assert int(ref["counters"]["N_EVAL"].sum()) > int(_run("ValueSim", 100, -1)["counters"]["N_EVAL"].sum())


def test_stores_that_cannot_carry_a_cap_refuse_it():
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.pyTetris import Tetris
    game = Tetris((20, 10), 1, 0, 0, seed=5, n_games=8)
    lp = agents.ValueSimLP(sims=8, env=Tetris, env_args=game.env_args, n_games=8, max_nodes=2000, model=Model_VV(backend="hip", seed=0),
                           online=False)
    lp.update_root(game)
    for cap in (-1, 0):
        lp.store.set_request_cap(cap, n_sub=lp.n_sub, ev_every=lp.ev_every)
    with pytest.raises(RuntimeError):
        lp.store.set_request_cap(4, n_sub=lp.n_sub, ev_every=lp.ev_every)
    with pytest.raises(RuntimeError):
        lp.store.set_request_cap(-2, n_sub=lp.n_sub, ev_every=lp.ev_every)
