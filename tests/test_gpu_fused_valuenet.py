"""k_vn_conv_fc1 (valuenet_fused.inc), the convolutions and fc1 of the search's requests in one launch, against the two kernels
it replaces: for the same request list eval_v, eval_var and eval_served are equal bit for bit - at request counts around the
tile of 32 (1, 31, 32, 33, 65), on the launch's own grid and, through tm_valuenet_forward_requests_grid, on grids of 1 and 8
workgroups (several states a wave, several items a workgroup, tiles whose rows come from other workgroups), over a scratch full
of 0xFF bytes, under a request cap, across a change of the evaluator's epoch; and a short search with the one launch against the
same search under TM_VALUENET_FUSED=0 in a fresh process."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_ARGS = ((20, 10), 1, 0, 0)
GRIDS = (0, 1, 8)          # 0: the launch's own grid (one workgroup a compute unit, at most 256)


def _model():
    import heads_numerics as H
    from tetris_mcts_amd.model import Model_VV
    m = Model_VV(backend="hip", seed=0)
    m.set_flat_params(H.load_checkpoint("r06"))
    return m


def _agent(m, G, seed=41, moves=2):
    """a ValueSim store of G games a few moves into play (trees with visited nodes, filed outputs)"""
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.pyTetris import Tetris
    game = Tetris(*ENV_ARGS, seed=seed, n_games=G)
    agent = agents.ValueSim(sims=12, env=Tetris, env_args=ENV_ARGS, n_games=G, max_nodes=4000, model=m, online=False)
    agent.update_root(game)
    for _ in range(moves):
        act = agent.play()
        game.play(act)
        agent.update_root(game)
    return agent


def _list_games(s, games):
    """the next launches of the tree kernel run over these games only (tm_store::game_list)"""
    t = torch.tensor(list(games), dtype=torch.int32, device="cuda")
    s.t["game_list"] = t
    s.s.game_list, s.s.n_listed = t.data_ptr(), len(games)


def _requests(s):
    return int(s.t["eval_cnt"][:, s.s.eval_parity].sum().item())


def _evaluate(m, s, grid):
    """the pending list through the path `grid` names (< 0: the two kernels): (eval_v, eval_var, eval_served) bits"""
    from tetris_mcts_amd import _lib
    from tetris_mcts_amd.store import _stream
    P, prep, scr = m.hip_buffers(s.n_games * s.eval_slots)
    for k in ("eval_v", "eval_var"):
        s.t[k].fill_(float("nan"))
    s.t["eval_served"].fill_(-1)
    _lib.check(_lib.lib().tm_valuenet_forward_requests_grid(P, prep, 0, 0, C.byref(s.s), scr, _stream(), grid),
               "tm_valuenet_forward_requests_grid")
    return tuple(s.t[k].clone().view(torch.int32) for k in ("eval_v", "eval_var", "eval_served"))


def _hold(m, s, what, grids=GRIDS):
    ref = _evaluate(m, s, -1)
    assert not torch.isnan(ref[0].view(torch.float32)).all() or _requests(s) == 0
    for grid in grids:
        got = _evaluate(m, s, grid)
        for name, a, b in zip(("eval_v", "eval_var", "eval_served"), ref, got):
            assert torch.equal(a, b), (what, "grid", grid, name, int((a != b).sum()))
    _evaluate(m, s, -1)      # (the outputs the next backup reads: the reference's)


def _no_error():
    from tetris_mcts_amd import _lib
    torch.cuda.synchronize()
    assert _lib.lib().tm_valuenet_fused_error(1) == 0


@pytest.mark.parametrize("G,count", [(64, 1), (64, 31), (64, 32), (64, 33), (512, 65)])
def test_one_launch_is_the_two_kernels(G, count):
    from tetris_mcts_amd import store as st
    m = _model()
    s = _agent(m, G).store
    _list_games(s, range(G - count, G) if count > 1 else [G // 2])
    s.move_begin(8)
    for step in range(3):
        s.sim_step(st.SIM_BACKUP | st.SIM_FRONT)
        assert _requests(s) == count, (step, _requests(s))
        _hold(m, s, (G, count, step))
    _no_error()


def test_scratch_full_of_ones_before_its_first_use():
    from tetris_mcts_amd import store as st
    s = _agent(_model(), 64).store
    s.move_begin(8)
    s.sim_step(st.SIM_BACKUP | st.SIM_FRONT)
    ref = _evaluate(_model(), s, -1)
    for grid in GRIDS:
        m = _model()                                   # a model of its own: a scratch no launch has seen
        m._ensure_scratch(64).view(torch.uint8).fill_(0xFF)
        got = _evaluate(m, s, grid)
        assert all(torch.equal(a, b) for a, b in zip(ref, got)), grid
        got = _evaluate(m, s, grid)                    # and the same list again, on what the launch left behind
        assert all(torch.equal(a, b) for a, b in zip(ref, got)), grid
    _no_error()


def test_under_a_request_cap():
    from tetris_mcts_amd import store as st
    m = _model()
    s = _agent(m, 64).store
    s.move_begin(8)
    s.sim_step(st.SIM_BACKUP | st.SIM_FRONT)
    posted = _requests(s)
    assert posted > 17
    for rot in (0, 1):
        s.s.eval_cap, s.s.eval_rot = 17, rot
        _hold(m, s, ("cap", rot))
        assert int(s.t["eval_served"].sum().item()) == 17
    _no_error()


def test_across_a_change_of_epoch():
    from tetris_mcts_amd import store as st
    m = _model()
    s = _agent(m, 64).store
    s.move_begin(12)
    counts = []
    for step in range(4):
        if step == 2:
            s.s.eval_epoch += 1      # (other weights: nothing filed per observation answers a leaf any more)
        s.sim_step(st.SIM_BACKUP | st.SIM_FRONT | st.SIM_EVAL_NEEDED)
        counts.append(_requests(s))
        _hold(m, s, ("epoch", step))
    print("requests a launch:", counts)
    assert max(counts) > 0
    _no_error()


def _search(path=None):
    """64 games x 40 sims for 3 moves through the native loop: actions, root statistics, packed games"""
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.pyTetris import Tetris
    G = 64
    game = Tetris(*ENV_ARGS, seed=7000, n_games=G)
    agent = agents.ValueSim(sims=40, env=Tetris, env_args=ENV_ARGS, n_games=G, max_nodes=8000, model=Model_VV(backend="hip", seed=0),
                            online=False)
    agent.update_root(game)
    out = {}
    for mv in range(3):
        a = agent.play()
        out["actions%d" % mv] = np.array(a, copy=True)
        out["stats%d" % mv] = np.array(agent.get_stats(), copy=True)
        game.play(a)
        agent.update_root(game)
        out["games%d" % mv] = game.packed().copy()
    torch.cuda.synchronize()
    if path:
        np.savez(path, **out)
    return out


def test_search_with_one_launch_is_the_search_with_two(tmp_path):
    path = str(tmp_path / "two_kernels.npz")
    env = dict(os.environ, TM_VALUENET_FUSED="0")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_fused_valuenet as T; T._search(%r)" % (ROOT, os.path.dirname(__file__), path)
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT, timeout=120)
    ref, got = np.load(path), _search()
    assert sorted(ref.files) == sorted(got)
    for k in ref.files:
        assert ref[k].tobytes() == got[k].tobytes(), k
    _no_error()
