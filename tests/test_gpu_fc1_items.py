"""k_vn_fc1's grid of work items on the GPU (valuenet.hip; the dealing itself: tests/test_fc1_items.py).  The matrix-core forward
against the plain one-thread-per-output forward, bit for bit, at sizes around every edge of the dealing - one state, partial last
tiles, both tile shapes (32 states below 8 192 rows, 64 from there on), fewer items than the resident grid and more (workgroups that
take a second and third item) - with garbage in the scratch; and through the request list, where the kernel reads the number of
requests itself: a short ValueSim and a short ValueSimLP search against the oracle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SIZES = (1, 31, 32, 33, 63, 64, 65, 1867, 2048, 4095, 4096, 8191, 8192, 8193)
KIND = {"ValueSim": 0, "ValueSimLP": 1}


@pytest.mark.parametrize("n", SIZES)
def test_forward_is_the_plain_forward_bit_for_bit(golden_dir, n):
    import torch
    from tetris_mcts_amd.model import Model_VV
    params = np.load(os.path.join(golden_dir, "ref_valuenet.npz"))["params"]
    m, plain = Model_VV(backend="hip"), Model_VV(backend="hip_plain")
    m.set_flat_params(params)
    plain.set_flat_params(params)
    g = torch.Generator(device="cuda").manual_seed(1000 + n)
    states = (torch.randint(0, 3, (n, 200), device="cuda", generator=g) - 1).to(torch.int8)
    pv, pr = [t.clone() for t in plain.inference_device(states)]
    m.inference_device(states)                       # (allocates the scratch)
    for _ in range(2):
        m._scratch.view(torch.int32).random_(-2**31, 2**31 - 1)
        v = torch.full((n,), float("nan"), device="cuda")
        r = torch.full((n,), float("nan"), device="cuda")
        m.inference_device(states, v, r)
        assert torch.equal(v.view(torch.int32), pv.view(torch.int32)), (n, (v - pv).abs().max().item())
        assert torch.equal(r.view(torch.int32), pr.view(torch.int32)), (n, (r - pr).abs().max().item())
    # the kernel leaves its tiles' arrival counters at zero (the first pad word of every tile's first scratch row)
    tile = 64 if n >= 8192 else 32
    assert int(m._scratch[:n:tile, 2048].view(torch.int32).abs().sum().item()) == 0


@pytest.mark.parametrize("name,G,sims,moves", [("ValueSim", 40, 30, 6), ("ValueSimLP", 40, 12, 5)])
def test_request_list_search_replays_in_the_oracle(oracle, golden_dir, name, G, sims, moves):
    """the request path: 40 games make one or two ragged tiles of requests a launch (ValueSim), a handful for ValueSimLP's seven
    slots a game - every action and every root statistic of every game against the oracle's own value net"""
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.pyTetris import Tetris
    params = np.load(os.path.join(golden_dir, "ref_valuenet.npz"))["params"]
    model = Model_VV(backend="hip")
    model.set_flat_params(params)
    env_args = ((20, 10), 1, 0, 0)
    game = Tetris(*env_args, seed=61, n_games=G)
    agent = getattr(agents, name)(sims=sims, env=Tetris, env_args=env_args, n_games=G, max_nodes=20000, model=model, online=False)
    agent.update_root(game)
    og = [oracle.Game(1, 0, 0, 61 + g) for g in range(G)]
    oa = [oracle.Agent(KIND[name], max_nodes=20000, evaluator="valuenet", params=params) for _ in range(G)]
    for g in range(G):
        oa[g].update_root(og[g])
    for mv in range(moves):
        act = np.atleast_1d(agent.play())
        stats = agent.get_stats()
        for g in range(G):
            a = oa[g].play(sims)
            assert a == act[g], (name, "move", mv, "game", g, a, act[g])
            assert oa[g].stats().tobytes() == stats[g].tobytes(), (name, "stats", mv, g)
            og[g].play(a)
            oa[g].update_root(og[g])
        game.play(act)
        agent.update_root(game)
        assert [o.score for o in og] == list(np.atleast_1d(game.score))
