"""The split-precision value-net backend ("hip_bf16x3": valuenet_x3.inc, k_vn_conv_x3 + k_vn_fc1) on the GPU: the 1e-4 output
contract against the reference's own outputs and an fp64 forward, fp32-level accuracy of the split convolutions, batch
invariance and launch-to-launch bits, the request path, the native search loop against the oracle replaying the same
evaluator, and re-preparation after an online fit."""
import copy
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {"ValueSim": 0, "ValueSimLP": 1, "ValueSimC": 2}


def _tol(P):
    """(v, var) tolerance, scaled as tests/test_gpu_valuenet.py scales it"""
    return TOL * max(1.0, float(P[478338]) / 100.0), TOL * max(1.0, float(P[478339]) / 1000.0)


def _models(params):
    from tetris_mcts_amd.model import Model_VV
    out = []
    for b in ("hip", "hip_bf16x3"):
        m = Model_VV(backend=b)
        m.set_flat_params(params)
        out.append(m)
    return out


def _f64(model, states):
    """fp64 torch forward of the model's weights: (v, var) and conv3's output a3 [n, 1792] (channel-major)"""
    import torch
    net = copy.deepcopy(model.model).double()
    x = states.reshape(-1, 1, 20, 10).double()
    with torch.no_grad():
        out = net(x)
        a3 = net.head[:6](x).reshape(x.shape[0], -1)
    return out[:, 0], out[:, 1], a3


def _check_accuracy(m32, mx3, states, ref=None, tol=None, what=""):
    """mx3 within tol of ref (when given) and of the fp64 forward; its error, and that of its convolutions (a3, read from the
    scratch rows), within a small multiple of the fp32 HIP path's on the same states"""
    import torch
    n = states.shape[0]
    v32, r32 = [t.clone() for t in m32.inference_device(states)]
    a32 = m32._scratch[:n, :1792].double()
    vx, rx = [t.clone() for t in mx3.inference_device(states)]
    ax = mx3._scratch[:n, :1792].double()
    v64, r64, a64 = _f64(mx3, states)
    if ref is not None:
        assert (vx.double() - ref[:, 0]).abs().max().item() <= tol[0], what
        assert (rx.double() - ref[:, 1]).abs().max().item() <= tol[1], what
    ev, er = (vx.double() - v64).abs().max().item(), (rx.double() - r64).abs().max().item()
    e32v, e32r = (v32.double() - v64).abs().max().item(), (r32.double() - r64).abs().max().item()
    if tol is not None:
        assert ev <= tol[0] and er <= tol[1], (what, ev, er)
    # (+ a floor of a few fp32 ulps of the outputs, for states the fp32 path happens to round right)
    assert ev <= 2 * e32v + 4 * v64.abs().max().item() * 2.0 ** -24, (what, ev, e32v)
    assert er <= 2 * e32r + 4 * r64.abs().max().item() * 2.0 ** -24, (what, er, e32r)
    # the split convolutions as accurate as the fp32 fma chains (a dropped plane: 4-20x the fp32 path's error here)
    ea3, e32a3 = (ax - a64).abs().max().item(), (a32 - a64).abs().max().item()
    assert ea3 <= 2 * e32a3, (what, ea3, e32a3)
    return vx, rx


@pytest.mark.parametrize("pk,ok", [("params", "out"), ("params2", "out2")])
def test_x3_within_tolerance_of_the_reference(golden_dir, pk, ok):
    import torch
    z = np.load(os.path.join(golden_dir, "ref_valuenet.npz"))
    m32, mx3 = _models(z[pk])
    base = torch.from_numpy(z["states"].reshape(-1, 200)).cuda()
    ref = torch.from_numpy(z[ok]).cuda().double()
    tol = _tol(z[pk])
    for B in (1, 7, 33, 64):
        _check_accuracy(m32, mx3, base[:B].contiguous(), ref[:B], tol, (pk, B))
    g = torch.Generator(device="cuda").manual_seed(5)
    for B in (9001, 7169):          # 64-state fc1 tiles from 8192 states on, 32-state tiles below; ragged
        idx = torch.randint(0, 64, (B,), device="cuda", generator=g)
        _check_accuracy(m32, mx3, base[idx].contiguous(), ref[idx], tol, (pk, B))


def test_x3_outputs_depend_on_the_state_only(golden_dir):
    """batch invariance, position invariance, launch-to-launch bits, garbage in the scratch, the request path"""
    import torch
    z = np.load(os.path.join(golden_dir, "ref_valuenet.npz"))
    _, m = _models(z["params2"])
    base = torch.from_numpy(z["states"].reshape(-1, 200)).cuda()
    v0, r0 = [t.clone() for t in m.inference_device(base)]
    big = base.repeat(141, 1)
    perm = torch.randperm(big.shape[0], device="cuda")[:9001]
    vb, rb = [t.clone() for t in m.inference_device(big[perm].contiguous())]
    src = perm % 64
    assert torch.equal(vb, v0[src]) and torch.equal(rb, r0[src])
    for lo, n in ((0, 1), (5, 7), (100, 33), (4000, 4001)):
        vp, rp = m.inference_device(big[perm][lo:lo + n].contiguous())
        assert torch.equal(vp, vb[lo:lo + n]) and torch.equal(rp, rb[lo:lo + n]), (lo, n)
    for _ in range(3):
        m._scratch.view(torch.int32).random_(-2**31, 2**31 - 1)
        v, r = m.inference_device(big[perm].contiguous())
        assert torch.equal(v, vb) and torch.equal(r, rb)
    # the request path (observations rendered inside k_vn_conv_x3) = the dense-state path on the same rendered states
    from tetris_mcts_amd import agents, store as st
    from tetris_mcts_amd.pyTetris import Tetris
    env_args = ((20, 10), 1, 0, 0)
    for name in ("ValueSim", "ValueSimLP"):
        game = Tetris(*env_args, seed=31, n_games=40)
        agent = getattr(agents, name)(sims=12, env=Tetris, env_args=env_args, n_games=40, max_nodes=4000, model=m, online=False)
        agent.update_root(game)
        for _ in range(3):
            act = agent.play()
            game.play(act)
            agent.update_root(game)
        s = agent.store
        s.move_begin(4)
        s.sim_step(st.SIM_BACKUP | st.SIM_FRONT)
        states = s.render_eval().clone()
        used = s.t["eval_obs"] != 0
        assert int(used.sum()) > 0
        s.t["eval_v"].fill_(float("nan"))
        s.t["eval_var"].fill_(float("nan"))
        m.inference_requests(s)
        vd, rd = m.inference_device(states)
        assert torch.equal(s.t["eval_v"][used], vd[used]) and torch.equal(s.t["eval_var"][used], rd[used]), name


def test_x3_r06_checkpoint_on_searched_states():
    """the committed r06 checkpoint on the states a short real search asked for (render_eval of every launch)"""
    import torch
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.pyTetris import Tetris
    ck = os.path.join(ROOT, "tetris_mcts_amd", "checkpoints", "value_net_online_r06.pt")
    m32, mx3 = Model_VV(backend="hip"), Model_VV(backend="hip_bf16x3")
    m32.load(ck, verbose=False)
    mx3.load(ck, verbose=False)
    seen = []

    def ev(states):
        seen.append(states.clone())
        return m32.inference_device(states)
    env_args = ((20, 10), 1, 0, 0)
    game = Tetris(*env_args, seed=3, n_games=64)
    agent = agents.ValueSimLP(sims=8, env=Tetris, env_args=env_args, n_games=64, max_nodes=20000, evaluator=ev, online=False)
    agent.update_root(game)
    for _ in range(4):
        act = agent.play()
        game.play(act)
        agent.update_root(game)
    states = torch.cat(seen)
    states = states[(states != 0).any(dim=1)].contiguous()
    assert states.shape[0] > 1000
    _check_accuracy(m32, mx3, states, None, None, "r06")


def _replay(oracle, params, name, G, sims, max_nodes, seed, moves):
    """The native loop on "hip_bf16x3" against the oracle agent whose evaluator callable runs the same backend"""
    import torch
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.pyTetris import Tetris
    model, evm = Model_VV(backend="hip_bf16x3"), Model_VV(backend="hip_bf16x3")
    model.set_flat_params(params)
    evm.set_flat_params(params)

    def ev(states):
        v, var = evm.inference_device(torch.from_numpy(states.reshape(-1, 200)).cuda())
        return v.cpu().numpy(), var.cpu().numpy()
    env_args = ((20, 10), 1, 0, 0)
    game = Tetris(*env_args, seed=seed, n_games=G)
    agent = getattr(agents, name)(sims=sims, env=Tetris, env_args=env_args, n_games=G, max_nodes=max_nodes, model=model,
                                  online=False)
    agent.update_root(game)
    assert agent.search_model() is agent.model
    og = [oracle.Game(1, 0, 0, seed + g) for g in range(G)]
    oa = [oracle.Agent(KIND[name], max_nodes=max_nodes, evaluator=ev) for _ in range(G)]
    for g in range(G):
        oa[g].update_root(og[g])
    for m in range(moves):
        act = np.atleast_1d(agent.play())
        stats = agent.get_stats().reshape(G, 3, 7)
        for g in range(G):
            a = oa[g].play(sims)
            assert oa[g].error == 0
            assert a == act[g], (name, "move", m, "game", g, a, act[g])
            assert oa[g].stats().tobytes() == stats[g].tobytes(), (name, "stats", m, g)
            og[g].play(a)
            oa[g].update_root(og[g])
        game.play(act)
        agent.update_root(game)
        assert [o.score for o in og] == list(np.atleast_1d(game.score))
        ended = np.atleast_1d(game.end)
        if ended.any():
            game.reset("ended")
            for g in np.nonzero(ended)[0]:
                og[g].reset()
            agent.update_root(game)
            for g in np.nonzero(ended)[0]:
                oa[g].update_root(og[g])
    assert all(o.n_gc >= 1 for o in oa), [o.n_gc for o in oa]
    assert agent.store.counter("N_GC") == sum(o.n_gc for o in oa)
    assert agent.store.counter("N_EXPAND") == sum(o.n_expand for o in oa)


@pytest.mark.parametrize("name,sims,max_nodes", [("ValueSim", 40, 3000), ("ValueSimLP", 30, 3000), ("ValueSimC", 30, 3000)])
def test_native_loop_on_x3_replays_in_the_oracle(oracle, golden_dir, name, sims, max_nodes):
    params = np.load(os.path.join(golden_dir, "ref_valuenet.npz"))["params"]
    _replay(oracle, params, name, G=4, sims=sims, max_nodes=max_nodes, seed=41, moves=40)


def test_x3_planes_follow_an_online_fit(golden_dir, tmp_path, monkeypatch):
    import torch
    from tetris_mcts_amd.model import Model_VV
    monkeypatch.chdir(tmp_path)              # (train_data writes its checkpoint under ./pytorch_model/)
    z = np.load(os.path.join(golden_dir, "ref_valuenet.npz"))
    m = Model_VV(backend="hip_bf16x3")
    m.set_flat_params(z["params"])
    states = torch.from_numpy(z["states"].reshape(-1, 200)).cuda()
    v0, r0 = [t.clone() for t in m.inference_device(states)]
    epoch0 = m.weights_epoch
    g = torch.Generator().manual_seed(3)
    n = 512
    data = [torch.randint(-1, 2, (n, 1, 20, 10), generator=g).float(), torch.rand(n, 1, generator=g) * 50,
            torch.rand(n, 1, generator=g) * 100 + 1, torch.randint(1, 30, (n, 1), generator=g).float()]
    m.train_data(data, batch_size=64, iters_per_val=4, max_iters=8, log=False)
    assert m.weights_epoch != epoch0
    v1, r1 = [t.clone() for t in m.inference_device(states)]
    assert not torch.equal(v1, v0)
    fresh = Model_VV(backend="hip_bf16x3")
    fresh.set_flat_params(m.flat_params().cpu())
    v2, r2 = fresh.inference_device(states)
    assert torch.equal(v1, v2) and torch.equal(r1, r2)
