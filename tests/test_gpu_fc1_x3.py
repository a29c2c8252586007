"""The split-precision fc1 of the value net (Model_VV("hip_bf16x3", fc1="bf16x3"): valuenet_fc1_x3.inc, k_vn_conv_x3 + k_vn_fc1_x3) on
the GPU: the 1e-4 output contract against the reference's outputs and an fp64 forward; the layer alone against fp64 on the very a3
the kernel read, beside k_vn_fc1's fp32 chain; outputs that depend on the state only (batch, position, tile shape, launch, garbage
in the scratch, the request path); the hand-off over many launches; the native search loop against the oracle replaying the same
evaluator; re-preparation after a fit; refusals and defaults.

The figures of the layer test (both errors against fp64, their ratio) are printed before the assertion: run with -s."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {"ValueSim": 0, "ValueSimLP": 1}
OFF_F1W, OFF_F1B = 18816, 477568


def _tol(P):
    """(v, var) tolerance, scaled as tests/test_gpu_valuenet.py scales it"""
    return TOL * max(1.0, float(P[478338]) / 100.0), TOL * max(1.0, float(P[478339]) / 1000.0)


def _model(params=None, fc1="bf16x3", backend="hip_bf16x3", ck=None):
    from tetris_mcts_amd.model import Model_VV
    m = Model_VV(backend=backend, fc1=fc1) if fc1 is not None else Model_VV(backend=backend)
    if params is not None:
        m.set_flat_params(params)
    if ck is not None:
        m.load(ck, verbose=False)
    return m


def _f64(model, states):
    """fp64 torch forward of the model's weights: (v, var)"""
    import torch
    net = copy.deepcopy(model.model).double()
    with torch.no_grad():
        out = net(states.reshape(-1, 1, 20, 10).double())
    return out[:, 0], out[:, 1]


def _layer(model, states):
    """(v, var, a3, h) of one forward: a3 and h read from the scratch rows the kernels wrote"""
    n = states.shape[0]
    v, r = [t.clone() for t in model.inference_device(states)]
    return v, r, model._scratch[:n, :1792].clone(), model._scratch[:n, 1792:2048].clone()


def _check_layer(mf, mx, states, what):
    """fc1 alone: both models' convolutions give the same a3 bits; fc1 in fp64 from that a3; the split fc1's error within twice
    the fp32 chain's plus four fp32 ulps of the largest hidden unit.  Returns the figures."""
    import torch
    vx, rx, ax, hx = _layer(mx, states)
    vf, rf, af, hf = _layer(mf, states)
    assert torch.equal(ax.view(torch.int32), af.view(torch.int32)), what
    P = mx.flat_params().double()
    W, b = P[OFF_F1W:OFF_F1W + 256 * 1792].reshape(256, 1792), P[OFF_F1B:OFF_F1B + 256]
    h64 = torch.relu(ax.double() @ W.T + b)
    ex, ef, top = (hx.double() - h64).abs().max().item(), (hf.double() - h64).abs().max().item(), h64.abs().max().item()
    print("fc1 alone %s: x3 %.3e fp32 chain %.3e max|h| %.3e ratio %.3f" % (what, ex, ef, top, ex / max(ef, 1e-300)))
    assert ex <= 2 * ef + 4 * 2.0 ** -24 * top, (what, ex, ef, top)
    return (vx, rx), (vf, rf)


def _check_outputs(mf, mx, states, ref, tol, what):
    """item 1: outputs within tol of the reference and of the fp64 forward (and item 2's rule on the layer)"""
    (vx, rx), _ = _check_layer(mf, mx, states, what)
    v64, r64 = _f64(mx, states)
    assert (vx.double() - ref[:, 0]).abs().max().item() <= tol[0], what
    assert (rx.double() - ref[:, 1]).abs().max().item() <= tol[1], what
    ev, er = (vx.double() - v64).abs().max().item(), (rx.double() - r64).abs().max().item()
    assert ev <= tol[0] and er <= tol[1], (what, ev, er)


@pytest.fixture(scope="module")
def fixture_z(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_valuenet.npz"))


@pytest.mark.parametrize("pk,ok", [("params", "out"), ("params2", "out2")])
def test_fc1_x3_within_tolerance_of_the_reference(fixture_z, pk, ok):
    import torch
    z = fixture_z
    mf, mx = _model(z[pk], fc1="fp32"), _model(z[pk])
    base = torch.from_numpy(z["states"].reshape(-1, 200)).cuda()
    ref = torch.from_numpy(z[ok]).cuda().double()
    tol = _tol(z[pk])
    for B in (1, 7, 33, 64):
        _check_outputs(mf, mx, base[:B].contiguous(), ref[:B], tol, (pk, B))
    g = torch.Generator(device="cuda").manual_seed(5)
    for B in (4001, 9001):      # 32-state tiles, more items than the grid: the item loop; 64-state tiles; both ragged
        idx = torch.randint(0, 64, (B,), device="cuda", generator=g)
        _check_outputs(mf, mx, base[idx].contiguous(), ref[idx], tol, (pk, B))


def test_fc1_x3_r06_checkpoint_on_searched_states():
    """the committed r06 checkpoint on the states a short real search asked for (at most 2 000 of them): the layer's error rule
    alone, no absolute tolerance"""
    import torch
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.pyTetris import Tetris
    ck = os.path.join(ROOT, "tetris_mcts_amd", "checkpoints", "value_net_online_r06.pt")
    mf, mx = _model(fc1="fp32", ck=ck), _model(ck=ck)
    seen = []

    def ev(states):
        seen.append(states.clone())
        return mf.inference_device(states)
    env_args = ((20, 10), 1, 0, 0)
    game = Tetris(*env_args, seed=3, n_games=64)
    agent = agents.ValueSimLP(sims=8, env=Tetris, env_args=env_args, n_games=64, max_nodes=20000, evaluator=ev, online=False)
    agent.update_root(game)
    for _ in range(4):
        act = agent.play()
        game.play(act)
        agent.update_root(game)
    states = torch.cat(seen)
    states = states[(states != 0).any(dim=1)][:2000].contiguous()
    assert states.shape[0] > 1000
    _check_layer(mf, mx, states, "r06")


@pytest.mark.parametrize("pk", ["params", "params2"])
@pytest.mark.parametrize("n", [64, 9001])
def test_fc1_x3_layer_alone(fixture_z, pk, n):
    import torch
    z = fixture_z
    mf, mx = _model(z[pk], fc1="fp32"), _model(z[pk])
    base = torch.from_numpy(z["states"].reshape(-1, 200)).cuda()
    idx = torch.arange(n, device="cuda") % 64 if n == 64 else torch.randint(0, 64, (n,), device="cuda",
                                                                              generator=torch.Generator(device="cuda").manual_seed(7))
    _check_layer(mf, mx, base[idx].contiguous(), (pk, n))


def test_fc1_x3_outputs_depend_on_the_state_only(fixture_z):
    """batch and position invariance across both tile shapes, launch-to-launch bits over garbage in the scratch, the request
    path"""
    import torch
    z = fixture_z
    m = _model(z["params2"])
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


def test_fc1_x3_hand_off_over_many_launches(fixture_z):
    """300 launches each of 9 001 and 4 001 ragged states, every launch's bits compared on the device with the first launch's,
    one host read at the end"""
    import torch
    z = fixture_z
    m = _model(z["params2"])
    base = torch.from_numpy(z["states"].reshape(-1, 200)).cuda()
    g = torch.Generator(device="cuda").manual_seed(11)
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    for n in (9001, 4001):
        states = base[torch.randint(0, 64, (n,), device="cuda", generator=g)].contiguous()
        v0, r0 = [t.clone() for t in m.inference_device(states)]
        v, r = torch.empty_like(v0), torch.empty_like(r0)
        for _ in range(300):
            m.inference_device(states, v, r)
            bad += (v.view(torch.int32) != v0.view(torch.int32)).sum() + (r.view(torch.int32) != r0.view(torch.int32)).sum()
    assert int(bad.item()) == 0


def _replay(oracle, params, name, G, sims, max_nodes, seed, moves):
    """The native loop with fc1 x3 against the oracle agent whose evaluator callable is a second model of the same
    configuration"""
    import torch
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.pyTetris import Tetris
    model, evm = _model(params), _model(params)

    def ev(states):
        v, var = evm.inference_device(torch.from_numpy(states.reshape(-1, 200)).cuda())
        return v.cpu().numpy(), var.cpu().numpy()
    env_args = ((20, 10), 1, 0, 0)
    game = Tetris(*env_args, seed=seed, n_games=G)
    agent = getattr(agents, name)(sims=sims, env=Tetris, env_args=env_args, n_games=G, max_nodes=max_nodes, model=model,
                                  online=False)
    agent.update_root(game)
    assert agent.search_model() is agent.model and agent.model.fc1 == "bf16x3"
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
    assert agent.store.counter("N_EXPAND") == sum(o.n_expand for o in oa)


@pytest.mark.parametrize("name,sims,max_nodes", [("ValueSim", 40, 3000), ("ValueSimLP", 30, 3000)])
def test_native_loop_with_fc1_x3_replays_in_the_oracle(oracle, fixture_z, name, sims, max_nodes):
    _replay(oracle, fixture_z["params"], name, G=4, sims=sims, max_nodes=max_nodes, seed=41, moves=40)


def test_fc1_x3_planes_follow_a_fit(fixture_z, tmp_path, monkeypatch):
    import torch
    monkeypatch.chdir(tmp_path)              # (train_data writes its checkpoint under ./pytorch_model/)
    z = fixture_z
    m = _model(z["params"])
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
    fresh = _model(m.flat_params().cpu())
    v2, r2 = fresh.inference_device(states)
    assert torch.equal(v1, v2) and torch.equal(r1, r2)


def test_fc1_refusals_and_defaults(fixture_z):
    import abi_shape
    import torch
    from tetris_mcts_amd import _lib, store as st
    from tetris_mcts_amd.model import Model_VV
    for backend in ("hip", "torch"):
        with pytest.raises(ValueError):
            Model_VV(backend=backend, fc1="bf16x3")
    with pytest.raises(ValueError):
        Model_VV(backend="hip_bf16x3", fc1="bf16")
    z = fixture_z
    states = torch.from_numpy(z["states"].reshape(-1, 200)).cuda()
    for backend in ("hip", "hip_bf16x3"):
        a, b = _model(z["params2"], fc1="fp32", backend=backend), _model(z["params2"], fc1=None, backend=backend)
        (va, ra), (vb, rb) = a.inference_device(states), b.inference_device(states)
        assert torch.equal(va, vb) and torch.equal(ra, rb), backend
    # (the split fc1 is another function of the state than the fp32 chain: some bits differ)
    vx, rx = _model(z["params2"]).inference_device(states)
    assert not (torch.equal(vx, vb) and torch.equal(rx, rb))
    L = _lib.lib()
    for kind, kw, dist in ((st.KIND_VALUESIM, {}, False), (st.KIND_DIST, dict(dist_bins=50, dist_range=(0.0, 5000.0)), True)):
        s = st.TreeStore(4, 1000, kind=kind, **kw)
        h = C.c_void_p()
        _lib.check(L.tm_search_create(C.byref(h), C.byref(s.s), 1, 0), "tm_search_create")
        try:
            abi_shape.check_setter(L, h, dist)
        finally:
            L.tm_search_destroy(h)
