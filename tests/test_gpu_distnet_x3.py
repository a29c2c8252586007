"""The split-precision backend of the distributional head ("hip_bf16x3": distnet_x3.inc, k_dn_conv_x3 + k_dn_fc) on the GPU: the
1e-6 relative contract against the reference's own Net, fp32-level accuracy of the split conv2 against an fp64 forward, batch
invariance and launch-to-launch bits, the request path, the native search loop against the oracle replaying the same
evaluator, re-preparation after a weight change, and the search handle's backend switch."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KEYS = ["seq__conv1__weight", "seq__conv1__bias", "seq__conv2__weight", "seq__conv2__bias", "seq__fc1__weight",
        "seq__fc1__bias", "seq__fc_v__weight", "seq__fc_v__bias"]


def _ref(golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_distnet.npz"))
    return g, np.concatenate([g[k].ravel() for k in KEYS]).astype(np.float32)


def _model(backend, params=None, atoms=50, seed=None):
    from tetris_mcts_amd.model_distributional import Model_Dist
    m = Model_Dist(atoms=atoms, backend=backend, seed=seed)
    if params is not None:
        m.set_flat_params(params)
    return m


def _boards(n, seed):
    import torch
    rng = np.random.default_rng(seed)
    st = rng.integers(-1, 2, size=(n, 200)).astype(np.int8)
    st[: n // 2, :100] = 0                    # half of them with an empty upper half, like real boards
    return torch.from_numpy(st).cuda()


def _f64(model, states):
    """fp64 torch forward of the model's weights: the distribution [n, atoms] and conv2's LeakyReLU'd output a2 [n, 2048]"""
    import torch
    net = copy.deepcopy(model.model).double()
    n = states.shape[0]
    x = torch.zeros(n, 1, 22, 10, dtype=torch.float64, device=states.device)
    x[:, 0, 2:, :] = states.reshape(n, 20, 10).double()
    with torch.no_grad():
        return net(x), net.seq[:4](x).reshape(n, -1)


def _check_accuracy(m32, mx3, states, what):
    """mx3's distribution and conv2 output (read from the scratch rows) within 2x the fp32 HIP head's error against the fp64
    forward, plus a floor of a few fp32 ulps (for states the fp32 path happens to round right)"""
    n, a = states.shape[0], mx3.atoms
    p32 = m32.inference_device(states)[:, :a].double()
    a32 = m32._scratch[:n, :2048].double()
    px = mx3.inference_device(states)[:, :a].double()
    ax = mx3._scratch[:n, :2048].double()
    p64, a64 = _f64(mx3, states)
    ep, ep32 = (px - p64).abs().max().item(), (p32 - p64).abs().max().item()
    ea, ea32 = (ax - a64).abs().max().item(), (a32 - a64).abs().max().item()
    assert ep <= 2 * ep32 + 4 * p64.abs().max().item() * 2.0 ** -24, (what, ep, ep32)
    assert ea <= 2 * ea32 + 4 * a64.abs().max().item() * 2.0 ** -24, (what, ea, ea32)
    return px


def test_x3_within_tolerance_of_the_reference(golden_dir):
    import torch
    g, P = _ref(golden_dir)
    m32, mx3 = _model("hip", P), _model("hip_bf16x3", P)
    x = g["x"]
    st = torch.from_numpy(np.ascontiguousarray(x[:, 0, 2:, :].reshape(16, 200).astype(np.int8))).cuda()
    y = mx3.inference_device(st)[:, :50].cpu().numpy()
    # the head's contract, as the fp32 head is held (tests/test_gpu_dist_agent.py)
    assert np.abs(y - g["y"]).max() <= 1e-6 * np.abs(g["y"]).max() and np.all(np.abs(y - g["y"]) <= 1e-6 * g["y"] + 1e-9)
    assert np.array_equal(mx3.inference(x)[0], y)                  # the reference's signature takes the same kernels
    _check_accuracy(m32, mx3, st, "fixture")
    for n in (1, 16, 1003, 4096):
        _check_accuracy(m32, mx3, _boards(n, n), n)
    # other numbers of atoms go through the same kernels
    for atoms in (7, 64):
        m32, mx3 = _model("hip", atoms=atoms, seed=atoms), _model("hip_bf16x3", atoms=atoms, seed=atoms)
        px = _check_accuracy(m32, mx3, _boards(40, atoms), atoms)
        assert torch.allclose(px.sum(1), torch.ones(40, dtype=torch.float64, device="cuda"), atol=1e-5)
        assert float(mx3.inference_device(_boards(40, atoms))[:, atoms:].abs().sum()) == 0.0


def test_x3_outputs_depend_on_the_state_only(golden_dir):
    """batch invariance, position invariance, launch-to-launch bits, garbage in the scratch"""
    import torch
    _, P = _ref(golden_dir)
    m = _model("hip_bf16x3", P)
    st = _boards(1003, 7)
    ref = m.inference_device(st).clone()
    for i in (0, 1, 500, 1002):
        assert torch.equal(m.inference_device(st[i:i + 1].contiguous())[0], ref[i]), i
    perm = torch.randperm(1003, device="cuda")
    assert torch.equal(m.inference_device(st[perm].contiguous()), ref[perm])
    for lo, n in ((5, 7), (100, 33), (400, 600)):
        assert torch.equal(m.inference_device(st[lo:lo + n].contiguous()), ref[lo:lo + n]), (lo, n)
    m._scratch.view(torch.int32).random_(-2**31, 2**31 - 1)
    assert torch.equal(m.inference_device(st), ref)
    assert torch.equal(m.inference_device(st), ref)


def test_x3_request_path_equals_the_dense_path(golden_dir):
    """tm_distnet_forward_requests under TM_VALUENET_BF16X3 over a store's pending requests (nodes rendered inside k_dn_conv_x3) =
    tm_distnet_forward under it on the same boards from render_eval(), bit for bit; slots without a request are left untouched"""
    import torch
    from tetris_mcts_amd import agents, store as st
    from tetris_mcts_amd.pyTetris import Tetris
    _, P = _ref(golden_dir)
    m = _model("hip_bf16x3", P)
    env_args = ((20, 10), 1, 0, 0)
    G = 40
    game = Tetris(*env_args, seed=31, n_games=G)
    agent = agents.DistValueSim(sims=12, env=Tetris, env_args=env_args, n_games=G, max_nodes=4000, model=m)
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
    s.t["eval_dist"].fill_(float("nan"))
    m.inference_requests(s)
    dense = m.inference_device(states)
    assert torch.equal(s.t["eval_dist"][used, :50], dense[used, :50])
    assert torch.isnan(s.t["eval_dist"][~used]).all() and torch.isnan(s.t["eval_dist"][:, 50:]).all()


def _compare_dist_trees(oracle, agent, oa, max_nodes, bins=50):
    """every reachable node's statistics and its `bins` atoms, bit for bit (tests/test_gpu_dist_agent.py)"""
    import torch
    s = agent.store
    assert (s.errors() == 0).all()
    gs = s.t["gs"].cpu().numpy()
    for g, o in enumerate(oa):
        stat = s.t["obs_stat"][g].view(torch.float32).cpu().numpy()         # [N, 4] = visit, mean, variance, M2
        dist = s.t["node_dist"][g].cpu().numpy()
        assert o.error == 0 and gs[g, 0] == o.root and gs[g, 8] == o.n_sims and gs[g, 7] == o.n_expand, (g, gs[g, :10])
        assert gs[g, 9] == o.n_gc
        ns, nd = o.dist_arrays()
        mark = np.zeros(max_nodes, np.uint8)
        oracle.lib().orc_get_all_childs(o.root, oracle.ptr(o.arrays()["child"]), max_nodes, oracle.ptr(mark))
        occ = np.nonzero(mark)[0]
        occ = occ[occ != 0]
        assert stat[occ][:, [0, 1, 2, 3]].tobytes() == np.ascontiguousarray(ns[occ][:, [0, 1, 3, 4]]).tobytes(), g
        assert nd.shape[1] == bins
        assert dist[occ, :bins].tobytes() == np.ascontiguousarray(nd[occ]).tobytes(), g
        assert np.all(dist[occ, bins:] == 0)


def _native_loop_replay(oracle, atoms, vmin, vmax, G, sims, max_nodes, moves):
    import torch
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.pyTetris import Tetris
    env_args = ((20, 10), 1, 0, 0)
    seeds = 919 + np.arange(G)
    model = _model("hip_bf16x3", atoms=atoms, seed=0)
    evm = _model("hip_bf16x3", model.flat_params().cpu(), atoms=atoms)

    def ev(states):
        return evm.inference_device(torch.from_numpy(states.reshape(-1, 200)).cuda())[:, :atoms].cpu().numpy()
    game = Tetris(*env_args, seed=seeds, n_games=G)
    agent = agents.DistValueSim(atoms=atoms, vmin=vmin, vmax=vmax, sims=sims, env=Tetris, env_args=env_args, n_games=G,
                                max_nodes=max_nodes, model=model)
    assert agent.search_model() is model
    agent.update_root(game)
    og = [oracle.Game(seed=int(s)) for s in seeds]
    oa = [oracle.Agent(6, max_nodes=max_nodes, low=5, evaluator=ev, dist_bins=atoms, dist_vmin=vmin, dist_vmax=vmax) for _ in range(G)]
    for g in range(G):
        oa[g].update_root(og[g])
    for m in range(moves):
        act = np.atleast_1d(agent.play())
        stats = agent.get_stats().reshape(G, 3, 7)
        for g in range(G):
            a = oa[g].play(sims)
            assert oa[g].error == 0
            assert a == act[g], ("action", m, g, a, act[g])
            assert oa[g].stats().tobytes() == stats[g].tobytes(), ("stats", m, g)
            og[g].play(a)
            oa[g].update_root(og[g])
        game.play(act)
        agent.update_root(game)
        ended = np.atleast_1d(game.end)
        if ended.any():
            game.reset("ended")
            agent.update_root(game)
            for g in np.nonzero(ended)[0]:
                og[g].reset()
                oa[g].update_root(og[g])
    _compare_dist_trees(oracle, agent, oa, max_nodes, bins=atoms)
    assert agent.store.search_stats(1, 0)["runs"] == moves             # the native loop ran the moves
    assert agent.store.counter("N_GC") > 0


def test_native_loop_on_x3_replays_in_the_oracle(oracle):
    """DistValueSim on "hip_bf16x3" inside the native launch loop (tm_search_run, TM_VALUENET_BF16X3) against oracle kind 6
    whose evaluator callable runs a second "hip_bf16x3" head on the same weights: actions, root statistics, every reachable
    node's statistics and distribution, through garbage collections"""
    _native_loop_replay(oracle, 50, 0.0, 5000.0, G=6, sims=150, max_nodes=3000, moves=12)


def test_native_loop_on_x3_replays_in_the_oracle_at_64_atoms(oracle):
    """the same at 64 atoms over [0, 32) (the regime `full_wave` of tests/dist_regimes.py): the split-precision head's request
    path indexes its parameter blob with the store's atom count, and the backup's shifts are whole-bin, most of them past the top"""
    _native_loop_replay(oracle, 64, 0.0, 32.0, G=6, sims=60, max_nodes=1200, moves=6)


def test_x3_planes_follow_weight_changes(golden_dir, tmp_path, monkeypatch):
    import torch
    monkeypatch.chdir(tmp_path)              # (train_data may write under the working directory)
    g, P = _ref(golden_dir)
    m = _model("hip_bf16x3", P)
    st = _boards(64, 3)
    d0 = m.inference_device(st).clone()
    P2 = P + np.random.default_rng(1).standard_normal(P.size).astype(np.float32) * 1e-3
    m.set_flat_params(P2)
    d1 = m.inference_device(st).clone()
    assert not torch.equal(d1, d0)
    assert torch.equal(d1, _model("hip_bf16x3", P2).inference_device(st))
    # a short fit (the online leg's train_data): the planes are re-prepared from the new weights
    gen = torch.Generator().manual_seed(3)
    n = 256
    x = torch.zeros(n, 1, 22, 10)
    x[:, 0, 2:, :] = torch.randint(-1, 2, (n, 20, 10), generator=gen).float()
    target = torch.softmax(torch.randn(n, 50, generator=gen), 1)
    m.train_data([x, target, torch.ones(n, 1)], batch_size=64, iters_per_val=4, max_iters=8, log=False)
    d2 = m.inference_device(st).clone()
    assert not torch.equal(d2, d1)
    assert torch.equal(d2, _model("hip_bf16x3", m.flat_params().cpu()).inference_device(st))


def test_search_handle_takes_the_backend_on_a_dist_store():
    import abi_shape
    from tetris_mcts_amd import _lib, store as st
    s = st.TreeStore(4, 1000, kind=st.KIND_DIST, dist_bins=50, dist_range=(0.0, 5000.0))
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.tm_search_create(C.byref(h), C.byref(s.s), 1, 0), "tm_search_create")
    try:
        abi_shape.check_setter(L, h, dist=True)
    finally:
        L.tm_search_destroy(h)
