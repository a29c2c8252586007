"""Root-distribution records on the device (csrc/episodes.hip: tm_episode_record_root_dists; episodes.EpisodeRecorder.record_root_dists;
play.py --save_root_dists; reanalyse.py --agent_type DistValueSim --root_dists; train.py --head dist --td --bootstrap search): the
kernel is its numpy statement, a recorded row is the root's node_dist row, a re-analysed row - 368 + 272 bytes - is a function of
its position and not of its slot, batch or place in the input, and the fit reads what either wrote.  All comparisons are of bits.

One recording (play.py --agent_type DistValueSim --save --save_positions --save_root_dists, 8 games x 20 simulations x 12 moves under
Model_Dist(backend="hip", seed=0)) serves every test that needs one."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G8, SIMS = 8, 20
KEPT = ("episode", "cycle", "slot", "move", "action", "combo", "lines", "score", "line_stats", "board")


def _checkpoint(d, seed):
    from tetris_mcts_amd.model_distributional import Model_Dist
    Model_Dist(atoms=50, backend="hip", seed=seed).save(os.path.join(str(d), "pytorch_model", "model_checkpoint_dist"), verbose=False)


def _run_play(tmp_path, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "play.py"), "--agent_type", "DistValueSim", "--n_games", "8", "--mcts_sims", "20",
                        "--max_moves", "12", "--save", "--save_positions", "--save_dir", str(tmp_path) + "/"] + list(flags),
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(the run with --save_root_dists, the same command without, RootDistLoader of the first)"""
    from tetris_mcts_amd.episodes import RootDistLoader
    a, b = tmp_path_factory.mktemp("with_root_dists"), tmp_path_factory.mktemp("without")
    for d in (a, b):
        _checkpoint(d, 0)
    _run_play(a, "--cycle", "3", "--save_root_dists")
    _run_play(b, "--cycle", "3")
    return a, b, RootDistLoader(str(a) + "/data3")


def _tetris(n_games=G8, seed=100):
    from tetris_mcts_amd.pyTetris import Tetris
    return Tetris((20, 10), 1, 0, 0, seed=seed, n_games=n_games)


def _agent(n_games=G8, max_nodes=4096, seed=0, sims=SIMS, backend="hip"):
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.model_distributional import Model_Dist
    from tetris_mcts_amd.pyTetris import Tetris
    return agents.DistValueSim(sims=sims, env=Tetris, env_args=((20, 10), 1, 0, 0), n_games=n_games, max_nodes=max_nodes, online=False,
                               model=Model_Dist(atoms=50, backend=backend, seed=seed))


def _raw(rows):
    return np.ascontiguousarray(rows).view(np.uint8).reshape(len(rows), rows.dtype.itemsize)


def _take(table, idx):
    return _raw(table)[np.asarray(idx)].copy().view(table.dtype).reshape(-1)


def _by_key(rows, dists):
    """(cycle, episode, move) -> the 368 + 272 bytes of the row"""
    return {(int(r["cycle"]), int(r["episode"]), int(r["move"])): _raw(rows)[i].tobytes() + _raw(dists)[i].tobytes()
            for i, r in enumerate(rows)}


# ---- the kernel against its numpy statement ----
@pytest.mark.parametrize("atoms", [7, 50, 64])
def test_the_kernel_is_its_numpy_statement(atoms):
    """64 games x 64 nodes; a thread per dword of n x 68, so every wave stores parts of two rows: n = 1 ends inside the first wave, 5
    inside the second workgroup, 64 fills seventeen.  Random bit patterns (NaNs among them) in node_dist, roots set by hand - one
    past the pool, one negative -, ended rows among the State rows, guard bands on both sides and the rows beyond n untouched."""
    from tetris_mcts_amd import _lib
    from tetris_mcts_amd import store as st
    from tetris_mcts_amd.episodes import STATE_DTYPE, record_root_dists_numpy
    G = N = 64
    store = st.TreeStore(G, N, kind=st.KIND_DIST, dist_bins=atoms, low=5)
    rng = np.random.default_rng(atoms)
    bits = rng.integers(0, 2 ** 32, (G, N, 64), dtype=np.uint64).astype(np.uint32)
    bits[:, :, 3] = 0x7FC00000 | (bits[:, :, 3] & 0x3FFFFF)                    # a quiet NaN with a payload in every row
    bits[::2, :, 5] = 0xFF800001                                               # a signalling one
    store.t["node_dist"].copy_(torch.from_numpy(bits.view(np.int32)).view(torch.float32))
    roots = rng.integers(0, N, G).astype(np.int32)
    roots[2], roots[4], roots[63] = N, -1, N - 1
    store.t["gs"][:, st.GS["ROOT"]] = torch.from_numpy(roots).cuda()
    rows = np.zeros(G, STATE_DTYPE)
    rows["episode"], rows["cycle"], rows["slot"], rows["move"] = rng.integers(0, 10 ** 6, G), 9, np.arange(G), rng.integers(0, 500, G)
    rows["score"] = rng.integers(0, 10 ** 6, G)
    for g in (0, 3, 40):                                                       # ended games: -1, then zeros
        rows[g] = np.zeros((), STATE_DTYPE)
        rows["episode"][g] = -1
    d_rows = torch.from_numpy(_raw(rows).reshape(-1).copy()).cuda()
    node_dist = bits.view(np.float32)
    GUARD = 256
    for n in (1, 5, 64):
        buf = torch.full((GUARD + G * 272 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        _lib.check(_lib.lib().tm_episode_record_root_dists(C.byref(store.s), C.c_void_p(d_rows.data_ptr()), n,
                                                           C.c_void_p(buf.data_ptr() + GUARD),
                                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "tm_episode_record_root_dists")
        got = buf.cpu().numpy()
        assert (got[:GUARD] == 0xA5).all() and (got[-GUARD:] == 0xA5).all(), "nothing outside the rows"
        assert (got[GUARD + n * 272:-GUARD] == 0xA5).all(), "the rows beyond n are untouched"
        want = record_root_dists_numpy(rows[:n], roots, node_dist, atoms)
        assert got[GUARD:GUARD + n * 272].tobytes() == _raw(want).tobytes(), (atoms, n)
    assert store.t["node_dist"].cpu().numpy().view(np.uint32).tobytes() == bits.tobytes(), "node_dist is read only"
    assert d_rows.cpu().numpy().tobytes() == _raw(rows).tobytes(), "the State rows are read only"
    # n = 0 launches nothing; a tree of another kind, n beyond the store and a NULL are refused before any HIP call
    lib, p = _lib.lib(), C.c_void_p(d_rows.data_ptr())
    assert lib.tm_episode_record_root_dists(C.byref(store.s), p, 0, p, None) == 0
    assert lib.tm_episode_record_root_dists(C.byref(store.s), p, G + 1, p, None) == 1
    assert lib.tm_episode_record_root_dists(C.byref(store.s), p, 1, None, None) == 1
    other = st.TreeStore(2, 64)
    assert lib.tm_episode_record_root_dists(C.byref(other.s), p, 1, p, None) == 1


def test_the_refusals_on_the_device_too():
    import test_root_dists as H
    from tetris_mcts_amd import _lib
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    H.refused_root_dist_arguments(_lib.lib(), (t.data_ptr() + 15) // 16 * 16)


# ---- one recording ----
def test_the_dist_shard_pairs_with_the_data_shard_and_nothing_else_changes(runs):
    from tetris_mcts_amd.episodes import IDENTITY
    a, b, L = runs
    assert L.length == G8 * 12 and (L.atoms, L.vmin, L.vmax) == (50, 0.0, 5000.0) and L.dists.dtype.itemsize == 272
    for c in IDENTITY:
        assert (L.rows[c] == L.dists[c]).all() and (L.rows[c] == L.positions[c]).all(), c
    d = L.dists["dist"]
    assert np.isfinite(d).all() and (d >= 0).all() and not d[:, 50:].any() and (d[:, :50].sum(axis=1) > 0).all()
    names = lambda x: sorted(f for f in os.listdir(x) if f.endswith(".npy"))  # noqa: E731
    with_d, without = names(a), names(b)
    assert [f for f in with_d if not f.startswith("rootdist")] == without and without
    assert [f for f in with_d if f.startswith("rootdist")] == sorted(
        [f.replace("data", "rootdist", 1) for f in without if f.startswith("data") and ".episodes." not in f] + ["rootdist3.head.npy"])
    for f in without:                                       # data, episodes and positions: byte-equal files
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    assert any(f.startswith("positions3.part") for f in without) and any(f.startswith("data3.part") for f in without)


def test_a_recorded_row_is_the_roots_node_dist_row(tmp_path):
    """in-process, five moves into a ring of two: every flush path (full ring, both pinned buffers, the partial ring at close)"""
    from tetris_mcts_amd import store as st
    from tetris_mcts_amd.episodes import EpisodeRecorder, RootDistLoader
    game, agent = _tetris(), _agent()
    agent.update_root(game)
    rec = EpisodeRecorder(str(tmp_path) + "/", "data", 5, G8, ring_moves=2)
    rec.record_positions()
    rec.record_root_dists(agent.atoms, *agent.vrange)
    want = []
    for _ in range(5):
        action = agent.play()
        s = agent.store
        root = s.t["gs"][:, st.GS["ROOT"]].long()
        want.append(s.t["node_dist"][torch.arange(G8, device=root.device), root].cpu().numpy().copy())
        rec.add(agent, game)
        game.play(action)
        rec.advance(game)
        agent.update_root(game)
        assert not np.atleast_1d(game.end).any()
    rec.close()
    L = RootDistLoader(str(tmp_path) + "/data5")
    assert L.counts == [2 * G8, 2 * G8, G8] and L.length == 5 * G8 and hasattr(L, "positions")
    want = np.concatenate(want)
    assert want.shape == (5 * G8, 64) and L.dists["dist"].tobytes() == want.tobytes()
    assert (L.dists["slot"] == np.tile(np.arange(G8), 5)).all() and (L.dists["move"] == np.repeat(np.arange(5), G8)).all()
    value, _ = agent.get_value()                           # (of the last root: only that the rows are distributions the agent reads)
    assert np.isfinite(value).all() and (want[:, :50].sum(axis=1) > 0.99).all()
    # an agent whose tree keeps no distribution is refused
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.pyTetris import Tetris
    other = agents.ValueSim(sims=4, env=Tetris, env_args=((20, 10), 1, 0, 0), n_games=G8, max_nodes=512, online=False,
                            model=Model_VV(backend="hip", seed=0))
    other.update_root(game)
    rec2 = EpisodeRecorder(str(tmp_path / "v") + "/", "data", 5, G8, ring_moves=2)
    rec2.record_root_dists(50, 0, 5000)
    with pytest.raises(TypeError, match="distributional tree"):
        rec2.add(other, game)


# ---- re-analysis ----
def test_the_first_move_is_the_recording_and_every_row_keeps_what_is_kept(runs):
    from tetris_mcts_amd.reanalyse import reanalyse_rows
    a, b, L = runs
    assert (L.rows["move"][:G8] == 0).all()
    new, dists = reanalyse_rows(_agent(max_nodes=100000), _tetris(seed=7), L.rows, L.positions)
    assert new.dtype == L.rows.dtype and dists.dtype == L.dists.dtype and len(new) == len(dists) == L.length
    assert _raw(new)[:G8].tobytes() == _raw(L.rows)[:G8].tobytes() and _raw(dists)[:G8].tobytes() == _raw(L.dists)[:G8].tobytes()
    for c in KEPT:
        assert new[c].tobytes() == L.rows[c].tobytes(), c
    for c in ("episode", "cycle", "slot", "move"):
        assert dists[c].tobytes() == L.rows[c].tobytes(), c
    assert _raw(new)[:, 365:].tobytes() == _raw(L.rows)[:, 365:].tobytes()
    assert not np.array_equal(dists["dist"][G8:], L.dists["dist"][G8:]), "the recorded trees of later moves were not empty"
    assert not dists["dist"][:, 50:].any() and np.isfinite(dists["dist"]).all()


@pytest.mark.parametrize("backend", ["hip", "hip_bf16x3"])
def test_a_row_does_not_depend_on_order_slot_or_batch(runs, backend):
    from tetris_mcts_amd.reanalyse import reanalyse_rows
    a, b, L = runs
    n = L.length
    base = _by_key(*reanalyse_rows(_agent(backend=backend), _tetris(seed=1), L.rows, L.positions))
    assert len(base) == n and all(len(v) == 640 for v in base.values())
    perm = np.random.default_rng(5).permutation(n)
    shuffled = reanalyse_rows(_agent(backend=backend), _tetris(seed=2), _take(L.rows, perm), _take(L.positions, perm))
    assert shuffled[0]["move"].tolist() == L.rows["move"][perm].tolist(), "the output is in the order of the input"
    # batches of 5: ragged against the 8 slots of a move, a last batch of 2 (97 rows), and row 3 again at the end, in another batch
    idx = np.concatenate([perm[::-1], [perm[-4]]])
    fives = reanalyse_rows(_agent(n_games=5, backend=backend), _tetris(n_games=5, seed=3), _take(L.rows, idx), _take(L.positions, idx))
    assert len(fives[0]) == len(fives[1]) == n + 1
    assert _raw(fives[0])[-1].tobytes() == _raw(fives[0])[3].tobytes() and _raw(fives[1])[-1].tobytes() == _raw(fives[1])[3].tobytes()
    for run in (_by_key(*shuffled), _by_key(*fives)):
        assert run.keys() == base.keys()
        for k in base:
            assert run[k] == base[k], (backend, k)


def test_the_default_pool_does_not_show(runs):
    from tetris_mcts_amd.reanalyse import default_max_nodes, reanalyse_rows
    a, b, L = runs
    rows, pos = L.rows[:3 * G8], L.positions[:3 * G8]
    x = reanalyse_rows(_agent(max_nodes=4096), _tetris(), rows, pos)
    y = reanalyse_rows(_agent(max_nodes=default_max_nodes(SIMS)), _tetris(), rows, pos)
    assert _raw(x[0]).tobytes() == _raw(y[0]).tobytes() and _raw(x[1]).tobytes() == _raw(y[1]).tobytes()


def test_other_weights_change_the_distributions_and_no_kept_column(runs):
    from tetris_mcts_amd.reanalyse import reanalyse_rows
    a, b, L = runs
    new, dists = reanalyse_rows(_agent(seed=1), _tetris(seed=4), L.rows, L.positions)
    for c in KEPT:
        assert new[c].tobytes() == L.rows[c].tobytes(), c
    assert (dists["dist"][:, :50] != L.dists["dist"][:, :50]).any(axis=1).mean() > 0.5
    assert (new["value"] != L.rows["value"]).mean() > 0.5


def test_a_flipped_score_bit_is_refused_and_nothing_of_either_table_is_written(runs, tmp_path):
    from tetris_mcts_amd.reanalyse import reanalyse_files
    a, b, L = runs
    D, R = str(tmp_path / "D"), str(tmp_path / "R")
    os.makedirs(D)
    at = 2 * G8 + 3                                          # in the third batch of eight: row 3 of it
    for f in os.listdir(a):
        if not f.endswith(".npy"):
            continue
        t = np.load(os.path.join(str(a), f))
        if f.startswith("positions3.part"):
            t = _raw(t).copy().view(t.dtype).reshape(-1)
            t["game"][at, 14] ^= 1
        np.save(os.path.join(D, f), t)
    with pytest.raises(ValueError) as e:
        reanalyse_files([D + "/data3"], R, _agent(), _tetris(seed=21))
    msg = str(e.value)
    assert "row 3" in msg and "combo, lines or score" in msg and "data3.part00000.npy" in msg, msg
    assert not [f for f in os.listdir(R) if f.endswith(".npy")], "no output file of either table, no sidecar"


# ---- the route ----
def test_reanalyse_then_train_reads_the_result_as_a_recording(runs, tmp_path):
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.episodes import RootDistLoader
    from tetris_mcts_amd.model_distributional import Model_Dist
    a, b, L = runs
    _checkpoint(tmp_path, 1)
    R = str(tmp_path / "R")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "reanalyse.py"), "--data_paths", str(a) + "/data3", "--out_dir", R,
                        "--agent_type", "DistValueSim", "--root_dists", "--mcts_sims", str(SIMS), "--n_games", "8", "--max_nodes", "4096"],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(R)) == sorted(f for f in os.listdir(a) if f.startswith(("data3.", "rootdist3.")))
    assert open(os.path.join(R, "rootdist3.head.npy"), "rb").read() == open(os.path.join(str(a), "rootdist3.head.npy"), "rb").read()
    new = RootDistLoader(R + "/data3")
    assert new.length == L.length and new.position_files is None and (new.atoms, new.vmin, new.vmax) == (50, 0.0, 5000.0)
    for c in KEPT:
        assert new.rows[c].tobytes() == L.rows[c].tobytes(), c
    assert (new.dists["dist"] != L.dists["dist"]).any(axis=1).mean() > 0.5, "searched under the other seed's weights"
    from tetris_mcts_amd.reanalyse import reanalyse_rows
    want, want_d = reanalyse_rows(_agent(seed=1), _tetris(seed=9), L.rows, L.positions)
    assert _raw(new.rows).tobytes() == _raw(want).tobytes() and _raw(new.dists).tobytes() == _raw(want_d).tobytes()
    # train.py reads R as a recording
    ck = tmp_path / "pytorch_model" / "model_checkpoint_dist"
    before = ck.read_bytes()
    t = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--head", "dist", "--td", "--td_lambda", "0.9", "--bootstrap", "search",
                        "--max_iters", "20", "--batch_size", "32", "--data_paths"] + sorted(glob.glob(R + "/data*")),
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert t.returncode == 0, t.stderr[-2000:]
    assert "iters:20/20" in t.stdout and ck.read_bytes() != before, "train.py wrote model_checkpoint_dist"
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        from tetris_mcts_amd import agents
        from tetris_mcts_amd.pyTetris import Tetris
        fitted = Model_Dist(atoms=50, backend="hip", seed=5)
        fitted.load(verbose=False)
        game = _tetris(n_games=2, seed=5)
        agent = agents.DistValueSim(sims=20, env=Tetris, env_args=game.env_args, n_games=2, max_nodes=2000)
        assert torch.equal(agent.model.flat_params(), fitted.flat_params()), "a DistValueSim that builds its own model loads it"
        agent.update_root(game)
        assert np.atleast_1d(agent.play()).shape == (2,)
        # on the device: at lambda = 0 the targets handed to train_data are the recorded rows, on_round's p_rows the file's
        seen = []
        model = Model_Dist(atoms=50, backend="hip", seed=0)
        res = O.fit_episodes_dist(model, [R + "/data3"], td=True, bootstrap="search", max_iters=4, batch_size=32,
                                  on_round=lambda r, data, p: seen.append((r, [d.clone() for d in data], p.clone())))
        assert len(seen) == 1 and [x["iters"] for x in res["rounds"]] == [4]
        _, data, p = seen[0]
        assert p.is_cuda and p.cpu().numpy().tobytes() == new.dists["dist"].tobytes()
        table, stem_rows, eps, ep_stems = O.load_stems([R + "/data3"])
        order = O.episode_index(O.rows_tensor(table, "cuda"), stem_rows, eps, ep_stems).order.cpu().numpy()
        assert data[1].shape == (L.length, 50) and data[1].cpu().numpy().tobytes() == new.dists["dist"][order, :50].tobytes()
    finally:
        os.chdir(cwd)
