"""Re-analysis on the device (csrc/tree.hip: tm_pool_fresh; csrc/episodes.hip: tm_episode_rerecord; tetris_mcts_amd/reanalyse.py;
reanalyse.py): a store made fresh is a new store to an agent, a re-analysed row is a function of its position and not of its
slot, batch or place in the input, the kernel is its numpy statement, and a position that is not its row's is refused.

One recording (play.py --save --save_positions, 8 games x 20 simulations x 12 moves under Model_VV(seed=0)) serves every test."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G8, SIMS = 8, 20
SEARCHED = ("value", "variance", "child_stats", "policy")
KEPT = ("episode", "cycle", "slot", "move", "action", "combo", "lines", "score", "line_stats", "board")


def _checkpoint(d, seed):
    from tetris_mcts_amd.model import Model_VV
    Model_VV(backend="hip", seed=seed).save(os.path.join(str(d), "pytorch_model", "model_checkpoint"), verbose=False)


def _run_play(tmp_path, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "play.py"), "--agent_type", "ValueSim", "--n_games", "8", "--mcts_sims", "20",
                        "--max_moves", "12", "--save", "--save_dir", str(tmp_path) + "/"] + list(flags),
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """(directory, PositionLoader) of the one recorded run"""
    from tetris_mcts_amd.episodes import PositionLoader
    d = tmp_path_factory.mktemp("recording")
    _checkpoint(d, 0)
    _run_play(d, "--cycle", "3", "--save_positions")
    return d, PositionLoader(str(d) + "/data3")


def _tetris(n_games=G8, seed=100):
    from tetris_mcts_amd.pyTetris import Tetris
    return Tetris((20, 10), 1, 0, 0, seed=seed, n_games=n_games)


def _agent(name="ValueSim", n_games=G8, max_nodes=4096, seed=0, sims=SIMS):
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.pyTetris import Tetris
    return getattr(agents, name)(sims=sims, env=Tetris, env_args=((20, 10), 1, 0, 0), n_games=n_games, max_nodes=max_nodes, online=False,
                                 model=Model_VV(backend="hip", seed=seed))


def _raw(rows):
    return np.ascontiguousarray(rows).view(np.uint8).reshape(len(rows), rows.dtype.itemsize)


def _take(table, idx):
    """the rows idx of a table, pad bytes included"""
    return _raw(table)[np.asarray(idx)].copy().view(table.dtype).reshape(-1)


def _by_key(rows):
    return {(int(r["cycle"]), int(r["episode"]), int(r["move"])): _raw(rows)[i].tobytes() for i, r in enumerate(rows)}


def _moves(agent, game, n):
    out = []
    for _ in range(n):
        act = np.atleast_1d(agent.play()).copy()
        stats = agent.get_stats().reshape(game.n_games, 3, 7)
        game.play(act)
        agent.update_root(game)
        if np.atleast_1d(game.end).any():
            game.reset("ended")
            agent.update_root(game)
        out.append((act.tobytes(), stats.tobytes(), game.packed().tobytes(), game._ls.cpu().numpy().tobytes()))
    return out


def test_a_store_made_fresh_is_a_new_store():
    from tetris_mcts_amd.store import GS
    game = _tetris()
    start = (game.games.clone(), game._ls.clone())
    agent = _agent()
    new_store = {k: t.clone() for k, t in agent.store.t.items() if t is not None}
    rng0 = agent.store.t["gs"][:, GS["RNG_POS"]].clone()
    agent.update_root(game)
    _moves(agent, game, 6)
    assert bool((agent.store.t["gs"][:, GS["RNG_POS"]] != rng0).any()), "check_low drew from rand(): the stream is part of the test"
    assert bool((agent.store.t["rng"] != new_store["rng"]).any())
    agent.store.pool_fresh()
    for k, t in new_store.items():
        same = agent.store.t[k].cpu().numpy().tobytes() == t.cpu().numpy().tobytes()          # (bytes: the tables of constants hold NaN)
        assert same or k in ("env_game", "env_line_stats"), "tm_pool_fresh leaves %s as the moves left it" % k
    assert agent.store.s.eval_parity == 0
    game.games.copy_(start[0])
    game._ls.copy_(start[1])
    game._host = None
    agent.update_root(game)
    after = _moves(agent, game, 3)
    other_game = _tetris()
    other = _agent()
    other.update_root(other_game)
    want = _moves(other, other_game, 3)
    for m, (x, y) in enumerate(zip(after, want)):
        for what, p, q in zip(("actions", "statistics", "games", "line statistics"), x, y):
            assert p == q, ("move", m, what)
    assert len(want[0][1]) == G8 * 84
    assert int(agent.store.errors().abs().sum().item()) == 0


def test_the_first_move_is_the_recording_and_every_row_keeps_what_is_kept(recording):
    """under the recording's agent, simulations, weights and pool the rows of the run's first move - whose trees were empty too -
    come back in all 368 bytes; every other row keeps its copied and recomputed columns, and its statistics are those of a newly
    built agent on an environment that holds the same positions"""
    from tetris_mcts_amd.reanalyse import reanalyse_rows
    d, L = recording
    assert L.length == G8 * 12 and (L.rows["move"][:G8] == 0).all()
    game, agent = _tetris(seed=7), _agent(max_nodes=100000)
    new = reanalyse_rows(agent, game, L.rows, L.positions)
    assert new.dtype == L.rows.dtype and len(new) == L.length
    assert _raw(new)[:G8].tobytes() == _raw(L.rows)[:G8].tobytes()
    for c in KEPT:
        assert new[c].tobytes() == L.rows[c].tobytes(), c
    assert _raw(new)[:, 365:].tobytes() == _raw(L.rows)[:, 365:].tobytes()
    # a later move's batch against a new agent on the same positions
    lo = 5 * G8
    env = _tetris(seed=999)
    env.games.copy_(torch.from_numpy(np.ascontiguousarray(L.positions["game"][lo:lo + G8]).view(np.int32)))
    env._ls.copy_(torch.from_numpy(np.ascontiguousarray(L.positions["line_stats"][lo:lo + G8])))
    env._host = None
    fresh = _agent(max_nodes=100000)
    fresh.update_root(env)
    fresh.play()
    value, variance = fresh.get_value_and_variance()
    assert new["child_stats"][lo:lo + G8].tobytes() == fresh.get_stats().tobytes()
    assert new["value"][lo:lo + G8].tobytes() == value.tobytes() and new["variance"][lo:lo + G8].tobytes() == variance.tobytes()
    assert not np.array_equal(new["value"][G8:], L.rows["value"][G8:]), "the recorded trees of later moves were not empty"


@pytest.mark.parametrize("name", ["ValueSim", "ValueSimLP", "ValueSimC"])
def test_a_row_does_not_depend_on_order_slot_or_batch(recording, name):
    from tetris_mcts_amd.reanalyse import reanalyse_rows
    d, L = recording
    n = L.length
    base = _by_key(reanalyse_rows(_agent(name), _tetris(seed=1), L.rows, L.positions))
    assert len(base) == n
    perm = np.random.default_rng(5).permutation(n)
    shuffled = reanalyse_rows(_agent(name), _tetris(seed=2), _take(L.rows, perm), _take(L.positions, perm))
    assert shuffled["move"].tolist() == L.rows["move"][perm].tolist(), "the output is in the order of the input"
    # batches of 5: ragged against the 8 slots of a move, a last batch of 2 (97 rows), and row 3 again at the end, in another batch
    idx = np.concatenate([perm[::-1], [perm[-4]]])
    fives = reanalyse_rows(_agent(name, n_games=5), _tetris(n_games=5, seed=3), _take(L.rows, idx), _take(L.positions, idx))
    assert len(fives) == n + 1 and _raw(fives)[-1].tobytes() == _raw(fives)[3].tobytes()
    for run in (_by_key(shuffled), _by_key(fives)):
        assert run.keys() == base.keys()
        for k in base:
            assert run[k] == base[k], (name, k)


@pytest.mark.parametrize("name", ["ValueSim", "ValueSimLP", "ValueSimC"])
def test_the_pool_size_does_not_show(recording, name):
    """the default pool (the bound of the expansion rule plus the marking threshold) against 4096 nodes, for every agent offered: a
    pool the bound does not cover would raise the tree's error flag (reanalyse_rows raises), one that shows would change bytes"""
    from tetris_mcts_amd.reanalyse import default_max_nodes, reanalyse_rows
    d, L = recording
    assert 7 * (SIMS + 1) + 2 + 256 <= default_max_nodes(SIMS) < 4096
    rows, pos = L.rows[:3 * G8], L.positions[:3 * G8]
    a = reanalyse_rows(_agent(name, max_nodes=4096), _tetris(), rows, pos)
    b = reanalyse_rows(_agent(name, max_nodes=default_max_nodes(SIMS)), _tetris(), rows, pos)
    assert _raw(a).tobytes() == _raw(b).tobytes()


def _rerecord(game, agent, old, n, fault0=(0x7FFFFFFF, 0)):
    """tm_episode_rerecord with guard bands around the rows: (rows, fault)"""
    from tetris_mcts_amd import _lib
    GUARD = 256
    d_old = torch.from_numpy(_raw(old).reshape(-1).copy()).cuda()
    buf = torch.full((GUARD + n * 368 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    fault = torch.tensor(list(fault0) + [77, 77], dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().tm_episode_rerecord(C.byref(game.s), C.byref(agent.store.s), C.c_void_p(agent.store.stats_buf.data_ptr()),
                                              C.c_void_p(d_old.data_ptr()), n, C.c_void_p(buf.data_ptr() + GUARD),
                                              C.c_void_p(fault.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "tm_episode_rerecord")
    got, f = buf.cpu().numpy(), fault.cpu().numpy()
    assert (got[:GUARD] == 0xA5).all() and (got[-GUARD:] == 0xA5).all() and f[2:].tolist() == [77, 77], "nothing outside the outputs"
    return got[GUARD:-GUARD].copy().view(old.dtype), f[:2].tolist()


def test_the_kernel_is_its_numpy_statement_and_the_guard_names_the_first_bad_row(recording):
    from tetris_mcts_amd.reanalyse import NO_FAULT, Reanalyser, rerecord_numpy
    d, L = recording
    lo, n = 4 * G8 + 1, 5                                   # five rows in eight slots: a ragged workgroup, unused slots
    rows, pos = _take(L.rows, range(lo, lo + n)), _take(L.positions, range(lo, lo + n))
    game, agent = _tetris(seed=11), _agent()
    R = Reanalyser(agent, game)
    R.submit(rows, pos)
    first = R.collect()
    stats = agent.store.stats_buf.cpu().numpy()[:n]
    value, variance = agent.get_value_and_variance()
    want, fault = rerecord_numpy(rows, pos, stats, value[:n], variance[:n])
    assert fault is None and _raw(first).tobytes() == _raw(want).tobytes()
    got, f = _rerecord(game, agent, rows, n)
    assert _raw(got).tobytes() == _raw(want).tobytes() and f == [NO_FAULT, 0]
    assert (got["child_stats"][:, 0].sum(axis=1) > 0).all() and np.isfinite(got["policy"]).all()

    def flipped(edit):
        bad = _take(rows, range(n))
        edit(bad)
        return bad
    score = flipped(lambda r: r["score"].__setitem__(2, r["score"][2] ^ 1))
    board = flipped(lambda r: r["board"].__setitem__((3, 19, 0), r["board"][3, 19, 0] ^ 1))
    stat = flipped(lambda r: r["line_stats"].__setitem__((1, 2), r["line_stats"][1, 2] ^ 4))
    both = flipped(lambda r: (r["board"].__setitem__((4, 0, 0), 1), r["line_stats"].__setitem__((4, 0), 9), r["score"].__setitem__(2, -1)))
    for bad, (row, group, count) in ((score, (2, 0, 1)), (board, (3, 2, 1)), (stat, (1, 1, 1)), (both, (2, 0, 2))):
        got, f = _rerecord(game, agent, bad, n)
        assert f == [4 * row + group, count], (row, group, f)
        assert rerecord_numpy(bad, pos, stats, value[:n], variance[:n])[1] == (row, group, count)
    # n = 0 launches nothing; n beyond the environment and a NULL are refused before any HIP call
    from tetris_mcts_amd import _lib
    lib, p = _lib.lib(), C.c_void_p(agent.store.stats_buf.data_ptr())
    assert lib.tm_episode_rerecord(C.byref(game.s), C.byref(agent.store.s), p, p, 0, p, p, None) == 0
    assert lib.tm_episode_rerecord(C.byref(game.s), C.byref(agent.store.s), p, p, G8 + 1, p, p, None) == 1
    assert lib.tm_episode_rerecord(C.byref(game.s), C.byref(agent.store.s), p, p, 1, p, None, None) == 1


def _copy_recording(d, to, edit_rows=None, edit_positions=None):
    """the recording's shards in another directory, one table edited"""
    os.makedirs(to, exist_ok=True)
    for f in os.listdir(d):
        if not f.endswith(".npy"):
            continue
        t = np.load(os.path.join(str(d), f))
        raw = _raw(t).copy().view(t.dtype).reshape(-1) if len(t) else t
        if f.startswith("data3.part") and edit_rows:
            edit_rows(raw)
        if f.startswith("positions3.part") and edit_positions:
            edit_positions(raw)
        np.save(os.path.join(to, f), raw)


@pytest.mark.parametrize("what", ["score", "board", "line_stats", "piece"])
def test_a_position_that_is_not_its_rows_is_refused_and_nothing_is_written(recording, tmp_path, what):
    from tetris_mcts_amd.reanalyse import reanalyse_files
    d, L = recording
    D, R = str(tmp_path / "D"), str(tmp_path / "R")
    at = 2 * G8 + 3                                          # in the third batch of eight: row 3 of it
    edits = dict(score=dict(edit_positions=lambda p: p["game"].__setitem__((at, 14), p["game"][at, 14] ^ 1)),
                 board=dict(edit_positions=lambda p: p["game"].__setitem__((at, 9), p["game"][at, 9] ^ (1 << 16))),
                 line_stats=dict(edit_positions=lambda p: p["line_stats"].__setitem__((at, 0), p["line_stats"][at, 0] ^ 1)),
                 piece=dict(edit_positions=lambda p: p["game"].__setitem__((at, 10), (p["game"][at, 10] & ~np.uint32(0xFF)) | np.uint32(9))))
    _copy_recording(d, D, **edits[what])
    with pytest.raises(ValueError) as e:
        reanalyse_files([D + "/data3"], R, _agent(), _tetris(seed=21))
    msg = str(e.value)
    words = dict(score=("row 3", "combo, lines or score"), board=("row 3", "board"), line_stats=("row 3", "line_stats"),
                 piece=("row 3", "piece > 6", "nothing was loaded"))[what]
    assert all(w in msg for w in words) and "data3.part00000.npy" in msg, msg
    assert not [f for f in os.listdir(R) if f.endswith(".npy")], "no output file"


def test_other_weights_change_the_values_and_train_reads_the_result(recording, tmp_path):
    from tetris_mcts_amd.episodes import EpisodeLoader
    d, L = recording
    _checkpoint(tmp_path, 1)
    R = str(tmp_path / "R")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "reanalyse.py"), "--data_paths", str(d) + "/data3", "--out_dir", R,
                        "--agent_type", "ValueSim", "--mcts_sims", str(SIMS), "--n_games", "8", "--max_nodes", "4096"],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(R)) == sorted(f for f in os.listdir(d) if f.startswith("data3."))
    for f in os.listdir(R):
        if ".episodes." in f:
            assert open(os.path.join(R, f), "rb").read() == open(os.path.join(str(d), f), "rb").read()
    new = EpisodeLoader(R + "/data3", by_episode=False)
    assert new.length == L.length and len(new.episodes) == len(EpisodeLoader(str(d) + "/data3").episodes)
    for c in KEPT:
        assert new.rows[c].tobytes() == L.rows[c].tobytes(), c
    assert (new.rows["value"] != L.rows["value"]).mean() > 0.5
    assert np.isfinite(new.rows["policy"]).all() and (new.rows["child_stats"][:, 0].sum(axis=1) > 0).all()
    ck = tmp_path / "pytorch_model" / "model_checkpoint"
    before = ck.read_bytes()
    import glob
    t = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--td", "--td_lambda", "0.9", "--max_iters", "20", "--batch_size", "32",
                        "--data_paths"] + sorted(glob.glob(R + "/data*")), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert t.returncode == 0, t.stderr[-2000:]
    assert ck.read_bytes() != before, "train.py wrote a checkpoint"
