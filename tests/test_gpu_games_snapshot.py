"""Game snapshots on the device (csrc/games_snapshot.hip: tm_env_check, tm_env_save, tm_env_load, tm_episode_resume;
tetris_mcts_amd/games.py; play.py --games_in / --games_out / --games_every).

The check is held to games.check_games_numpy, game for game, on what the engine produces (no fault, ever) and on hand-edited
bytes (every class of fault, and combinations).  The bad bytes are only ever CHECKED: no test steps, renders or searches them -
the point is that the loader keeps them out of a store.  A loaded environment is then shown to be the environment: to the engine
(bit-equal games under the same actions), to an agent (bit-equal actions and statistics) and to the episode recorder (the rows of
a second play.py run continue the first run's)."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import games_snapshot_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G64 = 64


def _tetris(app=1, randomizer=0, seed=0, n_games=G64):
    from tetris_mcts_amd.pyTetris import Tetris
    return Tetris((20, 10), app, 0, randomizer, seed=seed, n_games=n_games)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_on_device(games, line_stats, app):
    """tm_env_check on host arrays: (fault [n], n_bad)"""
    from tetris_mcts_amd import _lib
    n = len(games)
    d_g = torch.from_numpy(np.ascontiguousarray(games, np.uint32).view(np.int32)).cuda()
    d_l = None if line_stats is None else torch.from_numpy(np.ascontiguousarray(line_stats, np.int32)).cuda()
    out = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().tm_env_check(_p(d_g), None if d_l is None else _p(d_l), n, app, _p(out),
                                       C.c_void_p(out.data_ptr() + 4 * n), _stream()), "tm_env_check")
    h = out.cpu().numpy()
    return h[:n], int(h[n])


def _bytes(game):
    return game.packed().tobytes(), game._ls.cpu().numpy().tobytes()


_played = {}


def _play_random(app, randomizer):
    """64 games, 300 actions each: random ones in the even slots, hard drops only in the odd slots (such a game ends every 10 or 11
    moves); a game that ends is LEFT ended for one move before it is reset.  Checked at every tenth move; returns the last state."""
    key = (app, randomizer)
    if key in _played:
        return _played[key]
    from tetris_mcts_amd import games as GM
    game = _tetris(app, randomizer, seed=31 + 100 * app + randomizer)
    rng = np.random.default_rng(1000 + 10 * app + randomizer)
    waited = np.zeros(G64, bool)
    ended_checked = 0
    for move in range(300):
        if move % 10 == 0 or (waited.any() and ended_checked < 8):       # (and the first few moves that find a game ended)
            games, ls = game.packed().copy(), game._ls.cpu().numpy()
            fault, n_bad = _check_on_device(games, ls, app)
            want = GM.check_games_numpy(games, ls, app)
            assert fault.tolist() == want.tolist(), (app, randomizer, move)
            assert n_bad == 0 and not fault.any(), (app, randomizer, move, np.nonzero(fault)[0], fault[fault != 0])
            ended_checked += int(((games[:, 11] >> 8) & 1).sum())
        a = rng.integers(0, 7, size=G64).astype(np.int32)
        a[1::2] = 3
        game.play(a)
        end = np.atleast_1d(game.end).astype(bool)
        game.reset(end & waited)
        waited = end & ~waited
    assert ended_checked > 0, "ended games were among the checked ones"
    _played[key] = (game.packed().copy(), game._ls.cpu().numpy().copy())
    return _played[key]


@pytest.mark.parametrize("app,randomizer", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_no_false_positives(app, randomizer):
    _play_random(app, randomizer)


def test_check_without_line_stats_and_odd_sizes():
    """n that is no multiple of the workgroup's 64 games or of the count's 256 threads, one game, and line_stats = NULL"""
    from tetris_mcts_amd import games as GM
    games, ls = _play_random(1, 0)
    big = np.concatenate([games] * 9)[:515]
    big_ls = np.concatenate([ls] * 9)[:515]
    bad, bad_ls, where = K.inject(big[:G64], big_ls[:G64], [g for g in range(G64) if not (big[g, 11] >> 8) & 1])
    big[300:300 + G64], big_ls[300:300 + G64] = bad, bad_ls
    for n in (1, 63, 65, 257, 515):
        for with_ls in (True, False):
            fault, n_bad = _check_on_device(big[-n:], big_ls[-n:] if with_ls else None, 1)
            want = GM.check_games_numpy(big[-n:], big_ls[-n:] if with_ls else None, 1)
            assert fault.tolist() == want.tolist() and n_bad == int(np.count_nonzero(want)), (n, with_ls)


def test_every_fault_class_is_caught_and_nothing_is_loaded(tmp_path):
    from tetris_mcts_amd import _lib
    from tetris_mcts_amd import games as GM
    games, ls = _play_random(1, 0)
    live = [g for g in range(G64) if not (games[g, 11] >> 8) & 1]
    assert len(live) >= len(K.INJECTIONS)
    bad, bad_ls, where = K.inject(games, ls, live[::-1])
    want = GM.check_games_numpy(bad, bad_ls, 1)
    for g, (name, bits) in where.items():
        assert int(want[g]) & bits == bits, (name, int(want[g]))
    assert set(np.nonzero(want)[0].tolist()) == set(where), "one bad game per injection, the others untouched"
    fault, n_bad = _check_on_device(bad, bad_ls, 1)
    assert fault.tolist() == want.tolist()
    assert n_bad == len(K.INJECTIONS) == int(np.count_nonzero(want))
    # tm_env_load: the same report, and not one byte of the store changes
    env = _tetris(1, 0, seed=777)
    env.play(np.full(G64, 3, np.int32))
    before = _bytes(env)
    d_g = torch.from_numpy(bad.view(np.int32)).cuda()
    d_l = torch.from_numpy(bad_ls).cuda()
    out = torch.full((G64 + 1,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().tm_env_load(C.byref(env.s), _p(d_g), _p(d_l), _p(out), C.c_void_p(out.data_ptr() + 4 * G64), _stream()),
               "tm_env_load")
    h = out.cpu().numpy()
    assert h[:G64].tolist() == want.tolist() and int(h[G64]) == len(K.INJECTIONS)
    assert _bytes(env) == before
    # one bad game among 64 is enough
    one = games.copy()
    K.set_piece(one[live[0]], piece=255, y=127)
    path = str(tmp_path / "one")
    GM.write_snapshot(path, GM._meta(env), one, ls, np.zeros(G64, np.int32))
    with pytest.raises(ValueError) as e:
        env.load_games(path)
    assert "slot %d " % live[0] in str(e.value) and "fault bits %d" % (K.PIECE | K.PLACE) in str(e.value) and path in str(e.value)
    assert _bytes(env) == before
    # load_games names the FIRST bad slot of many
    path = str(tmp_path / "bad")
    GM.write_snapshot(path, GM._meta(env), bad, bad_ls, np.zeros(G64, np.int32))
    with pytest.raises(ValueError) as e:
        env.load_games(path)
    first = min(where)
    assert "slot %d " % first in str(e.value) and "fault bits %d" % int(want[first]) in str(e.value)
    assert "%d of %d games" % (len(K.INJECTIONS), G64) in str(e.value)
    assert _bytes(env) == before
    # and the bytes the injections started from do load: the store holds them (ended games reset, as load_games says)
    path = str(tmp_path / "good")
    GM.write_snapshot(path, GM._meta(env), games, ls, np.arange(G64, dtype=np.int32))
    move = env.load_games(path)
    ended = ((games[:, 11] >> 8) & 1) != 0
    now, now_ls = env.packed(), env._ls.cpu().numpy()
    assert now[~ended].tobytes() == games[~ended].tobytes() and now_ls[~ended].tobytes() == ls[~ended].tobytes()
    assert move[~ended].tolist() == np.arange(G64)[~ended].tolist() and not move[ended].any()
    assert not ((now[:, 11] >> 8) & 1).any() and (now[ended, 12] == 1).all() and not now_ls[ended].any()


@pytest.mark.parametrize("app,randomizer", [(1, 0), (2, 1)])
def test_a_loaded_environment_is_the_environment(app, randomizer, tmp_path):
    a, b = _tetris(app, randomizer, seed=5), _tetris(app, randomizer, seed=900)
    rng = np.random.default_rng(77)
    stream = rng.integers(0, 7, size=(100, G64)).astype(np.int32)
    stream[:, 1::2] = 3                       # (the odd slots end and are reset along the way)
    moves = np.zeros(G64, np.int32)
    for m in range(40):
        a.play(stream[m])
        moves += 1
        end = np.atleast_1d(a.end)
        moves[end] = 0
        a.reset("ended")
    assert _bytes(a) != _bytes(b)
    path = str(tmp_path / "games")
    assert a.save_games(path, moves) == path
    got = b.load_games(path)
    assert got.dtype == np.int32 and got.tolist() == moves.tolist()
    assert _bytes(a) == _bytes(b)
    assert np.atleast_1d(b.score).tolist() == np.atleast_1d(a.score).tolist()        # (the cached host fields were dropped)
    for m in range(40, 100):
        a.play(stream[m])
        b.play(stream[m])
        assert _bytes(a) == _bytes(b), m
        if m % 7 == 0:
            a.reset("ended")
            b.reset("ended")
            assert _bytes(a) == _bytes(b), m


def test_saving_an_ended_game_and_loading_it_resets_it(tmp_path):
    a, b = _tetris(1, 0, seed=5, n_games=4), _tetris(1, 0, seed=60, n_games=4)
    drop = np.full(4, 3, np.int32)
    for m in range(40):
        a.play(drop)
        if np.atleast_1d(a.end).any():
            break
    end = np.atleast_1d(a.end).copy()
    assert end.any()
    path = str(tmp_path / "games")
    a.save_games(path, np.full(4, m + 1, np.int32))
    with np.load(path) as z:
        assert (((z["games"][:, 11] >> 8) & 1) != 0).tolist() == end.tolist(), "an ended game is stored ended"
        assert z["games"].tobytes() == a.packed().tobytes()
    move = b.load_games(path)
    a.reset("ended")
    assert _bytes(a) == _bytes(b) and move.tolist() == np.where(end, 0, m + 1).tolist()


def _agent(name, game):
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.pyTetris import Tetris
    kw = dict(random_seed=11) if name == "Vanilla" else dict(model=_model())
    agent = getattr(agents, name)(sims=30, env=Tetris, env_args=game.env_args, n_games=game.n_games, max_nodes=4096, online=False, **kw)
    agent.update_root(game)
    return agent


def _model():
    from tetris_mcts_amd.model import Model_VV
    return Model_VV(backend="hip", seed=0)


def _moves(agent, game, n):
    out = []
    for _ in range(n):
        act = np.atleast_1d(agent.play()).copy()
        stats = agent.get_stats().reshape(game.n_games, 3, 7)
        assert stats.dtype == np.float32
        game.play(act)
        agent.update_root(game)
        if np.atleast_1d(game.end).any():
            game.reset("ended")
            agent.update_root(game)
        out.append((act.tobytes(), stats.tobytes(), game.packed().tobytes(), game._ls.cpu().numpy().tobytes()))
    return out


@pytest.mark.parametrize("name", ["ValueSim", "Vanilla"])
def test_a_loaded_batch_is_indistinguishable_to_an_agent(name, tmp_path):
    G = 8
    game = _tetris(1, 0, seed=100, n_games=G)
    first = _agent(name, game)
    _moves(first, game, 10)
    first.close()
    path = str(tmp_path / "games")
    game.save_games(path, np.full(G, 10, np.int32))
    copy = _tetris(1, 0, seed=4242, n_games=G)
    copy.load_games(path)
    assert _bytes(copy) == _bytes(game)
    a = _agent(name, game)
    on_original = _moves(a, game, 6)
    a.close()
    b = _agent(name, copy)
    on_copy = _moves(b, copy, 6)
    b.close()
    for m, (x, y) in enumerate(zip(on_original, on_copy)):
        for what, p, q in zip(("actions", "statistics", "games", "line statistics"), x, y):
            assert p == q, (name, "move", m, what)
    assert len(on_original[0][1]) == G * 84


def _run_play(tmp_path, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "play.py"), "--agent_type", "ValueSim", "--n_games", "8", "--mcts_sims", "20",
                        "--max_moves", "12", "--save", "--save_dir", str(tmp_path) + "/"] + list(flags),
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _render(packed, reset=False):
    """the board of one packed game by the oracle engine; reset: of the game that game.reset() makes of it"""
    from oracle import binding as B
    og = B.Game(1, 0, 0, 0)
    og.g.view(np.uint32)[:] = packed
    if reset:
        og.reset()
    return og.getState()


def test_records_continue_across_two_runs(tmp_path):
    from tetris_mcts_amd.episodes import EpisodeLoader
    S = str(tmp_path / "games")
    _run_play(tmp_path, "--cycle", "1", "--games_out", S)
    with np.load(S) as z:
        games, move, ls = z["games"], z["move"], z["line_stats"]
    alive = ((games[:, 11] >> 8) & 1) == 0
    one = EpisodeLoader(str(tmp_path) + "/data1", by_episode=False)
    assert alive.any()
    for s in np.nonzero(alive)[0]:
        mine = one.rows[one.slot == s]
        # the slot's last row of cycle 1 is the move before the snapshot's count (or the game was reset after that row: count 0)
        assert int(move[s]) == (int(mine["move"][-1]) + 1 if int(mine["episode"][-1]) not in one.episodes["episode"].tolist() else 0)
    _run_play(tmp_path, "--cycle", "2", "--games_in", S, "--games_out", S)
    two = EpisodeLoader(str(tmp_path) + "/data2", by_episode=False)
    assert two.length > 0 and (two.cycle == 2).all()
    ended_ids = {int(e["episode"]): e for e in two.episodes}
    for s in range(8):
        mine = two.rows[two.slot == s]                      # file order: move by move
        assert len(mine) > 0
        r0 = mine[0]
        if alive[s]:
            assert int(r0["move"]) == int(move[s]), s
            assert r0["board"].tobytes() == _render(games[s]).tobytes(), s
            assert int(r0["score"]) == int(games[s, 14].view(np.int32)) and int(r0["lines"]) == int(games[s, 15].view(np.int32))
            assert r0["line_stats"].tolist() == ls[s].tolist()
        else:
            assert int(r0["move"]) == 0 and int(r0["score"]) == 0, s
            assert r0["board"].tobytes() == _render(games[s], reset=True).tobytes(), s
        for prev, cur in zip(mine[:-1], mine[1:]):
            if int(cur["episode"]) == int(prev["episode"]):
                assert int(cur["move"]) == int(prev["move"]) + 1, s
            else:
                assert int(cur["move"]) == 0 and int(prev["episode"]) in ended_ids, s
        for e in set(mine["episode"].tolist()) & set(ended_ids):
            rows = mine[mine["episode"] == e]
            assert int(ended_ids[e]["moves"]) == int(rows["move"][-1]) + 1, (s, e)
    with np.load(S) as z:
        move2, games2 = z["move"], z["games"]
    for s in range(8):
        mine = two.rows[two.slot == s]
        if not ((games2[s, 11] >> 8) & 1) and int(mine["episode"][-1]) not in ended_ids:
            assert int(move2[s]) == int(mine["move"][-1]) + 1, s
    never_ended = [s for s in range(8) if alive[s] and len(set(two.rows[two.slot == s]["episode"].tolist())) == 1
                   and not (games2[s, 11] >> 8) & 1]
    assert all(int(move2[s]) == int(move[s]) + 12 for s in never_ended)


def test_games_every_leaves_a_loadable_file_while_the_run_goes_on(tmp_path, monkeypatch, capsys):
    """play.py's own loop in this process, with the writer watched: at moves 5 and 10 of a 12-move run (and at its end) the file
    is whole, loads into an environment, and its move counts are the moves played so far"""
    from tetris_mcts_amd import games as GM
    spec_ = importlib.util.spec_from_file_location("tm_play_games_every", os.path.join(ROOT, "play.py"))
    cli = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(cli)
    S = str(tmp_path / "games")
    seen = []
    real = GM.write_snapshot

    def watched(path, meta, games, line_stats, move):
        out = real(path, meta, games, line_stats, move)
        probe = _tetris(1, 0, seed=999, n_games=4)
        got = probe.load_games(path)
        ended = ((np.asarray(games)[:, 11] >> 8) & 1) != 0
        assert probe.packed()[~ended].tobytes() == np.asarray(games)[~ended].tobytes()
        seen.append(got.copy())
        return out
    monkeypatch.setattr(GM, "write_snapshot", watched)
    cli.main(["--agent_type", "Vanilla", "--n_games", "4", "--mcts_sims", "8", "--max_moves", "12", "--games_out", S, "--games_every", "5"])
    capsys.readouterr()
    assert len(seen) == 3
    for k, move in zip((5, 10, 12), seen):
        assert move.max() == k and (move >= 0).all(), (k, move)       # a slot whose game ended on the way counts from there
    with np.load(S) as z:
        assert z["move"].tolist() == seen[-1].tolist()
