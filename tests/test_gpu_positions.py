"""Position records on the device (csrc/episodes.hip: tm_episode_record_positions; episodes.EpisodeRecorder.record_positions;
play.py --save --save_positions): every position row is the game its State row was made from - to the oracle engine, which renders
it to the row's board and steps it to the next row's game - and the State shards do not change by a byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_play(tmp_path, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "play.py"), "--agent_type", "ValueSim", "--n_games", "8", "--mcts_sims", "20",
                        "--max_moves", "12", "--save", "--save_dir", str(tmp_path) + "/"] + list(flags),
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _oracle_game(packed, line_stats=None):
    from oracle import binding as B
    og = B.Game(1, 0, 0, 0)
    og.g.view(np.uint32)[:] = packed
    if line_stats is not None:
        og.line_stats[:] = line_stats
    return og


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """one run with --save_positions, and the same command without"""
    a, b = tmp_path_factory.mktemp("with_positions"), tmp_path_factory.mktemp("without")
    from tetris_mcts_amd.model import Model_VV
    for d in (a, b):               # (the weights both runs load: without a checkpoint an agent draws its own)
        Model_VV(backend="hip", seed=0).save(str(d / "pytorch_model" / "model_checkpoint"), verbose=False)
    _run_play(a, "--cycle", "2", "--save_positions")
    _run_play(b, "--cycle", "2")
    return a, b


def test_every_position_is_the_game_of_its_row(runs):
    from tetris_mcts_amd.episodes import IDENTITY, PositionLoader
    L = PositionLoader(str(runs[0]) + "/data2")
    assert L.length == 8 * 12 and L.positions.dtype.itemsize == 96
    f = L.positions
    for c in IDENTITY:
        assert (L.rows[c] == f[c]).all(), c
    for i in range(L.length):
        row, g = L.rows[i], f["game"][i]
        assert row["board"].tobytes() == _oracle_game(g).getState().tobytes(), i
        assert int(row["score"]) == int(g[14].view(np.int32)) and int(row["lines"]) == int(g[15].view(np.int32)), i
        assert int(row["combo"]) == int(np.uint16(g[11] >> 16).view(np.int16)), i
        assert row["line_stats"].tolist() == f["line_stats"][i].tolist(), i
        assert not (g[11] >> 8) & 1, "no row of a game that has ended"


def test_the_recorded_action_steps_a_position_to_the_next(runs):
    """within an episode the oracle engine, stepping position m with the action the row recorded, arrives at position m + 1"""
    from tetris_mcts_amd.episodes import PositionLoader
    L = PositionLoader(str(runs[0]) + "/data2")
    order = np.lexsort((L.rows["move"], L.rows["episode"]))
    stepped = 0
    for i, j in zip(order[:-1], order[1:]):
        if L.rows["episode"][i] != L.rows["episode"][j]:
            continue
        assert L.rows["move"][j] == L.rows["move"][i] + 1
        og = _oracle_game(L.positions["game"][i], L.positions["line_stats"][i])
        og.play(int(L.rows["action"][i]))
        assert og.g.view(np.uint32).tobytes() == L.positions["game"][j].tobytes(), (i, j)
        assert og.line_stats.tobytes() == L.positions["line_stats"][j].tobytes(), (i, j)
        stepped += 1
    assert stepped >= 8 * 11 - 16


def test_the_state_shards_do_not_change_by_a_byte(runs):
    names = lambda d: sorted(f for f in os.listdir(d) if f.endswith(".npy"))  # noqa: E731
    with_p, without = names(runs[0]), names(runs[1])
    assert [f for f in with_p if not f.startswith("positions")] == without and without
    assert [f for f in with_p if f.startswith("positions")] == [f.replace("data", "positions", 1) for f in without if ".episodes." not in f]
    for f in without:
        assert open(os.path.join(runs[0], f), "rb").read() == open(os.path.join(runs[1], f), "rb").read(), f


@pytest.mark.parametrize("G", [1, 5, 64])
def test_the_kernel_against_a_numpy_statement(G):
    """G x 24 dwords by workgroups of 256 threads: G = 1 and 5 end inside the first workgroup, 64 fills six; ended games among
    them; guard bands on both sides of the rows"""
    from tetris_mcts_amd import _lib
    from tetris_mcts_amd.pyTetris import Tetris
    game = Tetris((20, 10), 1, 0, 0, seed=50, n_games=G)
    rng = np.random.default_rng(G)
    for _ in range(7):
        game.play(rng.integers(0, 7, size=G).astype(np.int32))
    ended = np.zeros(G, bool)
    ended[::3] = G > 1
    if G == 1:
        ended_cases = (False, True)
    else:
        ended_cases = (None,)
    for case in ended_cases:
        if case is not None:
            ended[:] = case
        packed = game.packed().copy()
        packed[ended, 11] |= 1 << 8                       # (only ever recorded: nothing steps or searches these bytes)
        game.games.copy_(torch.from_numpy(packed.view(np.int32)))
        ls = rng.integers(0, 50, size=(G, 4)).astype(np.int32)
        game._ls.copy_(torch.from_numpy(ls))
        slot_state = rng.integers(0, 10 ** 6, size=(G, 4)).astype(np.int32)
        d_ss = torch.from_numpy(slot_state).cuda()
        GUARD = 64
        buf = torch.full((GUARD + G * 24 + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib().tm_episode_record_positions(C.byref(game.s), C.c_void_p(d_ss.data_ptr()), 9,
                                                          C.c_void_p(buf.data_ptr() + 4 * GUARD),
                                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "tm_episode_record_positions")
        got = buf.cpu().numpy()
        assert (got[:GUARD] == 0x5A5A5A5A).all() and (got[-GUARD:] == 0x5A5A5A5A).all(), "nothing outside the rows"
        assert d_ss.cpu().numpy().tobytes() == slot_state.tobytes(), "slot_state is read only"
        want = np.zeros((G, 24), np.uint32)
        want[:, 0], want[:, 1], want[:, 2], want[:, 3] = slot_state[:, 0], 9, np.arange(G), slot_state[:, 1]
        want[:, 4:20], want[:, 20:24] = packed, ls
        want[ended] = 0
        want[ended, 0] = 0xFFFFFFFF
        assert got[GUARD:-GUARD].view(np.uint32).reshape(G, 24).tolist() == want.tolist(), (G, case)


def test_the_call_refuses_bad_arguments_before_any_hip_call():
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    buf = (C.c_char * 512)()
    b = (C.addressof(buf) + 15) // 16 * 16
    s = _lib.TmStore()
    s.n_games, s.env_game, s.env_line_stats = 2, b, b
    assert lib.tm_episode_record_positions(C.byref(s), None, 0, b, None) == 1
    assert lib.tm_episode_record_positions(C.byref(s), b, 0, None, None) == 1
    assert lib.tm_episode_record_positions(C.byref(s), b, 0, b + 2, None) == 1
    s.n_games = 0
    assert lib.tm_episode_record_positions(C.byref(s), b, 0, b, None) == 1
