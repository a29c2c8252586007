"""The offline targets on the device (csrc/episode_targets.hip: tm_episode_targets, tm_episode_gather_states) against the numpy
statement of the same definitions (offline.targets_numpy) and, for the lambda-return, against the exact oracle of
episode_targets_cases.py with the derived bound of tests/test_offline.py: |value_i - exact_i| <= 2^-23 M_i.  Then the whole
route at small scale: recorded ValueSim episodes -> fit_episodes -> checkpoint -> train.py in a fresh process.

A bad `order` entry is a bounds check, not a provoked fault: the kernel compares the entry with n_rows before it forms an
address, and the test reads that nothing was read (zeros) and that the flag is set."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import episode_targets_cases as K
from test_gpu_episodes import FILL, Arena          # the guard bands of the recorder's tests
from test_offline import EPS, _bits, refused_arguments

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from tetris_mcts_amd import _lib
    return _lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows_dev(rows):
    from tetris_mcts_amd.offline import rows_tensor
    return rows_tensor(rows, "cuda")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _targets(rows_d, n_rows, order, seg, tail, mode, lam, wmode, n_seg=None):
    """the call into guarded arrays; (value, variance, weight, fault, return code), the fault word cleared before"""
    n = len(order)
    arena = Arena([4 * n, 4 * n, 4 * n, 4])
    o, f = arena.seg[3]
    arena.t[o:o + f] = 0
    keep = [_dev(np.asarray(order, np.int32)), _dev(np.asarray(seg, np.int32))] + [_dev(x) for x in tail]
    rc = _lib().tm_episode_targets(_p(rows_d), n_rows, _p(keep[0]), _p(keep[1]), len(seg) - 1 if n_seg is None else n_seg,
                                   _p(keep[2]), _p(keep[3]), _p(keep[4]), mode, lam, wmode, EPS, arena.ptr(0), arena.ptr(1),
                                   arena.ptr(2), arena.ptr(3), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    arena.check()
    return [arena.bytes(i).view(np.float32) for i in range(3)] + [int(arena.bytes(3).view(np.int32)[0]), rc]


_spec_cache = {}


def _spec(c, mode, lam, wmode):
    from tetris_mcts_amd import offline as O
    key = (id(c["rows"]), c["tail"][0].tobytes(), mode, lam)
    if key not in _spec_cache:
        _spec_cache[key] = O.targets_numpy(c["rows"], c["order"], c["seg"], *c["tail"], mode, lam, 0, EPS)
    value, variance, _, fault = _spec_cache[key]
    wkey = (id(c["rows"]), "w", wmode)
    if wkey not in _spec_cache:
        _spec_cache[wkey] = O.targets_numpy(c["rows"], c["order"], c["seg"], *c["tail"], 2, 0.0, wmode, EPS)[2]
    return value, variance, _spec_cache[wkey], fault


def _ulps(a, b):
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


@pytest.mark.parametrize("draw", ["pos", "mixed"])
@pytest.mark.parametrize("final", [True, False])
@pytest.mark.parametrize("presorted", [False, True])
def test_kernel_equals_the_numpy_statement(draw, final, presorted):
    """every mode x weight mode x lambda, with and without tails; `order` a permutation of file order (the real case) and the
    rows sorted beforehand (order = 0, 1, 2, ...)"""
    rows = K.case(draw, final, 0.0)["rows"]
    order = K.case(draw, final, 0.0)["order"]
    if presorted:
        rows_d, order_d = _rows_dev(rows[order]), np.arange(len(order), dtype=np.int32)
    else:
        rows_d, order_d = _rows_dev(rows), order
        assert (np.diff(order) != 1).any()
    worst_ulp = 0
    for mode, lams in ((0, (0.0,)), (2, (0.0,)), (1, K.LAMBDAS)):
        for lam in lams:
            c = K.case(draw, final, lam)
            for wmode in (0, 1, 2, 3):
                value, variance, weight, fault, rc = _targets(rows_d, len(rows), order_d, c["seg"], c["tail"], mode, lam, wmode)
                want = _spec(c, mode, lam, wmode)
                assert rc == 0 and fault == 0
                assert _bits(variance, want[1]) and _bits(weight, want[2]), (mode, lam, wmode)
                if mode != 1:
                    assert _bits(value, want[0]), (mode, wmode)
                    continue
                frac = c["exact"].bound_fraction(value) if wmode == 0 else None
                ulp = _ulps(value, want[0])
                worst_ulp = max(worst_ulp, ulp)
                if wmode == 0:
                    print("lambda-return %s final=%s presorted=%s lam=%s: %.3f of 2^-23 M; %d ulp from the numpy statement"
                          % (draw, final, presorted, lam, frac, ulp))
                    assert frac <= 1.0
                else:
                    assert _bits(value, first), "the weight mode does not touch the value"
                first = value
                if lam == 0.0:
                    assert _bits(value, rows["value"][order]), "lambda = 0 is v_i itself"
    print("largest difference from the numpy statement: %d ulp (expected 0 or 1)" % worst_ulp)


def _three_tables():
    from tetris_mcts_amd.episodes import STATE_DTYPE, EPISODE_DTYPE, _concat
    made = [K.make_table("pos", seed=k, cycle=K.CYCLE + k) for k in range(3)]
    rows, ep = _concat([m[0] for m in made], STATE_DTYPE), _concat([m[1] for m in made], EPISODE_DTYPE)
    order, seg = K.by_episode(rows)
    return rows, ep, order, seg


@pytest.mark.parametrize("n_seg", [1, 5, 37])
def test_nothing_else_is_written(n_seg):
    """guard bands around value, variance, weight and the fault word; the positions behind the last segment handed over keep
    the fill as well"""
    from tetris_mcts_amd import offline as O
    rows, ep, order, seg = _three_tables()
    assert len(seg) - 1 == 48
    tail = K.tails(rows, ep, order, seg)
    sub = seg[:n_seg + 1]
    got = _targets(_rows_dev(rows), len(rows), order, sub, [t[:n_seg] for t in tail], 1, 0.9, 3)
    want = O.targets_numpy(rows, order, sub, *[t[:n_seg] for t in tail], 1, 0.9, 3, EPS)
    end = int(sub[-1])
    assert got[4] == 0 and got[3] == 0
    for g, w in zip(got[:3], want[:3]):
        assert _ulps(g[:end], w[:end]) <= 1
        assert (g[end:].view(np.uint8) == FILL).all()
    assert _bits(got[1][:end], want[1][:end]) and _bits(got[2][:end], want[2][:end])


def test_nothing_to_do_launches_nothing():
    c = K.case("pos", True, 0.9)
    rows_d = _rows_dev(c["rows"])
    for kw in (dict(n_seg=0), dict(n_rows=0)):
        got = _targets(rows_d, kw.get("n_rows", len(c["rows"])), c["order"], c["seg"], c["tail"], 1, 0.9, 3, n_seg=kw.get("n_seg"))
        assert got[4] == 0 and got[3] == 0
        assert all((g.view(np.uint8) == FILL).all() for g in got[:3])


def test_a_bad_order_entry_reads_nothing():
    """one entry equal to n_rows and one equal to -1: zeros, weight 0 and fault == 1 at those positions only; the position is
    left out of its episode's series (the numpy statement says what that gives), every other episode and every copied column
    elsewhere is unchanged"""
    from tetris_mcts_amd import offline as O
    c = K.case("pos", True, 0.9)
    rows, n = c["rows"], len(c["rows"])
    rows_d = _rows_dev(rows)
    bad = [int(c["seg"][4]) + 100, int(c["seg"][7]) - 1]
    order = c["order"].copy()
    order[bad[0]], order[bad[1]] = n, -1
    others = np.ones(n, bool)
    others[bad] = False
    touched = others.copy()
    touched[c["seg"][4]:c["seg"][5]] = False
    touched[c["seg"][6]:c["seg"][7]] = False
    for mode in (0, 1, 2):
        clean = _targets(rows_d, n, c["order"], c["seg"], c["tail"], mode, 0.9, 3)
        got = _targets(rows_d, n, order, c["seg"], c["tail"], mode, 0.9, 3)
        want = O.targets_numpy(rows, order, c["seg"], *c["tail"], mode, 0.9, 3, EPS)
        assert clean[3:] == [0, 0] and got[3:] == [1, 0]
        for k in range(3):
            assert not got[k][bad].any()
            same = touched if (k == 0 and mode != 2) else others
            assert _bits(got[k][same], clean[k][same]), (mode, k)
        assert _bits(got[1], want[1]) and _bits(got[2], want[2])
        assert _bits(got[0], want[0]) if mode != 1 else _ulps(got[0], want[0]) <= 1
    # the same bound as everywhere, against the exact series WITHOUT the rows that were not read
    short, seg = np.delete(order, bad), c["seg"].copy()
    seg[5:] -= 1
    seg[7:] -= 1
    exact = K.Exact(rows, short, seg, c["tail"], 0.9)
    got = _targets(rows_d, n, order, c["seg"], c["tail"], 1, 0.9, 0)
    assert exact.bound_fraction(np.delete(got[0], bad)) <= 1.0


def test_refused_arguments():
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    refused_arguments(_lib(), (t.data_ptr() + 15) // 16 * 16)
    torch.cuda.synchronize()
    assert not t.any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_gather_states(n):
    """float32 [n][200] = rows["board"][idx] bit for bit, repeated indices included; guard bands; a bad index gives a board of
    zeros and sets the fault word, the other boards are unchanged"""
    rows = K.case("pos", True, 0.0)["rows"]
    rows_d = _rows_dev(rows)
    rng = np.random.default_rng(n)
    idx = rng.integers(0, len(rows), n).astype(np.int32)
    if n > 2:
        idx[1] = idx[0]
        idx[-1] = len(rows) - 1
    want = rows["board"][idx].astype(np.float32).reshape(n, 200)
    for bad in (None, len(rows), -1):
        use = idx.copy()
        if bad is not None:
            use[n // 2] = bad
        arena = Arena([n * 800, 4])
        o, f = arena.seg[1]
        arena.t[o:o + f] = 0
        idx_d = _dev(use)
        rc = _lib().tm_episode_gather_states(_p(rows_d), len(rows), _p(idx_d), n, arena.ptr(0), arena.ptr(1),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
        arena.check()
        got, fault = arena.bytes(0).view(np.float32).reshape(n, 200), int(arena.bytes(1).view(np.int32)[0])
        w = want.copy()
        if bad is not None:
            w[n // 2] = 0
        assert rc == 0 and fault == (bad is not None) and _bits(got, w)


def _record(tmp, G=12, sims=20, moves=40):
    """12 games of ValueSim at 20 simulations for 40 moves with a recorder, the odd slots hard-dropping so that episodes end
    (tests/test_gpu_episodes.py)"""
    from gpu_helpers import hash_eval_torch
    from test_gpu_tree import _make
    from tetris_mcts_amd.episodes import EpisodeRecorder
    game, agent = _make("ValueSim", G, sims, 8000, 0, evaluator=hash_eval_torch)
    rec = EpisodeRecorder(tmp + "/", "data", 3, G, ring_moves=16)
    for m in range(moves):
        act = np.atleast_1d(agent.play()).astype(np.int32).copy()
        act[1::2] = 3
        rec.add(agent, game, action=act)
        game.play(act)
        rec.advance(game)
        agent.update_root(game)
        if np.atleast_1d(game.end).any():
            game.reset("ended")
            agent.update_root(game)
    rec.close()
    torch.cuda.synchronize()
    return tmp + "/data3"


def test_record_fit_checkpoint_and_command_line(tmp_path, monkeypatch):
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.episodes import EpisodeLoader
    from tetris_mcts_amd.model import Model_VV
    stem = _record(str(tmp_path / "self1"))
    ld = EpisodeLoader(stem)
    assert ld.length == 12 * 40 and len(ld.episodes) >= 12, "every hard-dropping slot finished episodes"
    monkeypatch.chdir(tmp_path)
    model = Model_VV(backend="hip", seed=0)
    before = model.flat_params().clone()
    handed, inner = [], model.train_data

    def spy(data, **kw):
        handed.append(([d.clone() for d in data], kw))
        return inner(data, **kw)
    monkeypatch.setattr(model, "train_data", spy)
    res = O.fit_episodes(model, [stem], td=True, lam=0.9, fit_backend="hip", validation_backend="hip", max_iters=20, batch_size=64)
    assert res["iters"] == 20
    # what the fit was handed = the numpy route on the same shards
    data, kw = handed[0]
    want, info = O.training_set([stem], td=True, lam=0.9, device="cpu")
    assert kw["validation_fraction"] == 0.0 and kw["shuffle"] is False and kw["batch_size"] == 64 and info["n"] == ld.length
    got = [d.cpu().numpy() for d in data]
    assert got[0].shape == (ld.length, 1, 20, 10)
    for k in (0, 2, 3):
        assert _bits(got[k], want[k].numpy()), k
    a, b = got[1].reshape(-1), want[1].numpy().reshape(-1)
    # both routes run the same fp64 recurrence (the kernel as a scan) and round to fp32 once: at most the last bit apart
    print("values: largest difference from the numpy route %d ulp" % _ulps(a, b))
    assert (np.abs(a.astype(np.float64) - b) <= 2.0 ** -23 * np.maximum(np.abs(a), np.abs(b))).all()
    # the fit ran, the checkpoint is the fitted net
    after = model.flat_params()
    assert not torch.equal(before, after) and bool(torch.isfinite(after).all())
    assert os.path.isfile(os.path.join(str(tmp_path), "pytorch_model", "model_checkpoint"))
    fresh = Model_VV(backend="hip", seed=1)
    fresh.load(verbose=False)
    assert torch.equal(fresh.flat_params(), after)
    # the command line on the same directory, in a fresh process
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--data_paths", str(tmp_path / "self1" / "data*"), "--td",
                        "--td_lambda", "0.9", "--validation", "--val_mode", "1", "--val_episodes", "5", "--max_iters", "20",
                        "--batch_size", "64"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Loading model..." in r.stdout and "Saving model..." in r.stdout
    n_val = int(np.isin(ld.episode, np.arange(6)).sum())
    assert "Training data size: %d    Validation data size: %d" % (ld.length - n_val, n_val) in r.stderr
    again = Model_VV(backend="hip", seed=2)
    again.load(verbose=False)
    assert not torch.equal(again.flat_params(), after), "train.py went on from the checkpoint and wrote its own"
