"""The categorical episode targets on the device (csrc/episode_dist_targets.hip: tm_episode_dist_targets) against the numpy
statement of the same definitions (offline.dist_targets_numpy) and the exact oracle of dist_targets_cases.py under the derived
rule of tests/test_offline_dist.py, |x - exact| <= 2^-23 exact + 2^-149 per atom and +0 where exact is 0.  Kernel and statement
each obey it, so they are at most 2^-22 exact + 2^-148 apart (mode 1); mode 0 is a single product per atom and equal bit for bit.
Then the whole route at small scale: recorded ValueSim episodes -> fit_episodes_dist -> checkpoint -> train.py --head dist in a
fresh process -> DistValueSim.

The table (dist_targets_cases.py) holds episodes of 1, 2, 63, 64, 65 and 130 rows that begin at sorted positions 0, 1, 64, 194,
196, 260, 280 and 345: the kernel's run of 64 targets and its chunk of 64 rows, both neighbours, an episode over three chunks.
A bad `order` entry is a bounds check, not a provoked fault: the kernels compare the entry with n_rows before they form an
address, and the test reads that nothing was read (zeros) and that the bit is set."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dist_targets_cases as D
from test_gpu_episodes import FILL, Arena          # the guard bands of the recorder's tests
from test_offline_dist import EPS, EXACT_CASES, _bits, exact, refused_dist_arguments, spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HORIZONS, LAMBDAS = (0, 1, 5, 64, 200), (0.0, 0.5, 0.999, 1.0)


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


def _call(c, mode, lam=0.0, horizon=0, wmode=0, order=None, seg=None, rows=None, tail=None, n_rows=None, presorted=False):
    """the call into guarded arrays; (target [n, K], weight, fault, return code), the fault word cleared before.  The padding of
    the target rows keeps the arena's fill or the test fails here."""
    rows = c["rows"] if rows is None else rows
    order = c["order"] if order is None else order
    p_rows = c["p_rows"]
    if presorted:
        rows, p_rows, order = rows[order], p_rows[order], np.arange(len(order), dtype=np.int32)
    seg, tail, K, n = c["seg"] if seg is None else seg, c["tail"] if tail is None else tail, c["atoms"], len(order)
    arena = Arena([4 * 64 * n, 4 * n, 4])
    o, f = arena.seg[2]
    arena.t[o:o + f] = 0
    keep = [_rows_dev(rows), _dev(np.asarray(order, np.int32)), _dev(np.asarray(seg, np.int32)), _dev(tail[0]), _dev(tail[1]),
            _dev(p_rows)]
    rc = _lib().tm_episode_dist_targets(_p(keep[0]), len(rows) if n_rows is None else n_rows, _p(keep[1]), _p(keep[2]), len(seg) - 1,
                                        _p(keep[3]), _p(keep[4]), _p(keep[5]), 64, K, c["vmin"], c["vmax"], mode, lam, horizon, wmode,
                                        EPS, arena.ptr(0), 64, arena.ptr(1), arena.ptr(2),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    arena.check()
    full = arena.bytes(0).view(np.float32).reshape(n, 64)
    assert (full[:, K:].view(np.uint8) == FILL).all(), "the padding atoms of a target row were written"
    return full[:, :K].copy(), arena.bytes(1).view(np.float32), int(arena.bytes(2).view(np.int32)[0]), rc


_spec_cache = {}


def _spec1(c, final, lam, horizon):
    """the numpy statement in mode 1 without weights: computed once, shared by the tests, never changed"""
    key = (c["atoms"], final, lam, 0 if lam == 0.0 else horizon)
    if key not in _spec_cache:
        _spec_cache[key] = spec(c, 1, lam, horizon)[0]
    return _spec_cache[key]


def _within_twice_the_rule(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return bool((np.abs(a - b) <= 2.0 ** -22 * (1 + 2.0 ** -20) * np.maximum(a, b) + 2.0 ** -148).all())


def _ulps(a, b):
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


@pytest.mark.parametrize("atoms", [1, 2, 50, 64])
@pytest.mark.parametrize("presorted", [False, True])
def test_kernel_equals_the_numpy_statement(atoms, presorted):
    """every horizon x lambda, with and without tails; `order` a permutation of file order (the real case) and the rows sorted
    beforehand (order = 0, 1, 2, ...); NaN in the padding atoms of p_rows throughout"""
    worst = 0
    for final in (True, False):
        c = D.case(atoms, final)
        assert (np.diff(c["order"]) != 1).any() and np.isnan(c["p_rows"][:, atoms:]).all()
        target, weight, fault, rc = _call(c, 0, presorted=presorted)
        assert rc == 0 and fault == 0 and _bits(target, spec(c, 0)[0]) and _bits(weight, np.ones(len(weight)))
        for horizon in HORIZONS:
            for lam in LAMBDAS:
                target, weight, fault, rc = _call(c, 1, lam, horizon, presorted=presorted)
                want = _spec1(c, final, lam, horizon)
                assert rc == 0 and fault == 0 and np.isfinite(target).all(), (final, horizon, lam)
                assert _within_twice_the_rule(target, want), (final, horizon, lam)
                worst = max(worst, _ulps(target, want))
                if lam == 0.0 or horizon == 0:
                    assert _bits(target, c["p_rows"][c["order"], :atoms]), "lambda = 0 and horizon = 0 copy the row's bits"
    print("atoms=%d presorted=%s: largest difference from the numpy statement %d ulp (both add in one order: 0 expected)"
          % (atoms, presorted, worst))


@pytest.mark.parametrize("atoms,final,lam,horizon", EXACT_CASES)
def test_kernel_within_the_derived_bound_of_the_exact_targets(atoms, final, lam, horizon):
    c = D.case(atoms, final)
    target, _, fault, rc = _call(c, 1, lam, horizon)
    frac = exact(atoms, final, 1, lam, horizon).bound_fraction(target)
    print("atoms=%d tails=%s lam=%s horizon=%d: worst |x - exact| = %.3f of 2^-23 exact + 2^-149" % (atoms, final, lam, horizon, frac))
    assert rc == 0 and fault == 0 and frac <= 1.0
    if lam == 0.5 and horizon == 64:                  # (one Monte Carlo table beside it)
        assert exact(atoms, final, 0).bound_fraction(_call(c, 0)[0]) <= 1.0


def test_weights_are_tm_episode_targets_weights():
    """all four weight modes, both modes: the bits of tm_episode_targets' weight output on the same rows"""
    c = D.case(50, True)
    n, n_seg = len(c["order"]), len(c["seg"]) - 1
    rows_d, order_d, seg_d = _rows_dev(c["rows"]), _dev(c["order"]), _dev(c["seg"])
    kind_d, score_d, tval_d = _dev(c["tail"][0]), _dev(c["tail"][1]), torch.zeros(n_seg, device="cuda")
    for wmode in (0, 1, 2, 3):
        out = [torch.zeros(n, device="cuda") for _ in range(3)]
        fault = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = _lib().tm_episode_targets(_p(rows_d), n, _p(order_d), _p(seg_d), n_seg, _p(kind_d), _p(score_d), _p(tval_d), 2, 0.0, wmode,
                                       EPS, _p(out[0]), _p(out[1]), _p(out[2]), _p(fault), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        want = out[2].cpu().numpy()
        assert rc == 0 and int(fault.item()) == 0 and (wmode == 0 or len(set(want.tolist())) > 100)
        for mode in (0, 1):
            got = _call(c, mode, 0.5, 5, wmode)
            assert got[2:] == (0, 0) and _bits(got[1], want) and _bits(got[1], spec(c, mode, 0.5, 5, wmode)[1]), (wmode, mode)


@pytest.mark.parametrize("n_seg", [1, 3, 5])
def test_nothing_else_is_written(n_seg):
    """guard bands around target, weight and the fault word (in every call of this file); the positions behind the last segment
    handed over keep the fill as well, and so do those before the first one"""
    c = D.case(50, True)
    for first in (0, 1):
        sub, tail = c["seg"][first:n_seg + 1], [t[first:n_seg] for t in c["tail"]]
        if len(sub) < 2:
            continue
        a, b = int(sub[0]), int(sub[-1])
        for mode in (0, 1):
            target, weight, fault, rc = _call(c, mode, 0.9, 64, 3, seg=sub, tail=tail)
            want = spec(dict(c, tail=tail), mode, 0.9, 64, 3, seg=sub)
            assert rc == 0 and fault == 0 and _bits(weight[a:b], want[1][a:b]) and _within_twice_the_rule(target[a:b], want[0][a:b])
            for out in (target, weight):
                assert (out[:a].view(np.uint8) == FILL).all() and (out[b:].view(np.uint8) == FILL).all()


def test_nothing_to_do_launches_nothing():
    c = D.case(50, True)
    for kw in (dict(seg=c["seg"][:1], tail=[t[:0] for t in c["tail"]]), dict(n_rows=0)):
        target, weight, fault, rc = _call(c, 1, 0.9, 64, 3, **kw)
        assert rc == 0 and fault == 0
        assert (target.view(np.uint8) == FILL).all() and (weight.view(np.uint8) == FILL).all()


def test_fault_bits():
    """bit 0: order entries that are not rows (one equal to n_rows, one -1) give zero rows and weight 0 there and are left out of
    their episode's series - the numpy statement says what that gives; every other episode is unchanged.  Bit 1: a score that
    falls is a difference taken as 0.  Both at once: 3."""
    c = D.case(50, True)
    n = len(c["rows"])
    bad = [100, int(c["seg"][3]) - 1]                  # inside the 130-move episode (positions 64 .. 193); its last row
    order = c["order"].copy()
    order[bad[0]], order[bad[1]] = n, -1
    others = np.ones(n, bool)
    others[c["seg"][2]:c["seg"][3]] = False
    for mode in (0, 1):
        clean = _call(c, mode, 0.9, 64, 3)
        got = _call(c, mode, 0.9, 64, 3, order=order)
        want = spec(c, mode, 0.9, 64, 3, order=order)
        assert clean[2:] == (0, 0) and got[2:] == (1, 0) and want[2] == 1
        assert not got[0][bad].any() and not got[1][bad].any()
        assert _bits(got[0][others], clean[0][others]) and _bits(got[1], want[1])
        assert _bits(got[0], want[0]) if mode == 0 else _within_twice_the_rule(got[0], want[0])
        assert D.Exact(c, mode, 0.9, 64, order=order).bound_fraction(got[0]) <= 1.0
    kind, tscore = c["tail"]
    low = tscore.copy()
    low[2] = int(c["rows"]["score"][c["order"][64]]) - 1              # the 130-move episode ends below its first row
    for mode in (0, 1):
        got = _call(c, mode, 0.9, 200, tail=(kind, low))
        want = spec(dict(c, tail=(kind, low)), mode, 0.9, 200)
        assert got[2:] == (2, 0) and want[2] == 2 and np.isfinite(got[0]).all()
        assert _bits(got[0], want[0]) if mode == 0 else _within_twice_the_rule(got[0], want[0])
        both = _call(c, mode, 0.9, 200, order=order, tail=(kind, low))
        assert both[2:] == (3, 0) and not both[0][bad].any()
    rows = c["rows"].copy()
    rows["score"][c["order"][70]] = rows["score"][c["order"][64]] - 1  # a row inside the window drops
    assert _call(c, 1, 0.9, 64, rows=rows)[2] == 2 and _call(c, 1, 0.9, 0, rows=rows)[2] == 0


def test_two_runs_give_equal_bits():
    for atoms, lam, horizon in ((50, 0.999, 200), (64, 0.5, 64)):
        c = D.case(atoms, True)
        a, b = _call(c, 1, lam, horizon, 3), _call(c, 1, lam, horizon, 3)
        assert _bits(a[0], b[0]) and _bits(a[1], b[1]) and a[2:] == b[2:] == (0, 0)
    a, b = _call(c, 0), _call(c, 0)
    assert _bits(a[0], b[0])


def test_refused_arguments():
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    refused_dist_arguments(_lib(), (t.data_ptr() + 15) // 16 * 16)
    torch.cuda.synchronize()
    assert not t.any()


def test_record_fit_checkpoint_command_line_and_agent(tmp_path, monkeypatch):
    from test_gpu_offline import _record
    from test_gpu_tree import _make
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.episodes import EpisodeLoader
    from tetris_mcts_amd.model_distributional import Model_Dist
    stem = _record(str(tmp_path / "self1"))
    ld = EpisodeLoader(stem)
    assert ld.length == 12 * 40 and len(ld.episodes) >= 12
    monkeypatch.chdir(tmp_path)
    table, stem_rows, eps, ep_stems = O.load_stems([stem])
    idx = O.episode_index(O.rows_tensor(table), stem_rows, eps, ep_stems)
    boards = torch.from_numpy(np.ascontiguousarray(table["board"]).reshape(-1, 200)).cuda()
    model = Model_Dist(atoms=50, backend="hip", seed=0)
    before = model.flat_params().clone()
    handed, inner = [], model.train_data

    def spy(data, **kw):
        handed.append(([d.clone() for d in data], kw))
        return inner(data, **kw)
    monkeypatch.setattr(model, "train_data", spy)
    # mode 0: the realised returns of the episodes that ended
    res = O.fit_episodes_dist(model, [stem], max_iters=20, batch_size=64, validation_backend="hip")
    assert res["iters"] == 20 and len(handed) == 1
    data, kw = handed[0]
    want, weight, keep = O.episode_dist_targets(table, idx, device="cpu")
    keep = keep.numpy()
    assert 0 < keep.sum() < ld.length and kw["fit_backend"] == "hip_dist" and kw["validation_fraction"] == 0.0 and kw["shuffle"] is False
    assert _bits(data[1].cpu().numpy(), want.numpy()[keep]) and _bits(data[2].cpu().numpy().reshape(-1), weight.numpy()[keep])
    states = data[0].cpu().numpy()
    assert states.shape == (keep.sum(), 1, 22, 10) and not states[:, :, :2].any()
    assert np.array_equal(states[:, 0, 2:], table["board"][idx.order.numpy()][keep].astype(np.float32))
    after0 = model.flat_params().clone()
    assert not torch.equal(before, after0) and bool(torch.isfinite(after0).all())
    assert os.path.isfile(os.path.join(str(tmp_path), "pytorch_model", "model_checkpoint_dist"))
    # mode 1, two rounds: the distributions are the model's own, as it stands before each round
    seen = []

    def on_round(r, data, p_rows):
        own = model.inference_device(boards)
        seen.append((r, data[1].clone(), p_rows.clone(), own))
    res = O.fit_episodes_dist(model, [stem], td=True, lam=0.9, horizon=16, rounds=2, max_iters=20, batch_size=64, on_round=on_round)
    assert [r["iters"] for r in res["rounds"]] == [10, 10] and len(seen) == 2 and len(handed) == 3
    for r, target, p_rows, own in seen:
        assert _bits(p_rows[:, :50].cpu().numpy(), own[:, :50].cpu().numpy()), "p_rows are the head's outputs on the recorded boards"
        want = O.episode_dist_targets(table, idx, td=True, lam=0.9, horizon=16, p_rows=p_rows.cpu(), device="cpu")[0].numpy()
        assert target.shape == (ld.length, 50) and _within_twice_the_rule(target.cpu().numpy(), want)
        assert _bits(handed[1 + r][0][1].cpu().numpy(), target.cpu().numpy())
    assert not _bits(seen[0][2].cpu().numpy(), seen[1][2].cpu().numpy()), "refreshed from the head the first round fitted"
    after = model.flat_params().clone()
    assert not torch.equal(after0, after) and bool(torch.isfinite(after).all())
    fresh = Model_Dist(atoms=50, backend="hip", seed=1)
    fresh.load(verbose=False)
    assert torch.equal(fresh.flat_params(), after)
    # the command line on the same directory, in a fresh process
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--head", "dist", "--data_paths", str(tmp_path / "self1" / "data*"),
                        "--td", "--td_lambda", "0.9", "--bootstrap", "net", "--bootstrap_rounds", "2", "--td_horizon", "16",
                        "--max_iters", "20", "--batch_size", "64"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Loading model..." in r.stdout and "Saving model..." in r.stdout and "iters:20/20" in r.stdout
    again = Model_Dist(atoms=50, backend="hip", seed=2)
    again.load(verbose=False)
    assert not torch.equal(again.flat_params(), after), "train.py went on from the checkpoint and wrote its own"
    # an agent built now plays with those weights; another atom count is refused
    game, agent = _make("DistValueSim", 4, 8, 2000, 0)
    assert torch.equal(agent.model.flat_params(), again.flat_params())
    with pytest.raises(ValueError, match="50 atoms"):
        _make("DistValueSim", 4, 8, 2000, 0, atoms=20, vmin=0, vmax=2000)
