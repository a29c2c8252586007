"""The discounted offline targets on the device (csrc/episode_targets.hip: tm_episode_targets_discounted) against the exact
oracle of discount_cases.py with the derived bound of tests/test_offline_discount.py, |value_i - exact_i| <= 2^-23 M_i, and
against the numpy statement (offline.targets_numpy), whose distance in ulp is measured and printed, not fixed.  At gamma = 1
without v_rows the call must return tm_episode_targets' bytes.  Then predict_rows, and the whole route at small scale: recorded
ValueSim episodes -> fit_episodes(bootstrap="net") over two rounds -> checkpoint -> train.py in a fresh process.

A bad `order` entry is a bounds check, not a provoked fault: the kernel compares the entry with n_rows before it forms an
address (of the row or of v_rows), and the test reads that nothing was read (zeros) and that the flag is set."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import discount_cases as D
import episode_targets_cases as K
from test_gpu_episodes import FILL, Arena
from test_gpu_offline import _dev, _lib, _p, _record, _rows_dev, _ulps
from test_offline import EPS, _bits
from test_offline_discount import refused_discounted_arguments

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(rows_d, n_rows, order, seg, tail, mode, lam, wmode, gamma=None, v_rows_d=None):
    """tm_episode_targets_discounted (gamma given) or tm_episode_targets (gamma None) into guarded arrays: [value, variance,
    weight, fault, return code], the fault word cleared before"""
    n, n_seg = len(order), len(seg) - 1
    arena = Arena([4 * n, 4 * n, 4 * n, 4])
    o, f = arena.seg[3]
    arena.t[o:o + f] = 0
    keep = [_dev(np.asarray(order, np.int32)), _dev(np.asarray(seg, np.int32))] + [_dev(x[:n_seg]) for x in tail]
    head = (_p(rows_d), n_rows, _p(keep[0]), _p(keep[1]), n_seg, _p(keep[2]), _p(keep[3]), _p(keep[4]))
    out = (arena.ptr(0), arena.ptr(1), arena.ptr(2), arena.ptr(3), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if gamma is None:
        rc = _lib().tm_episode_targets(*head, mode, lam, wmode, EPS, *out)
    else:
        rc = _lib().tm_episode_targets_discounted(*head, C.c_void_p(0) if v_rows_d is None else _p(v_rows_d), mode, lam, gamma, wmode,
                                                  EPS, *out)
    arena.check()
    return [arena.bytes(i).view(np.float32) for i in range(3)] + [int(arena.bytes(3).view(np.int32)[0]), rc]


_spec_cache = {}


def _spec(t, mode, lam, gamma, final, use_v_rows):
    """the numpy statement over all 37 episodes, computed once (its values do not depend on the weight mode or on the layout)"""
    from tetris_mcts_amd import offline as O
    key = (mode, lam, gamma, final, use_v_rows)
    if key not in _spec_cache:
        _spec_cache[key] = O.targets_numpy(t["rows"], t["order"], t["seg"], *D.tails(t, final), mode, lam, 0, EPS, gamma=gamma,
                                           v_rows=t["v_rows"] if use_v_rows else None)[0]
    return _spec_cache[key]


@pytest.mark.parametrize("n_seg", [1, 5, 37])
@pytest.mark.parametrize("presorted", [False, True])
def test_kernel_within_the_bound_and_nothing_else_written(n_seg, presorted):
    """every gamma x lambda, with and without tails, v_rows absent and given, modes 0, 1 and 2; `order` a permutation of table
    order and the rows sorted beforehand; guard bands around the three outputs and the fault word, the positions behind the last
    segment handed over keep the fill, rows and v_rows are unchanged; variance and weight are tm_episode_targets' bits"""
    t = D.table()
    n = len(t["rows"])
    if presorted:
        rows_h, order, v_h = t["sorted"], np.arange(n, dtype=np.int32), t["v_rows"][t["order"]]
    else:
        rows_h, order, v_h = t["rows"], t["order"], t["v_rows"]
    rows_d, v_d = _rows_dev(rows_h), _dev(v_h)
    seg, end = t["seg"][:n_seg + 1], int(t["seg"][n_seg])
    worst, worst_ulp, old = 0.0, 0, {}
    for final in (True, False):
        tail = D.tails(t, final)
        for wmode in (0, 1, 2, 3):
            old[wmode] = _call(rows_d, n, order, seg, tail, 2, 0.0, wmode)
            assert old[wmode][3:] == [0, 0]

        def run(mode, lam, gamma, use_v, wmode):
            got = _call(rows_d, n, order, seg, tail, mode, lam, wmode, gamma, v_d if use_v else None)
            assert got[3:] == [0, 0], (mode, lam, gamma, use_v)
            assert _bits(got[1][:end], old[wmode][1][:end]) and _bits(got[2][:end], old[wmode][2][:end])
            for g in got[:3]:
                assert (g[end:].view(np.uint8) == FILL).all()
            return got[0]
        for use_v in (False, True):
            for gi, gamma in enumerate(D.GAMMAS):
                for li, lam in enumerate(D.LAMBDAS):
                    value = run(1, lam, gamma, use_v, (gi + li) % 4)
                    frac = D.exact(1, lam, gamma, final, use_v).bound_fraction(value, range(end))
                    ulp = _ulps(value[:end], _spec(t, 1, lam, gamma, final, use_v)[:end])
                    worst, worst_ulp = max(worst, frac), max(worst_ulp, ulp)
                    assert frac <= 1.0, ("mode 1", final, use_v, gamma, lam, frac)
                    if lam == 0.0:
                        assert _bits(value[:end], (t["v_rows"][t["order"]] if use_v else t["sorted"]["value"])[:end])
                assert _bits(run(2, 0.0, gamma, use_v, gi)[:end], (t["v_rows"][t["order"]] if use_v else t["sorted"]["value"])[:end])
        for gi, gamma in enumerate(D.GAMMAS):
            value = run(0, 0.0, gamma, False, gi)
            frac = D.exact(0, 0.0, gamma, final, False).bound_fraction(value, range(end))
            ulp = _ulps(value[:end], _spec(t, 0, 0.0, gamma, final, False)[:end])
            worst, worst_ulp = max(worst, frac), max(worst_ulp, ulp)
            assert frac <= 1.0, ("mode 0", final, gamma, frac)
    print("n_seg=%d presorted=%s: the kernel uses %.3f of 2^-23 M at worst; %d ulp at most from the numpy statement"
          % (n_seg, presorted, worst, worst_ulp))
    assert rows_d.cpu().numpy().tobytes() == rows_h.tobytes() and _bits(v_d.cpu().numpy(), v_h)


@pytest.mark.parametrize("draw", ["pos", "mixed"])
def test_gamma_one_without_v_rows_is_the_old_call_byte_for_byte(draw):
    """every mode, weight mode and lambda of tests/test_gpu_offline.py's cases, with and without tails, and with bad order entries
    (fault = 1 on both sides)"""
    for final in (True, False):
        c = K.case(draw, final, 0.0)
        rows_d, n = _rows_dev(c["rows"]), len(c["rows"])
        bad = c["order"].copy()
        bad[int(c["seg"][4]) + 100], bad[int(c["seg"][7]) - 1] = n, -1
        for order, fault in ((c["order"], 0), (bad, 1)):
            for mode, lams in ((0, (0.0,)), (2, (0.0,)), (1, K.LAMBDAS)):
                for lam in lams:
                    for wmode in (0, 1, 2, 3):
                        old = _call(rows_d, n, order, c["seg"], c["tail"], mode, lam, wmode)
                        new = _call(rows_d, n, order, c["seg"], c["tail"], mode, lam, wmode, gamma=1.0)
                        assert old[3:] == new[3:] == [fault, 0]
                        assert all(_bits(a, b) for a, b in zip(old[:3], new[:3])), (final, mode, lam, wmode)


def test_bad_order_entries_and_a_bad_seg():
    """two order entries that are no rows in the middle of segments, and a last seg entry beyond the table: zeros and weight 0
    at the two positions, fault = 1, neither a row nor a v_rows element read there; the rest is the series WITHOUT those rows -
    the numpy statement says what that gives, and the bound holds against the exact oracle of the shortened series"""
    from tetris_mcts_amd import offline as O
    t = D.table()
    n = len(t["rows"])
    rows_d, v_d = _rows_dev(t["rows"]), _dev(t["v_rows"])
    bad = [int(t["seg"][5]) + 70, int(t["seg"][11]) + 3]                  # inside two episodes of 130 moves
    order, seg = t["order"].copy(), t["seg"].copy()
    order[bad[0]], order[bad[1]] = n, -1
    tail = D.tails(t, True)
    short, seg_short = np.delete(order, bad), t["seg"].copy()
    seg_short[6:] -= 1
    seg_short[12:] -= 1
    for mode, lam, use_v in ((1, 0.9, True), (0, 0.0, False)):
        clean = _call(rows_d, n, t["order"], seg, tail, mode, lam, 3, 0.999, v_d if use_v else None)
        got = _call(rows_d, n, order, seg, tail, mode, lam, 3, 0.999, v_d if use_v else None)
        want = O.targets_numpy(t["rows"], order, seg, *tail, mode, lam, 3, EPS, gamma=0.999, v_rows=t["v_rows"] if use_v else None)
        assert clean[3:] == [0, 0] and got[3:] == [1, 0] and want[3] == 1
        others = np.ones(n, bool)
        others[bad] = False
        for k in range(3):
            assert not got[k][bad].any()
        assert _bits(got[1], want[1]) and _bits(got[2], want[2])
        assert _bits(got[1][others], clean[1][others]) and _bits(got[2][others], clean[2][others])
        touched = others.copy()
        touched[seg[5]:seg[6]] = False
        touched[seg[11]:seg[12]] = False
        assert _bits(got[0][touched], clean[0][touched]), "every other episode is unchanged"
        exact = D.Exact(t, mode, lam, 0.999, True, use_v, order=short, seg=seg_short)
        frac = exact.bound_fraction(np.delete(got[0], bad))
        print("mode %d with two rows left out: %.3f of 2^-23 M; %d ulp from the numpy statement" % (mode, frac, _ulps(got[0], want[0])))
        assert frac <= 1.0
        # a seg entry beyond the table is clamped: the same outputs, and the flag
        far = seg.copy()
        far[-1] = n + 7
        clamped = _call(rows_d, n, t["order"], far, tail, mode, lam, 3, 0.999, v_d if use_v else None)
        assert clamped[3:] == [1, 0] and all(_bits(a, b) for a, b in zip(clamped[:3], clean[:3]))


def test_refused_arguments():
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    refused_discounted_arguments(_lib(), (t.data_ptr() + 15) // 16 * 16)
    torch.cuda.synchronize()
    assert not t.any()


def test_predict_rows_is_inference_device_on_the_gathered_boards():
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model import Model_VV
    rows = K.case("pos", True, 0.0)["rows"][:1000]
    rows_d = _rows_dev(rows)
    model = Model_VV(backend="hip", seed=0)
    boards = O.gather_states(rows_d, torch.arange(1000, dtype=torch.int32, device="cuda"))
    assert np.array_equal(boards.cpu().numpy().reshape(1000, 20, 10), rows["board"].astype(np.float32))
    v, var = model.inference_device(boards.reshape(1000, 200).to(torch.int8))
    v, var = v.cpu().numpy(), var.cpu().numpy()
    assert np.isfinite(v).all() and len(np.unique(v)) > 900
    for chunk in (64, 1000):
        got = O.predict_rows(model, rows_d, chunk=chunk)
        assert got[0].shape == got[1].shape == (1000,) and got[0].dtype == torch.float32
        assert _bits(got[0].cpu().numpy(), v) and _bits(got[1].cpu().numpy(), var), chunk
    with pytest.raises(ValueError):
        O.predict_rows(model, rows_d, chunk=0)


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """12 games of ValueSim recorded for 40 moves (tests/test_gpu_offline.py's recipe), once for the tests below"""
    return _record(str(tmp_path_factory.mktemp("discount") / "self1"))


FIT = dict(td=True, lam=0.9, fit_backend="hip", validation_backend="hip", batch_size=64)


def test_two_rounds_bootstrap_from_the_net_being_fitted(recorded, tmp_path, monkeypatch):
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model import Model_VV
    monkeypatch.chdir(tmp_path)
    model = Model_VV(backend="hip", seed=0)
    table = O.load_stems([recorded])[0]
    rows_d = O.rows_tensor(table, "cuda")
    seen = []

    def on_round(r, data, v_rows):
        again = O.predict_rows(model, rows_d)[0]                          # the model as it stands when the round begins
        seen.append(dict(r=r, data=[d.clone() for d in data], v_rows=v_rows.clone(), again=again, params=model.flat_params().clone()))
    first = O.predict_rows(model, rows_d)[0].clone()
    before = model.flat_params().clone()
    res = O.fit_episodes(model, [recorded], gamma=0.999, bootstrap="net", bootstrap_rounds=2, max_iters=40, on_round=on_round,
                         validation=True, val_set_size=0.1, generator=torch.Generator(device="cuda").manual_seed(3), **FIT)
    assert [s["r"] for s in seen] == [0, 1] and res["iters"] == 20 and [r["iters"] for r in res["rounds"]] == [20, 20]
    assert all(set(r) == {"iters", "best_validation", "graph_replay"} for r in res["rounds"])
    a, b = seen
    assert torch.equal(a["v_rows"], first) and torch.equal(a["params"], before), "round 1: the loaded model's predictions"
    assert torch.equal(b["v_rows"], b["again"]) and not torch.equal(b["params"], before), "round 2: the model after round 1"
    assert not torch.equal(a["v_rows"], b["v_rows"]) and not torch.equal(model.flat_params(), b["params"])
    # the split, the boards, the variances and the weights are computed once
    for k in (0, 2, 3):
        assert torch.equal(a["data"][k], b["data"][k]), k
    n = len(table)
    assert a["data"][0].shape == (n, 1, 20, 10), "mode 1 drops nothing: held-out rows are among them"
    # the values of both rounds: the numpy statement fed that round's predictions, over the same selection (the same draw)
    _, info = O.training_set([recorded], td=True, lam=0.9, validation=True, val_set_size=0.1, device="cuda",
                             generator=torch.Generator(device="cuda").manual_seed(3))
    assert info["n_val"] == n // 10 and torch.equal(info["rows"], rows_d) and info["sel"].shape == (n,)
    pos = info["sel"].cpu().numpy()
    assert sorted(pos.tolist()) == list(range(n))
    index = O.EpisodeIndex(*[x.cpu() for x in info["index"]])
    boards = table["board"][index.order.numpy()[pos]].astype(np.float32)
    for s in seen:
        v = s["v_rows"].cpu()
        args = dict(td=True, lam=0.9, gamma=0.999, device="cpu")
        want, var, weight, _ = O.episode_targets(table, index, v_rows=v, **args)
        M = O.episode_targets(table, index, v_rows=v.abs(), **args)[0].numpy().astype(np.float64)
        got = s["data"][1].reshape(-1).cpu().numpy()
        assert np.array_equal(s["data"][0].cpu().numpy().reshape(n, 20, 10), boards)
        assert _bits(s["data"][2].reshape(-1).cpu().numpy(), var.numpy()[pos])
        assert _bits(s["data"][3].reshape(-1).cpu().numpy(), weight.numpy()[pos])
        w = want.numpy()[pos]
        # scores do not fall, so M_i is the statement itself on |v|; each side is within 2^-24 M_i of the exact value plus
        # fp64's noise (below 2^-20 of that), so the two are within 2^-23 M_i (1 + 2^-20) of each other
        err = np.abs(got.astype(np.float64) - w.astype(np.float64))
        print("round %d: values at most %d ulp from the numpy statement, %.3f of 2^-23 M" %
              (s["r"], _ulps(got, w), float((err / np.maximum(2.0 ** -23 * M[pos], 1e-300)).max())))
        assert (err <= 2.0 ** -23 * M[pos] * (1 + 2.0 ** -20)).all()
    assert os.path.isfile(os.path.join(str(tmp_path), "pytorch_model", "model_checkpoint"))
    model.set_flat_params(torch.full_like(before, float("nan")))
    with pytest.raises(RuntimeError, match="not all finite"):
        O.fit_episodes(model, [recorded], gamma=0.999, bootstrap="net", max_iters=4, **FIT)


def test_the_defaults_are_the_fit_without_them(recorded, tmp_path, monkeypatch):
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model import Model_VV
    monkeypatch.chdir(tmp_path)
    ends = []
    for extra in ({}, dict(gamma=1.0, bootstrap="recorded", bootstrap_rounds=1, on_round=None)):
        model = Model_VV(backend="hip", seed=0)
        torch.manual_seed(11)
        res = O.fit_episodes(model, [recorded], max_iters=20, **FIT, **extra)
        assert res["iters"] == 20 and len(res["rounds"]) == 1
        ends.append(model.flat_params().clone())
    assert torch.equal(ends[0], ends[1]) and bool(torch.isfinite(ends[0]).all())


def test_train_command_line_with_the_new_flags(recorded, tmp_path):
    from tetris_mcts_amd.model import Model_VV
    cwd = str(tmp_path)
    start = Model_VV(backend="hip", seed=4)
    start.save(os.path.join(cwd, "pytorch_model", "model_checkpoint"), verbose=False)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--data_paths", os.path.join(os.path.dirname(recorded), "data*"),
                        "--td", "--td_lambda", "0.9", "--target_gamma", "0.999", "--bootstrap", "net", "--bootstrap_rounds", "2",
                        "--max_iters", "40", "--batch_size", "64"], capture_output=True, text=True, timeout=600, cwd=cwd)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Loading model..." in r.stdout and "Saving model..." in r.stdout and "iters:40/40" in r.stdout
    assert r.stderr.count("Training data size:") == 2, "two rounds, two fits"
    after = Model_VV(backend="hip", seed=5)
    after.load(os.path.join(cwd, "pytorch_model", "model_checkpoint"), verbose=False)
    assert not torch.equal(after.flat_params(), start.flat_params()) and bool(torch.isfinite(after.flat_params()).all())
