"""Categorical episode targets on the host (tetris_mcts_amd/offline.py: dist_targets_numpy, the specification of
tm_episode_dist_targets) against the exact oracle of dist_targets_cases.py, the closed forms of mode 0, the C call's refusals
(they answer without a GPU), train.py's --head dist flags, Model_Dist's checkpoint.  The GPU half is tests/test_gpu_offline_dist.py.

The accuracy rule is derived, not measured: every term is non-negative, so the fp64 accumulation of at most (horizon + 1)(K + 2)
products errs by about N 2^-53 relative, and one rounding to fp32 adds 2^-24: |x - exact| <= 2^-23 exact + 2^-149 per atom (the
second term: a result below fp32's normal range rounds to a multiple of 2^-149), and +0 where exact is 0."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import dist_targets_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 0.001
# (atoms, tails, lambda, horizon): every atom count, horizon and lambda of the GPU test's lists at least once
EXACT_CASES = [(50, True, 0.5, 64), (50, False, 0.999, 200), (64, True, 1.0, 5), (64, False, 0.5, 1), (2, True, 0.999, 64),
               (2, False, 1.0, 200), (1, True, 0.5, 5), (50, True, 0.0, 64), (64, True, 0.999, 0)]


def spec(c, mode, lam=0.0, horizon=0, wmode=0, order=None, seg=None):
    from tetris_mcts_amd import offline as O
    return O.dist_targets_numpy(c["rows"], c["order"] if order is None else order, c["seg"] if seg is None else seg, *c["tail"],
                                c["atoms"], c["vmin"], c["vmax"], mode, lam, horizon, wmode, EPS, c["p_rows"] if mode == 1 else None)


def _bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


_exact = {}


def exact(atoms, final, mode, lam=0.0, horizon=0):
    key = (atoms, final, mode, lam, 0 if lam == 0.0 else horizon)
    if key not in _exact:
        _exact[key] = D.Exact(D.case(atoms, final), mode, lam, horizon)
    return _exact[key]


@pytest.mark.parametrize("atoms,final,lam,horizon", EXACT_CASES)
def test_lambda_targets_within_the_derived_bound(atoms, final, lam, horizon):
    c = D.case(atoms, final)
    target, weight, fault = spec(c, 1, lam, horizon)
    frac = exact(atoms, final, 1, lam, horizon).bound_fraction(target)
    print("atoms=%d tails=%s lam=%s horizon=%d: worst |x - exact| = %.3f of 2^-23 exact + 2^-149" % (atoms, final, lam, horizon, frac))
    assert fault == 0 and frac <= 1.0 and target.shape == (len(c["order"]), atoms) and target.dtype == np.float32
    assert _bits(weight, np.ones(len(c["order"])))


@pytest.mark.parametrize("atoms", [1, 2, 50, 64])
@pytest.mark.parametrize("final", [True, False])
def test_monte_carlo_targets_and_their_closed_forms(atoms, final):
    c = D.case(atoms, final)
    K, rng = atoms, c["vmax"] - c["vmin"]
    delta = rng / K
    target, _, fault = spec(c, 0)
    assert fault == 0 and exact(atoms, final, 0).bound_fraction(target) <= 1.0
    rows, order, seg = c["rows"], c["order"], c["seg"]
    kind, tscore = c["tail"]
    seen = set()
    for e in range(len(seg) - 1):
        s = rows["score"][order[seg[e]:seg[e + 1]]].astype(np.int64)
        s_end = int(tscore[e]) if kind[e] else int(s[-1])
        for i, j in enumerate(range(seg[e], seg[e + 1])):
            G, t = s_end - int(s[i]), target[j].astype(np.float64)
            assert (t != 0).sum() <= 2 and abs(t.sum() - 1) <= 2.0 ** -23
            if G + delta < rng:                        # both atoms below the top: the mean is the return, half an atom up
                mean = ((np.arange(K) + 0.5) * delta * t).sum()
                assert abs(mean - (G + delta / 2)) <= 2.0 ** -22 * (G + delta), (G, mean)
                seen.add("mean")
            if G >= rng - delta:                       # n >= K - 1: everything is in the top atom
                assert t[K - 1] == 1.0
                seen.add("top")
            if G / delta == np.floor(G / delta):       # a whole number of atoms: f = 0, one atom
                assert t[min(int(G / delta), K - 1)] == 1.0
                seen.add("whole")
    assert seen == ({"top", "whole"} if K == 1 else {"mean", "top", "whole"})


@pytest.mark.parametrize("atoms", [2, 50, 64])
def test_lambda_zero_and_horizon_zero_copy_the_row(atoms):
    c = D.case(atoms, True)
    want = c["p_rows"][c["order"], :atoms]
    for lam, horizon in ((0.0, 64), (0.0, 0), (0.5, 0), (1.0, 0)):
        assert _bits(spec(c, 1, lam, horizon)[0], want), (lam, horizon)


@pytest.mark.parametrize("final", [True, False])
def test_a_horizon_past_the_episode_is_the_untruncated_sum(final):
    c = D.case(50, final)
    longest = int(np.diff(c["seg"]).max()) + 1
    assert longest == 131
    whole = spec(c, 1, 0.999, longest)[0]
    assert _bits(whole, spec(c, 1, 0.999, 200)[0]) and _bits(whole, spec(c, 1, 0.999, 10 ** 6)[0])
    assert not _bits(whole, spec(c, 1, 0.999, 64)[0])


def test_weights_are_the_value_targets():
    from tetris_mcts_amd import offline as O
    c = D.case(50, True)
    tval = np.zeros(len(c["seg"]) - 1, np.float32)
    for wmode in (0, 1, 2, 3):
        want = O.targets_numpy(c["rows"], c["order"], c["seg"], *c["tail"], tval, 2, 0.0, wmode, EPS)[2]
        assert _bits(spec(c, 0, wmode=wmode)[1], want) and _bits(spec(c, 1, 0.5, 5, wmode=wmode)[1], want)


def test_a_bad_order_entry_and_a_falling_score():
    """an order entry that is not a row: a zero target row, weight 0 and bit 0 - and the series without it; a score that falls:
    the difference is taken as 0 and bit 1 is set"""
    c = D.case(50, True)
    n = len(c["rows"])
    bad = [100, int(c["seg"][3]) - 1]                  # inside the 130-move episode; its last row
    order = c["order"].copy()
    order[bad[0]], order[bad[1]] = n, -1
    for mode in (0, 1):
        target, weight, fault = spec(c, mode, 0.9, 64, 3, order=order)
        assert fault == 1 and not target[bad].any() and not weight[bad].any()
        clean = spec(c, mode, 0.9, 64, 3)
        others = np.ones(n, bool)
        others[c["seg"][2]:c["seg"][3]] = False
        assert _bits(target[others], clean[0][others]) and _bits(np.delete(weight, bad), np.delete(clean[1], bad))
        short, seg = np.delete(order, bad), c["seg"].copy()
        seg[3:] -= 2
        assert _bits(np.delete(target, bad, 0), spec(c, mode, 0.9, 64, 3, order=short, seg=seg)[0])
        assert D.Exact(c, mode, 0.9, 64, order=order).bound_fraction(target) <= 1.0
    rows = c["rows"].copy()
    j = int(c["order"][70])                            # mode 1: a row of the 130-move episode drops below the ones before it
    rows["score"][j] = rows["score"][c["order"][64]] - 1
    target, _, fault = spec(dict(c, rows=rows), 1, 0.9, 64)
    assert fault == 2 and np.isfinite(target).all() and (target >= 0).all()
    assert spec(dict(c, rows=rows), 1, 0.9, 0)[2] == 0, "no term looks at another row: nothing fell"
    kind, tscore = c["tail"]
    low = tscore.copy()
    low[2] = int(c["rows"]["score"][c["order"][64]]) - 1              # both modes: the episode ends below its first row
    for mode in (0, 1):
        target, _, fault = spec(dict(c, tail=(kind, low)), mode, 0.9, 200)
        assert fault == 2 and np.isfinite(target).all() and (target >= 0).all()
        if mode == 0:                                  # a difference taken as 0: all mass in atom 0
            assert (target[64:194, 0] == 1).all()


def _cli():
    spec_ = importlib.util.spec_from_file_location("tm_train_cli_dist", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


def test_train_cli_head_flags_and_defaults():
    cli = _cli()
    d = vars(cli.build_parser().parse_args([]))
    assert (d["head"], d["atoms"], d["vmin"], d["vmax"], d["td_horizon"]) == ("value", 50, 0.0, 5000.0, 64)
    assert type(d["atoms"]) is int and type(d["td_horizon"]) is int and type(d["vmax"]) is float
    a = cli.build_parser().parse_args(["--head", "dist", "--atoms", "20", "--vmin", "-5", "--vmax", "100", "--td_horizon", "8"])
    assert (a.head, a.atoms, a.vmin, a.vmax, a.td_horizon) == ("dist", 20, -5.0, 100.0, 8)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--head", "other"])


@pytest.mark.parametrize("flags,word", [
    (["--td"], "--td_lambda"), (["--td", "--td_lambda", "0.5"], "--bootstrap net"),
    (["--td", "--td_lambda", "0.5", "--bootstrap", "recorded"], "--bootstrap net"), (["--target_gamma", "0.999"], "--target_gamma"),
    (["--td", "--td_lambda", "0.5", "--bootstrap", "net", "--td_horizon", "-1"], "--td_horizon"),
    (["--td", "--td_lambda", "0.5", "--bootstrap", "net", "--new"], "--new"), (["--ewc"], "Fisher"), (["--save_loss"], "HDF5"),
    (["--atoms", "65"], "--atoms"), (["--vmin", "3", "--vmax", "3"], "--vmin"), (["--bootstrap_rounds", "2"], "--bootstrap net")])
def test_train_cli_head_dist_refusals(flags, word, monkeypatch):
    """refused with a message before anything is imported: a missing package would show"""
    cli = _cli()
    import builtins
    real = builtins.__import__

    def no_package(name, *a, **k):
        assert not name.startswith("tetris_mcts_amd"), "imported before the refusal"
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_package)
    with pytest.raises(SystemExit) as e:
        cli.main(["--head", "dist", "--data_paths", "x"] + flags)
    assert word in str(e.value.code)


def test_train_cli_value_head_is_untouched():
    """--head value: a --target_gamma, --td without --td_lambda and --td with recorded values stay what they were"""
    cli = _cli()
    for flags in (["--target_gamma", "0.999"], ["--td"], ["--td", "--td_lambda", "0.5"]):
        args = cli.build_parser().parse_args(["--data_paths", "x"] + flags)
        cli.check_args(args)
        assert args.head == "value"


def refused_dist_arguments(lib, ptr):
    """every refusal of tm_episode_dist_targets returns hipErrorInvalidValue; `ptr`: a non-null, 16-byte aligned address that is
    never dereferenced (the checks come before the first HIP call)"""
    INVALID, p, null = 1, C.c_void_p(ptr), C.c_void_p(0)

    def call(rows=p, n_rows=10, order=p, seg=p, n_seg=2, kind=p, score=p, p_rows=p, p_stride=64, atoms=50, vmin=0.0, vmax=5000.0,
             mode=1, lam=0.5, horizon=64, wmode=0, target=p, target_stride=64, weight=p, fault=p):
        return lib.tm_episode_dist_targets(rows, n_rows, order, seg, n_seg, kind, score, p_rows, p_stride, atoms, vmin, vmax, mode, lam,
                                           horizon, wmode, EPS, target, target_stride, weight, fault, null)
    inf, nan = float("inf"), float("nan")
    for kw in (dict(n_rows=-1), dict(n_seg=-1), dict(mode=-1), dict(mode=2), dict(wmode=-1), dict(wmode=4), dict(lam=-0.1),
               dict(lam=1.5), dict(lam=nan), dict(rows=null), dict(order=null), dict(seg=null), dict(kind=null), dict(score=null),
               dict(target=null), dict(weight=null), dict(fault=null), dict(rows=C.c_void_p(ptr + 2)), dict(n_rows=2 ** 31 - 1),
               dict(atoms=0), dict(atoms=65), dict(atoms=-3), dict(target_stride=49), dict(p_stride=49), dict(vmax=0.0),
               dict(vmin=5000.0), dict(vmax=inf), dict(vmin=-inf), dict(vmax=nan), dict(vmin=nan), dict(vmin=-1e308, vmax=1e308),
               dict(horizon=-1), dict(p_rows=null), dict(p_rows=C.c_void_p(ptr + 2)), dict(target=C.c_void_p(ptr + 1))):
        assert call(**kw) == INVALID, kw
    # nothing to do is not an error - unless an argument is refused whatever the sizes
    assert call(n_rows=0, rows=null) == 0 and call(n_seg=0, seg=null, kind=null, p_rows=null) == 0
    assert call(n_seg=0, mode=2) == INVALID and call(n_rows=0, atoms=65) == INVALID and call(n_rows=0, horizon=-1) == INVALID
    assert call(n_seg=0, vmax=-1.0) == INVALID and call(n_rows=0, target_stride=3) == INVALID


def test_refused_arguments_without_a_gpu():
    from tetris_mcts_amd import _lib
    buf = (C.c_char * 64)()
    refused_dist_arguments(_lib.lib(), (C.addressof(buf) + 15) // 16 * 16)


def test_checkpoint_round_trip_and_the_atom_count(tmp_path):
    from tetris_mcts_amd.model_distributional import CHECKPOINT, Model_Dist
    assert CHECKPOINT.endswith("pytorch_model/model_checkpoint_dist")
    path = str(tmp_path / "pytorch_model" / "model_checkpoint_dist")
    a = Model_Dist(atoms=20, device="cpu", seed=0, backend="torch")
    x = torch.zeros(4, 1, 22, 10)
    x[:, 0, 10:, ::2] = 1
    t = torch.full((4, 20), 1 / 20)
    a.train_data([x, t, torch.ones(4, 1)], batch_size=2, max_iters=3, validation_fraction=0.0, log=False)     # the optimiser has state
    a.save(path, verbose=False)
    ck = torch.load(path)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict"} and ck["optimizer_state_dict"]["param_groups"][0]["amsgrad"]
    assert set(ck["optimizer_state_dict"]["state"][0]) >= {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    b = Model_Dist(atoms=20, device="cpu", seed=1, backend="torch")
    assert not torch.equal(b.model.seq.fc1.weight, a.model.seq.fc1.weight)
    b.load(path, verbose=False)
    for k, v in a.model.state_dict().items():
        assert torch.equal(b.model.state_dict()[k], v), k
    sa, sb = a.optimizer.state_dict()["state"], b.optimizer.state_dict()["state"]
    assert all(torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]) and int(sa[i]["step"]) == int(sb[i]["step"]) == 3 for i in sa)
    with pytest.raises(ValueError, match="20 atoms"):
        Model_Dist(atoms=50, device="cpu", seed=0, backend="torch").load(path, verbose=False)
    fresh = Model_Dist(atoms=20, device="cpu", seed=2, backend="torch")
    before = {k: v.clone() for k, v in fresh.model.state_dict().items()}
    fresh.load(str(tmp_path / "nothing"), verbose=False)              # no file: nothing changes
    assert all(torch.equal(before[k], v) for k, v in fresh.model.state_dict().items())


def test_fit_episodes_dist_refuses_a_value_net_and_bad_options():
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model_distributional import Model_Dist

    class Model_VV:            # (fit_episodes_dist looks at the class before it looks at anything else)
        pass
    with pytest.raises(TypeError, match="fits a Model_Dist"):
        O.fit_episodes_dist(Model_VV(), ["nothing"])
    m = Model_Dist(atoms=20, device="cpu", seed=0, backend="torch")
    with pytest.raises(ValueError, match="no distribution"):
        O.fit_episodes_dist(m, ["nothing"], td=True)
    with pytest.raises(ValueError, match="rounds"):
        O.fit_episodes_dist(m, ["nothing"], rounds=2)
    with pytest.raises(ValueError, match="horizon"):
        O.fit_episodes_dist(m, ["nothing"], td=True, lam=0.5, horizon=-1)
    with pytest.raises(ValueError, match="vmin < vmax"):
        O.fit_episodes_dist(m, ["nothing"], vmin=3, vmax=3)


def test_the_route_on_the_host(tmp_path):
    """fit_episodes_dist with a torch head on CPU tensors: the data handed to train_data is the numpy statement on the files,
    mode 1's distributions are the model's, the checkpoint is written"""
    import episode_targets_cases as K
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model_distributional import Model_Dist
    rows, ep = K.make_table("pos")
    stem = str(tmp_path / "data4")
    K.write_shards(stem, rows[:K.G * 40], ep[ep["moves"] <= 2], split=K.G * 20)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        m = Model_Dist(atoms=20, device="cpu", seed=0, backend="torch")
        seen = []
        res = O.fit_episodes_dist(m, [stem], td=True, lam=0.9, horizon=8, vmin=0, vmax=40000, rounds=2, max_iters=4, batch_size=8,
                                  on_round=lambda r, data, p: seen.append((r, [d.clone() for d in data], p.clone())))
        assert [r["iters"] for r in res["rounds"]] == [2, 2] and os.path.isfile("pytorch_model/model_checkpoint_dist")
        assert len(seen) == 2 and not torch.equal(seen[0][2], seen[1][2]), "the distributions were refreshed from the fitted head"
        table, stem_rows, eps, ep_stems = O.load_stems([stem])
        idx = O.episode_index(O.rows_tensor(table), stem_rows, eps, ep_stems)
        for r, data, p in seen:
            want, weight, keep = O.episode_dist_targets(table, idx, td=True, lam=0.9, horizon=8, atoms=20, vmin=0, vmax=40000,
                                                        p_rows=p, device="cpu")
            assert bool(keep.all()) and _bits(data[1].numpy(), want.numpy()) and data[0].shape == (len(table), 1, 22, 10)
            assert not data[0][:, :, :2].any() and np.array_equal(data[0][:, 0, 2:].numpy(), table["board"][idx.order.numpy()])
        again = Model_Dist(atoms=20, device="cpu", seed=5, backend="torch")
        again.load(verbose=False)
        assert all(torch.equal(v, again.model.state_dict()[k]) for k, v in m.model.state_dict().items())
    finally:
        os.chdir(cwd)
