"""The discounted offline targets on the host (tetris_mcts_amd/offline.py: gamma, v_rows, bootstrap): the numpy statement
against the exact oracle of discount_cases.py, its identity with the undiscounted statement at the defaults, the refusals of
tm_episode_targets_discounted that answer without a GPU, and the new flags of train.py.  The GPU half is
tests/test_gpu_offline_discount.py.

The bound is the project's (tests/test_offline.py) with the discounted terms, |value_i - exact_i| <= 2^-23 M_i:
    mode 1  M_i = sum_k lam^k A_{i,k} / sum_k lam^k,  A_{i,k} = sum_{j<k} gamma^j |r_{i+j}| + gamma^k |v_{i+k}|
    mode 0  M_i = sum_k gamma^k |r_{i+k}|
It is derived, not measured: the one fp32 rounding costs at most 2^-24 M_i (|exact_i| <= M_i), and the fp64 recurrence over at
most 2^20 rows stays far below another 2^-24 M_i.  The numpy statement measured 0.50 of it on these tables."""
import ctypes as C

import numpy as np
import pytest

import discount_cases as D
import episode_targets_cases as K
from test_offline import EPS, _bits, _cli

N_SEG = 12           # every length twice: the host half of the grid (the device half runs all 37 episodes)


def _spec(t, mode, lam, gamma, final, use_v_rows, wmode=0, n_seg=N_SEG):
    from tetris_mcts_amd import offline as O
    kind, score, value = D.tails(t, final)
    return O.targets_numpy(t["rows"], t["order"], t["seg"][:n_seg + 1], kind[:n_seg], score[:n_seg], value[:n_seg], mode, lam, wmode,
                           EPS, gamma=gamma, v_rows=t["v_rows"] if use_v_rows else None)


@pytest.mark.parametrize("final", [True, False])
@pytest.mark.parametrize("use_v_rows", [False, True])
def test_lambda_return_within_the_derived_bound(final, use_v_rows):
    t = D.table()
    end, worst = int(t["seg"][N_SEG]), 0.0
    for gamma in D.GAMMAS:
        for lam in D.LAMBDAS:
            value, var, _, fault = _spec(t, 1, lam, gamma, final, use_v_rows)
            frac = D.exact(1, lam, gamma, final, use_v_rows, N_SEG).bound_fraction(value, range(end))
            worst = max(worst, frac)
            assert fault == 0 and frac <= 1.0, (gamma, lam, frac)
            assert _bits(var[:end], t["sorted"]["variance"][:end])
            if lam == 0.0:
                v = t["v_rows"][t["order"]] if use_v_rows else t["sorted"]["value"]
                assert _bits(value[:end], v[:end]), "lambda = 0 is v_i itself, whatever gamma"
    print("lambda-return final=%s v_rows=%s: worst |value - exact| = %.3f of 2^-23 M" % (final, use_v_rows, worst))


@pytest.mark.parametrize("final", [True, False])
def test_discounted_sum_within_the_derived_bound(final):
    t = D.table()
    end, worst = int(t["seg"][N_SEG]), 0.0
    for gamma in D.GAMMAS:
        value, _, _, fault = _spec(t, 0, 0.0, gamma, final, False)
        frac = D.exact(0, 0.0, gamma, final, False, N_SEG).bound_fraction(value, range(end))
        worst = max(worst, frac)
        assert fault == 0 and frac <= 1.0, (gamma, frac)
        if gamma == 1.0:
            assert frac == 0.0, "gamma = 1 is the integer statement: s_end - s_i below 2^24 is exact"
    print("discounted sum final=%s: worst |value - exact| = %.3f of 2^-23 M" % (final, worst))


@pytest.mark.parametrize("mode,lam,gamma", [(1, 0.9, 0.999), (1, 0.5, 0.5), (1, 1.0, 0.9), (1, 0.0, 0.9), (0, 0.0, 0.999)])
def test_the_oracle_is_the_definition(mode, lam, gamma):
    """the recurrences over dyadic rationals against the double sums of the definitions over fractions.Fraction, on the episodes
    of 1, 2 and 63 moves (with their tails) and the first rows of one of 130 moves (without)"""
    t = D.table()
    checked = 0
    for e, final, rows in ((0, True, 1), (1, True, 2), (2, True, 63), (5, False, 3)):
        ex = D.Exact(t, mode, lam, gamma, final, True, n_seg=e + 1)
        s, v = D.series(t, e, final, True)
        for i in range(rows):
            value, m = D.forward_sums(s, v, i, mode, lam, gamma)
            j = int(t["seg"][e]) + i
            assert ex.fraction(j) == value and ex.bound(j) == m and m >= abs(value)
            checked += 1
    assert checked == 1 + 2 + 63 + 3


def test_the_defaults_are_the_undiscounted_statement():
    """gamma = 1.0 and v_rows = None: the bits of the statement without them, on the tables of episode_targets_cases.py in all
    modes and weight modes, a bad order entry included"""
    from tetris_mcts_amd import offline as O
    for draw in ("pos", "mixed"):
        for final in (True, False):
            c = K.case(draw, final, 0.0)
            bad = c["order"].copy()
            bad[int(c["seg"][4]) + 100] = len(c["rows"])
            for order in (c["order"], bad):
                for mode, lams in ((0, (0.0,)), (2, (0.0,)), (1, K.LAMBDAS)):
                    for lam in lams:
                        for wmode in (0, 1, 2, 3):
                            args = (c["rows"], order, c["seg"], *c["tail"], mode, lam, wmode, EPS)
                            old, new = O.targets_numpy(*args), O.targets_numpy(*args, gamma=1.0, v_rows=None)
                            assert all(_bits(a, b) for a, b in zip(old[:3], new[:3])) and old[3] == new[3], (draw, final, mode, lam, wmode)


def test_copied_bits_and_refused_arguments_of_the_numpy_statement():
    from tetris_mcts_amd import offline as O
    t = D.table()
    for gamma in D.GAMMAS:
        v2 = _spec(t, 2, 0.0, gamma, True, True, n_seg=D.N_SEG)[0]
        assert _bits(v2, t["v_rows"][t["order"]]), "mode 2 copies v_rows' bits"
        assert _bits(_spec(t, 2, 0.0, gamma, True, False, n_seg=D.N_SEG)[0], t["sorted"]["value"])
    # a value that is not finite stays in its episode (IEEE rules), and is no error
    v = t["v_rows"].copy()
    v[t["order"][int(t["seg"][3]) + 10]] = np.inf
    kind, score, value = D.tails(t, True)
    got = O.targets_numpy(t["rows"], t["order"], t["seg"], kind, score, value, 1, 0.9, 0, EPS, gamma=0.999, v_rows=v)[0]
    a, b = int(t["seg"][3]), int(t["seg"][4])
    assert not np.isfinite(got[a:a + 11]).any() and np.isfinite(got[a + 11:b]).all()
    assert np.isfinite(got[:a]).all() and np.isfinite(got[b:]).all()
    for kw in (dict(gamma=0.0), dict(gamma=1.5), dict(gamma=-0.5), dict(gamma=float("nan"))):
        with pytest.raises(ValueError, match="gamma"):
            O.targets_numpy(t["rows"], t["order"], t["seg"], kind, score, value, 1, 0.9, 0, EPS, **kw)
    with pytest.raises(ValueError, match="mode 0"):
        O.targets_numpy(t["rows"], t["order"], t["seg"], kind, score, value, 0, 0.0, 0, EPS, v_rows=t["v_rows"])
    with pytest.raises(ValueError, match="v_rows"):
        O.targets_numpy(t["rows"], t["order"], t["seg"], kind, score, value, 1, 0.9, 0, EPS, v_rows=t["v_rows"][:-1])


def test_weights_and_variances_come_from_the_rows():
    """v_rows replaces the value column alone: variance and weight are those of the call without it, in every weight mode"""
    t = D.table()
    for wmode in (0, 1, 2, 3):
        with_v, without = _spec(t, 1, 0.9, 0.999, True, True, wmode), _spec(t, 1, 0.9, 1.0, True, False, wmode)
        assert _bits(with_v[1], without[1]) and _bits(with_v[2], without[2])


def refused_discounted_arguments(lib, ptr):
    """every refusal tm_episode_targets_discounted adds to tm_episode_targets' returns hipErrorInvalidValue, and so do those it
    inherits; `ptr`: a non-null, 16-byte aligned address that is never dereferenced"""
    INVALID, p, null = 1, C.c_void_p(ptr), C.c_void_p(0)

    def targets(rows=p, n_rows=10, order=p, seg=p, n_seg=2, kind=p, score=p, value=p, v_rows=null, mode=1, lam=0.5, gamma=0.999,
                wmode=0, out=(p, p, p), fault=p):
        return lib.tm_episode_targets_discounted(rows, n_rows, order, seg, n_seg, kind, score, value, v_rows, mode, lam, gamma, wmode,
                                                 EPS, *out, fault, null)
    for kw in (dict(gamma=0.0), dict(gamma=-0.5), dict(gamma=1.0000001), dict(gamma=float("nan")), dict(gamma=float("inf")),
               dict(v_rows=p, mode=0), dict(v_rows=C.c_void_p(ptr + 2)), dict(v_rows=C.c_void_p(ptr + 1), mode=2),
               # ... and what tm_episode_targets refuses
               dict(n_rows=-1), dict(n_seg=-1), dict(mode=-1), dict(mode=3), dict(wmode=-1), dict(wmode=4), dict(lam=-0.1),
               dict(lam=1.5), dict(lam=float("nan")), dict(rows=null), dict(order=null), dict(seg=null), dict(kind=null),
               dict(score=null), dict(value=null), dict(out=(null, p, p)), dict(out=(p, null, p)), dict(out=(p, p, null)),
               dict(fault=null), dict(rows=C.c_void_p(ptr + 2)), dict(n_rows=2 ** 31 - 1)):
        assert targets(**kw) == INVALID, kw
    # nothing to do is not an error - unless an argument is refused whatever the sizes
    assert targets(n_rows=0, rows=null) == 0 and targets(n_seg=0, seg=null, kind=null) == 0
    assert targets(n_seg=0, gamma=2.0) == INVALID and targets(n_rows=0, v_rows=p, mode=0) == INVALID
    assert targets(n_seg=0, v_rows=p) == 0 and targets(n_seg=0, gamma=1.0) == 0


def test_refused_arguments_without_a_gpu():
    from tetris_mcts_amd import _lib
    buf = (C.c_char * 64)()
    refused_discounted_arguments(_lib.lib(), (C.addressof(buf) + 15) // 16 * 16)


def test_train_cli_new_flags_and_their_refusals():
    cli = _cli()
    d = vars(cli.build_parser().parse_args([]))
    assert d["target_gamma"] == 1.0 and type(d["target_gamma"]) is float
    assert d["bootstrap"] == "recorded" and d["bootstrap_rounds"] == 1 and type(d["bootstrap_rounds"]) is int
    a = cli.build_parser().parse_args(["--target_gamma", "0.999", "--bootstrap", "net", "--bootstrap_rounds", "4"])
    assert (a.target_gamma, a.bootstrap, a.bootstrap_rounds) == (0.999, "net", 4)
    help_text = " ".join(cli.build_parser().format_help().split())
    assert "0.999 is the search's discount" in help_text
    lam = ["--td", "--td_lambda", "0.9"]
    for flags, word in ((["--target_gamma", "0"], "--target_gamma"), (["--target_gamma", "1.01"], "--target_gamma"),
                        (["--target_gamma", "nan"], "--target_gamma"), (["--bootstrap", "net"], "--bootstrap net"),
                        (["--bootstrap", "net", "--td"], "--bootstrap net"), (lam + ["--bootstrap", "net", "--new"], "--new"),
                        (lam + ["--bootstrap", "net", "--bootstrap_rounds", "0"], "--bootstrap_rounds"),
                        (lam + ["--bootstrap_rounds", "2"], "--bootstrap_rounds")):
        with pytest.raises(SystemExit) as e:
            cli.main(flags + ["--data_paths", "x"])
        assert word in str(e.value.code), (flags, e.value.code)
    # what is accepted goes on to the files (there are none)
    for flags in (["--target_gamma", "0.999"], lam + ["--target_gamma", "1.0", "--bootstrap", "recorded", "--bootstrap_rounds", "1"]):
        args = cli.build_parser().parse_args(flags + ["--data_paths", "x"])
        cli.check_args(args)


def test_fit_episodes_refuses_before_it_reads_files():
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model import Model_VV
    model = Model_VV.__new__(Model_VV)          # (the refusals come before the model is used: an empty one will do)
    model.device = "cpu"
    nothing = ["no/such/files*"]
    for kw in (dict(bootstrap="net", td=False), dict(bootstrap="net", td=True), dict(bootstrap="net"),
               dict(bootstrap="net", td=True, lam=0.9, bootstrap_rounds=0), dict(bootstrap="recorded", bootstrap_rounds=2),
               dict(bootstrap="other"), dict(gamma=0.0), dict(gamma=1.5), dict(td=True, lam=0.9, gamma=float("nan"))):
        with pytest.raises(ValueError):
            O.fit_episodes(model, nothing, **kw)
    with pytest.raises(RuntimeError, match="list_of_data is empty"):
        O.fit_episodes(model, nothing, td=True, lam=0.9, gamma=0.999, bootstrap="recorded")
