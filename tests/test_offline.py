"""Offline targets on the host (tetris_mcts_amd/offline.py): the numpy statement of tm_episode_targets against the exact oracle
of episode_targets_cases.py, episode_index on CPU tensors against EpisodeLoader's sort, training_set's layout and split, and the
command line of train.py.  The GPU half is tests/test_gpu_offline.py.

The bound of the lambda-return, |value_i - exact_i| <= 2^-23 M_i with M_i = sum lam^k |term_k| / sum lam^k >= |exact_i|, is
derived, not measured: fp32's half ulp is 2^-24 |exact_i|, the bound allows twice that of M_i; the fp64 accumulation adds at most
some L 2^-52 M_i, nothing beside it for L < 2^20.  A plain fp64 backward recurrence measured 0.50 of it on these tables."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import episode_targets_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 0.001


def _spec(c, mode, lam, wmode, order=None):
    from tetris_mcts_amd import offline as O
    return O.targets_numpy(c["rows"], c["order"] if order is None else order, c["seg"], *c["tail"], mode, lam, wmode, EPS)


def _bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


@pytest.mark.parametrize("draw", ["pos", "mixed"])
@pytest.mark.parametrize("final", [True, False])
def test_monte_carlo_and_copied_values_bit_for_bit(draw, final):
    """mode 0: s_end - s_i in integers, s_end the tail's score or the last row's; mode 2 and the variance column: the bits"""
    c = K.case(draw, final, 0.0)
    rows, order, seg = c["rows"], c["order"], c["seg"]
    kind, tscore, _ = c["tail"]
    assert kind.sum() == (len(c["episodes"]) if final else 0)
    want = np.zeros(len(order), np.float32)
    for e in range(len(seg) - 1):
        pos = order[seg[e]:seg[e + 1]]
        s_end = int(tscore[e]) if kind[e] else int(rows["score"][pos[-1]])
        want[seg[e]:seg[e + 1]] = [np.float32(s_end - int(s)) for s in rows["score"][pos]]
    v0, var0, w0, fault = _spec(c, 0, 0.0, 0)
    assert fault == 0 and _bits(v0, want) and _bits(var0, rows["variance"][order]) and _bits(w0, np.ones(len(order)))
    v2, var2, _, _ = _spec(c, 2, 0.0, 0)
    assert _bits(v2, rows["value"][order]) and _bits(var2, rows["variance"][order])


@pytest.mark.parametrize("draw", ["pos", "mixed"])
@pytest.mark.parametrize("final", [True, False])
@pytest.mark.parametrize("lam", K.LAMBDAS)
def test_lambda_return_within_the_derived_bound(draw, final, lam):
    c = K.case(draw, final, lam)
    value, var, _, fault = _spec(c, 1, lam, 0)
    frac = c["exact"].bound_fraction(value)
    print("lambda-return %s final=%s lam=%s: worst |value - exact| = %.3f of 2^-23 M" % (draw, final, lam, frac))
    assert fault == 0 and frac <= 1.0
    assert _bits(var, c["rows"]["variance"][c["order"]])
    if lam == 0.0:
        assert _bits(value, c["rows"]["value"][c["order"]]), "lambda = 0 is v_i itself"


def test_the_oracle_is_the_forward_loop():
    """the scaled-integer oracle against the reference's loop written over fractions.Fraction, on the short episodes"""
    from fractions import Fraction
    c = K.case("mixed", True, 0.9)
    rows, order, seg = c["rows"], c["order"], c["seg"]
    kind, tscore, tvalue = c["tail"]
    lam, checked = Fraction(0.9), 0
    for e in range(len(seg) - 1):
        if seg[e + 1] - seg[e] > 65:
            continue
        s = [Fraction(int(rows["score"][j])) for j in order[seg[e]:seg[e + 1]]] + ([Fraction(int(tscore[e]))] if kind[e] else [])
        v = [Fraction(float(rows["value"][j])) for j in order[seg[e]:seg[e + 1]]] + ([Fraction(float(tvalue[e]))] if kind[e] else [])
        for i in range(seg[e + 1] - seg[e]):
            idx_r, weight, _sum, _weight_sum = i, Fraction(1), Fraction(0), Fraction(0)
            while idx_r < len(s):
                _sum += weight * (s[idx_r] + v[idx_r] - s[i])
                _weight_sum += weight
                idx_r += 1
                weight *= lam
            assert c["exact"].fraction(seg[e] + i) == _sum / _weight_sum
            checked += 1
    assert checked >= 1 + 2 + 5 + 63 + 64 + 65


def test_weights():
    c = K.case("pos", True, 0.0)
    rows, order = c["rows"], c["order"]
    var = rows["variance"][order]
    visits = rows["child_stats"][order][:, 0, :]
    exact_sum = visits.astype(np.float64).sum(1)                      # integer-valued floats below 2^24: the sum is exact
    assert (exact_sum == np.round(exact_sum)).all() and exact_sum.max() < 2 ** 24
    w1, w2, w3 = (_spec(c, 2, 0.0, m)[2] for m in (1, 2, 3))
    assert _bits(w1, np.float32(1) / (var + np.float32(EPS)))
    assert _bits(w2, exact_sum.astype(np.float32))
    assert _bits(w3, exact_sum.astype(np.float32) / (var + np.float32(EPS)))


def test_a_bad_order_entry_reads_nothing():
    """an entry equal to n_rows and one equal to -1: zeros, weight 0 and the fault flag there; the row is left out of its
    episode's series, so every other episode is unchanged, and so are the copied columns everywhere else"""
    c = K.case("pos", True, 0.9)
    n = len(c["rows"])
    bad = [int(c["seg"][4]) + 100, int(c["seg"][7]) - 1]              # inside a 300-move episode; the last row of another one
    order = c["order"].copy()
    order[bad[0]], order[bad[1]] = n, -1
    others = np.ones(n, bool)
    others[bad] = False
    for mode in (0, 1, 2):
        clean, got = _spec(c, mode, 0.9, 3), _spec(c, mode, 0.9, 3, order)
        assert clean[3] == 0 and got[3] == 1
        for a, b in zip(clean[:3], got[:3]):
            assert not b[bad].any()
            same = others.copy()
            if mode != 2 and a is clean[0]:                           # the values of the two episodes that lost a row may move
                same[c["seg"][4]:c["seg"][5]] = False
                same[c["seg"][6]:c["seg"][7]] = False
            assert _bits(a[same], b[same])
    # the episode that lost row 100: the rows behind it are untouched, the ones before it see the series without it
    clean, got = _spec(c, 1, 0.9, 0)[0], _spec(c, 1, 0.9, 0, order)[0]
    a, b = int(c["seg"][4]), int(c["seg"][5])
    assert _bits(clean[bad[0] + 1:b], got[bad[0] + 1:b]) and not _bits(clean[a:bad[0]], got[a:bad[0]])
    keep = np.delete(np.arange(n), bad[0])
    short = np.delete(order, bad[0])
    seg = c["seg"].copy()
    seg[5:] -= 1
    from tetris_mcts_amd import offline as O
    without = O.targets_numpy(c["rows"], short, seg, *c["tail"], 1, 0.9, 0, EPS)[0]
    assert _bits(without[a:bad[0]], got[a:bad[0]]) and len(keep) == len(without)


def _stems(tmp_path):
    """two stems with colliding rank-local ids, two parts each"""
    out = []
    for k, draw in enumerate(("pos", "mixed")):
        rows, ep = K.make_table(draw, seed=k)
        stem = os.path.join(str(tmp_path), "data%d.r%d" % (K.CYCLE, k))
        K.write_shards(stem, rows, ep)
        os.utime(stem + ".part00001.npy", (1000 + k, 1000 + k))      # the order train.py sorts by
        os.utime(stem + ".part00000.npy", (900 + k, 900 + k))
        out.append(stem)
    return out


def test_episode_index_on_cpu_tensors(tmp_path):
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.episodes import EpisodeLoader
    stems = _stems(tmp_path)
    # one stem: the segments of EpisodeLoader(by_episode=True)
    ld = EpisodeLoader(stems[0], by_episode=True)
    table, stem_rows, ep, ep_stems = O.load_stems(stems[:1])
    idx = O.episode_index(O.rows_tensor(table), stem_rows, ep, ep_stems)
    raw = table.view(np.uint8).reshape(len(table), -1)                # (whole rows as bytes: the pad bytes travel too)
    assert raw[idx.order.numpy()].tobytes() == ld.rows.tobytes()
    key = np.stack([ld.cycle, ld.episode], 1)
    starts = np.nonzero(np.append(True, (key[1:] != key[:-1]).any(1)))[0]
    assert idx.seg.tolist() == starts.tolist() + [ld.length]
    named = set(ld.episodes["episode"].tolist())
    assert [bool(x) for x in idx.ended] == [int(e) in named for e in idx.episode]
    assert int((~idx.ended).sum()) == K.G and len(named) == len(ld.episodes) == 11
    final = {int(e["episode"]): int(e["score"]) for e in ld.episodes}
    assert [int(s) for s, e in zip(idx.final_score, idx.ended) if e] == [final[int(i)] for i, e in zip(idx.episode, idx.ended) if e]
    # two stems: the same ids twice, kept apart
    table, stem_rows, ep, ep_stems = O.load_stems(stems)
    both = O.episode_index(O.rows_tensor(table), stem_rows, ep, ep_stems)
    n_seg = len(idx.ended)
    assert len(both.ended) == 2 * n_seg and both.stem.tolist() == [0] * n_seg + [1] * n_seg
    assert both.episode[:n_seg].tolist() == both.episode[n_seg:].tolist()
    assert both.seg[:n_seg + 1].tolist() == idx.seg.tolist() and (both.order[:stem_rows[0]] < stem_rows[0]).all()
    assert (both.order[stem_rows[0]:] >= stem_rows[0]).all()
    for k in (0, 1):
        mine = [int(s) for s, e, st in zip(both.final_score, both.ended, both.stem) if e and st == k]
        table_k = {int(e["episode"]): int(e["score"]) for e in ep[ep_stems == k]}
        assert mine == [table_k[int(i)] for i, e, st in zip(both.episode, both.ended, both.stem) if e and st == k]
    # an episode table that lost a row: exactly that episode becomes censored
    fewer = O.episode_index(O.rows_tensor(table), stem_rows, ep[1:], ep_stems[1:])
    lost = (both.ended != fewer.ended).nonzero().flatten().tolist()
    assert len(lost) == 1 and (int(both.stem[lost[0]]), int(both.episode[lost[0]])) == (int(ep_stems[0]), int(ep["episode"][0]))


def test_training_set_layout_and_split(tmp_path):
    from tetris_mcts_amd import offline as O
    stems = _stems(tmp_path)
    pattern = os.path.join(str(tmp_path), "data*")
    assert O.choose_stems([pattern], 1) == stems[1:] and O.choose_stems([pattern], -1) == stems
    assert O.choose_stems([stems[0]], 1) == stems[:1] and O.choose_stems([str(tmp_path)], 2) == stems
    with pytest.raises(RuntimeError, match="list_of_data is empty"):
        O.choose_stems([os.path.join(str(tmp_path), "nothing*")], 1)
    table, stem_rows, ep, ep_stems = O.load_stems(stems[:1])
    idx = O.episode_index(O.rows_tensor(table), stem_rows, ep, ep_stems)
    length = np.diff(idx.seg.numpy())
    ended_row = np.repeat(idx.ended.numpy(), length)
    episode_row = np.repeat(idx.episode.numpy(), length)
    sorted_rows = table[idx.order.numpy()]
    # mode 1, val_mode 1: nothing is dropped; the rows of episodes 0 .. 5 are held out, and they are last
    data, info = O.training_set([stems[0]], td=True, lam=0.9, validation=True, val_mode=1, val_episodes=5, device="cpu")
    held = episode_row < 6
    assert info["n"] == len(table) and info["n_val"] == int(held.sum()) > 0 and info["censored_episodes"] == K.G
    want = np.concatenate([sorted_rows[~held], sorted_rows[held]])
    assert data[0].shape == (len(table), 1, 20, 10) and data[0].dtype == torch.float32
    assert np.array_equal(data[0].numpy().reshape(-1, 20, 10), want["board"].astype(np.float32))
    assert _bits(data[2].numpy().reshape(-1), want["variance"])
    assert int(info["n"] * info["validation_fraction"]) == info["n_val"]
    value = O.episode_targets(table, idx, td=True, lam=0.9, device="cpu")[0].numpy()
    assert _bits(data[1].numpy().reshape(-1), np.concatenate([value[~held], value[held]]))
    assert all(d.shape == (info["n"], 1) for d in data[1:])
    # mode 0: censored="drop" removes exactly the censored rows, "keep" none; terminal="rows" ends at the last row
    data0, info0 = O.training_set([stems[0]], device="cpu")
    assert info0["n"] == int(ended_row.sum()) < len(table) and info0["n_val"] == 0 and info0["validation_fraction"] == 0.0
    assert np.array_equal(data0[0].numpy().reshape(-1, 20, 10), sorted_rows[ended_row]["board"].astype(np.float32))
    final = {int(e["episode"]): int(e["score"]) for e in ep}
    assert data0[1].reshape(-1).tolist() == [float(final[int(e)] - int(s)) for e, s in zip(episode_row[ended_row], sorted_rows[ended_row]["score"])]
    keep0, _ = O.training_set([stems[0]], censored="keep", terminal="rows", device="cpu")
    assert keep0[0].shape[0] == len(table)
    last_score = np.repeat(sorted_rows["score"][idx.seg.numpy()[1:] - 1], length)
    assert keep0[1].reshape(-1).tolist() == (last_score - sorted_rows["score"]).astype(np.float32).tolist()
    # val_mode 0: a random fraction, capped
    g = torch.Generator().manual_seed(3)
    d, i = O.training_set([stems[0]], td=True, validation=True, val_set_size=0.25, generator=g, device="cpu")
    assert i["n_val"] == len(table) // 4 and i["n"] == len(table)
    boards = {r.tobytes() for r in d[0].numpy().reshape(len(table), -1)}
    assert len(boards) == len({r["board"].tobytes() for r in table}) == len(table), "every row once"
    d, i = O.training_set([stems[0]], td=True, validation=True, val_set_size=0.25, val_set_size_max=17, device="cpu")
    assert i["n_val"] == 17
    # weights reach the data
    dw, _ = O.training_set([stems[0]], td=True, weighted=True, weighted_mode=1, device="cpu")
    assert dw[3].reshape(-1).tolist() == sorted_rows["child_stats"][:, 0, :].astype(np.float64).sum(1).tolist()


def test_validation_fraction_gives_n_val_exactly():
    """train_data splits with int(n * fraction): (n_val + 0.5) / n lands on n_val for every n up to 5 000 and every n_val <= n"""
    from tetris_mcts_amd.offline import validation_fraction
    assert validation_fraction(10, 0) == 0.0
    for n in range(1, 5001):
        f = (np.arange(0, n + 1) + 0.5) / n                           # the same double arithmetic, all n_val at once
        assert ((n * f).astype(np.int64) == np.arange(0, n + 1)).all(), n
    for n, k in ((1, 1), (7, 3), (4999, 4999), (5000, 1), (5000, 2500)):
        assert int(n * validation_fraction(n, k)) == k


def _cli():
    """train.py by path under another name: nothing imports a top-level module named `train`"""
    spec = importlib.util.spec_from_file_location("tm_train_cli", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_cli_keeps_the_reference_flags():
    """train.py:15-39 of the reference: the flags this engine gives a meaning keep their types and defaults"""
    cli = _cli()
    ref = dict(batch_size=32, cycle=-1, data_paths=[], early_stopping=False, early_stopping_patience=10, epochs=10, ewc=False,
               last_nfiles=1, min_iters=-1, max_iters=-1, new=False, validation=False, val_episodes=0, val_mode=0,
               val_set_size=0.05, val_set_size_max=-1, val_total=25, save_loss=False, td=False, weighted=False, weighted_mode=0)
    d = vars(cli.build_parser().parse_args([]))
    for k, v in ref.items():
        assert d[k] == v and type(d[k]) is type(v), k
    assert d["td_lambda"] is None and d["terminal"] == "final" and d["censored"] == "drop" and d["fit_backend"] == "hip"
    a = cli.build_parser().parse_args(["--data_paths", "a*", "b*", "--td", "--td_lambda", "0.9", "--val_episodes", "5"])
    assert a.data_paths == ["a*", "b*"] and a.td_lambda == 0.9 and a.val_episodes == 5.0
    # the reference's iteration count (train.py:193-203)
    a = cli.build_parser().parse_args(["--epochs", "50", "--min_iters", "20000"])
    assert cli.iterations(a, 1000) == (20000, 20000 // 25 + 1)
    a = cli.build_parser().parse_args(["--epochs", "3", "--max_iters", "40", "--batch_size", "10"])
    assert cli.iterations(a, 1000) == (40, 40 // 25 + 1) and cli.iterations(a, 95) == (27, 2)


@pytest.mark.parametrize("flags,word", [(["--ewc"], "Fisher"), (["--save_loss"], "HDF5"), (["--td_lambda", "0.5"], "--td"),
                                        (["--td", "--td_lambda", "1.5"], "[0, 1]"), ([], "list_of_data is empty")])
def test_train_cli_refusals(flags, word):
    cli = _cli()
    with pytest.raises(SystemExit) as e:
        cli.main(flags + ([] if word == "list_of_data is empty" else ["--data_paths", "x"]))
    assert word in str(e.value.code)


def test_the_distributional_head_is_refused():
    from tetris_mcts_amd.offline import fit_episodes

    class Model_Dist:          # (fit_episodes looks at the class before it looks at anything else)
        pass
    with pytest.raises(TypeError, match="no episode target for a distribution"):
        fit_episodes(Model_Dist(), ["nothing"])
    with pytest.raises(ValueError):
        from tetris_mcts_amd.offline import target_mode
        target_mode(True, 1.5)


def test_nothing_imports_a_top_level_train():
    """train.py at the root shadows nothing: no Python file of the repository imports a top-level module named `train`"""
    import ast
    sources = [os.path.join(ROOT, f) for f in os.listdir(ROOT) if f.endswith(".py")]
    for top in ("agents", "tetris_mcts_amd", "scripts", "tests", "oracle"):
        for base, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [d for d in dirs if not d.startswith((".", "_"))]          # (build directories and caches)
            sources += [os.path.join(base, f) for f in files if f.endswith(".py")]
    assert len(sources) > 60
    for path in sources:
        for node in ast.walk(ast.parse(open(path).read())):
            if isinstance(node, ast.Import):
                assert all(a.name.split(".")[0] != "train" for a in node.names), path
            if isinstance(node, ast.ImportFrom) and node.level == 0:
                assert (node.module or "").split(".")[0] != "train", path


def refused_arguments(lib, ptr):
    """every refusal of the two calls returns hipErrorInvalidValue; `ptr`: a non-null, 16-byte aligned address that is never
    dereferenced (the checks come before the first HIP call)"""
    import ctypes as C
    INVALID, p, null = 1, C.c_void_p(ptr), C.c_void_p(0)

    def targets(rows=p, n_rows=10, order=p, seg=p, n_seg=2, kind=p, score=p, value=p, mode=1, lam=0.5, wmode=0, out=(p, p, p), fault=p):
        return lib.tm_episode_targets(rows, n_rows, order, seg, n_seg, kind, score, value, mode, lam, wmode, EPS, *out, fault, null)
    for kw in (dict(n_rows=-1), dict(n_seg=-1), dict(mode=-1), dict(mode=3), dict(wmode=-1), dict(wmode=4), dict(lam=-0.1),
               dict(lam=1.5), dict(lam=float("nan")), dict(rows=null), dict(order=null), dict(seg=null), dict(kind=null),
               dict(score=null), dict(value=null), dict(out=(null, p, p)), dict(out=(p, null, p)), dict(out=(p, p, null)),
               dict(fault=null), dict(rows=C.c_void_p(ptr + 2)), dict(n_rows=2 ** 31 - 1)):
        assert targets(**kw) == INVALID, kw
    # nothing to do is not an error - unless an argument is refused whatever the sizes
    assert targets(n_rows=0, rows=null) == 0 and targets(n_seg=0, seg=null, kind=null) == 0
    assert targets(n_seg=0, mode=3) == INVALID and targets(n_rows=0, lam=2.0) == INVALID

    def gather(rows=p, n_rows=10, idx=p, n=3, out=p, fault=p):
        return lib.tm_episode_gather_states(rows, n_rows, idx, n, out, fault, null)
    for kw in (dict(n_rows=-1), dict(n=-1), dict(rows=null), dict(idx=null), dict(out=null), dict(fault=null),
               dict(rows=C.c_void_p(ptr + 1)), dict(out=C.c_void_p(ptr + 4))):
        assert gather(**kw) == INVALID, kw
    assert gather(n=0, idx=null, out=null) == 0


def test_refused_arguments_without_a_gpu():
    import ctypes as C
    from tetris_mcts_amd import _lib
    buf = (C.c_char * 64)()
    refused_arguments(_lib.lib(), (C.addressof(buf) + 15) // 16 * 16)
