"""Node records (csrc/node_records.hip, tetris_mcts_amd/nodes.py, offline.node_training_set / fit_nodes), what holds without a
GPU: the row layout against the header, the argument checks of the three calls, the shard writer and the loader, the numpy
statement of tm_node_targets, and the refusals of the two command lines."""
import ctypes as C
import importlib.util
import io
import os
import re

import numpy as np
import pytest

import node_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 0.001


def _lib():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from tetris_mcts_amd import _lib
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()


def test_node_rows_have_the_headers_layout():
    from tetris_mcts_amd import nodes as N
    d = N.NODE_DTYPE
    assert d.itemsize == N.ROW_BYTES == int(re.search(r"#define\s+TM_NODE_ROW_BYTES\s+(\d+)", _header()).group(1)) == 64
    assert d.names == ("obs", "value", "variance", "visit", "slot")
    assert {n: d.fields[n][1] for n in d.names} == dict(obs=0, value=48, variance=52, visit=56, slot=60)
    assert d.fields["obs"][0].base == np.dtype("<u4") and d.fields["obs"][0].shape == (12,)
    assert [d.fields[n][0] for n in d.names[1:]] == [np.dtype("<f4")] * 3 + [np.dtype("<i4")]
    used = np.zeros(64, int)
    for n in d.names:
        f, off = d.fields[n][:2]
        used[off:off + f.itemsize] += 1
    assert used.tolist() == [1] * 64
    # the first 60 bytes are the harvest's tuple: the observation of TM_OBS_DW words, then replay_stat's value, variance, visit
    assert int(re.search(r"#define\s+TM_OBS_DW\s+(\d+)", _header()).group(1)) * 4 == d.fields["value"][1]


def test_the_three_calls_are_declared_exported_and_bound():
    L = _lib()
    lib = L.lib()
    declared = set(re.findall(r"\bint\s+(tm_[a-z_0-9]+)\s*\(", _header()))
    for name in ("tm_nodes_drain", "tm_nodes_sweep", "tm_node_targets"):
        assert name in declared and hasattr(lib, name) and name in L.SYMBOLS, name
    import __graft_entry__ as ge
    assert "node_records.hip" in ge.SOURCES


def test_the_calls_refuse_bad_arguments_before_any_hip_call():
    buf = (C.c_char * 64)()
    K.refused_node_arguments(_lib(), (C.addressof(buf) + 15) // 16 * 16)


def test_writer_and_loader_round_trip(tmp_path):
    from tetris_mcts_amd import nodes as N
    d = str(tmp_path) + "/sub/"                       # (created by the writer)
    w = N.NodeShardWriter(d, "nodes", 3)
    assert w.part == 0
    a, b = K.synthetic_rows(7, 0), K.synthetic_rows(4, 1)
    assert os.path.basename(w.write(a)) == "nodes3.part00000.npy"
    assert w.write(a[:0]) is None and w.part == 1, "a flush without rows writes no file"
    w.write(b)
    assert sorted(os.listdir(d)) == ["nodes3.part00000.npy", "nodes3.part00001.npy"]
    ld = N.NodeLoader(d + "nodes3")
    assert ld.rows.dtype == N.NODE_DTYPE and ld.length == 11 and ld.rows.tobytes() == a.tobytes() + b.tobytes()
    for c in N.NODE_DTYPE.names:
        assert np.array_equal(getattr(ld, c), np.concatenate([a[c], b[c]])), c
    assert ld.obs.shape == (11, 12) and ld.obs.dtype == np.uint32
    # the shards named one by one, in any order, give the same table
    assert N.NodeLoader([d + "nodes3.part00001.npy", d + "nodes3.part00000.npy"]).rows.tobytes() == ld.rows.tobytes()
    # opening over existing parts continues the numbering
    w2 = N.NodeShardWriter(d, "nodes", 3)
    assert w2.part == 2
    w2.write(a[:2])
    assert os.path.exists(d + "nodes3.part00002.npy") and N.NodeLoader([d + "nodes3"]).length == 13
    # another cycle and another rank are other stems
    assert N.NodeShardWriter(d, "nodes", 4).part == 0 and N.NodeShardWriter(d, "nodes", 3, rank=1).stem.endswith("nodes3.r1")
    with pytest.raises(ValueError, match="NODE_DTYPE"):
        w2.write(np.zeros(3, np.float32))
    # an episode shard is not a node shard
    from tetris_mcts_amd.episodes import STATE_DTYPE
    np.save(d + "data3.part00000.npy", np.zeros(2, STATE_DTYPE))
    with pytest.raises(ValueError, match="another layout"):
        N.NodeLoader(d + "data3")


def test_choose_stems_over_node_shards(tmp_path):
    from tetris_mcts_amd import nodes as N
    from tetris_mcts_amd.offline import choose_stems
    d = str(tmp_path) + "/"
    for cycle, t in ((1, 100), (2, 200), (3, 300)):
        w = N.NodeShardWriter(d, "nodes", cycle)
        name = w.write(K.synthetic_rows(3, cycle))
        os.utime(name, (t, t))
    assert choose_stems([d + "nodes*"], 2) == [d + "nodes2", d + "nodes3"]
    assert choose_stems([d + "nodes*"], -1) == [d + "nodes1", d + "nodes2", d + "nodes3"]


def test_loss_is_reported_with_the_counts_and_what_to_raise():
    from tetris_mcts_amd.nodes import report_loss
    out = io.StringIO()
    report_loss(0, 0, 100, 5, out=out)
    assert out.getvalue() == ""
    report_loss(7, 0, 100, 5, out=out)
    assert "7 node rows" in out.getvalue() and "ring_rows=100" in out.getvalue() and "replay_cap" not in out.getvalue()
    out = io.StringIO()
    report_loss(0, 9, 100, 5, out=out)
    assert "9 harvested tuples" in out.getvalue() and "replay_cap=5" in out.getvalue() and "raise replay_cap" in out.getvalue()


def _f32(x):
    return np.asarray(x, np.float32)


def test_the_numpy_statement_of_node_targets():
    from tetris_mcts_amd.nodes import node_targets_numpy
    rows = K.synthetic_rows(40, 5)
    var, visit, one, eps = rows["variance"], rows["visit"], np.float32(1), np.float32(EPS)
    want = {0: np.ones(40, np.float32), 1: one / (var + eps), 2: visit.copy(), 3: visit / (var + eps)}
    for wmode in range(4):
        obs, value, variance, weight, fault = node_targets_numpy(rows, wmode, EPS)
        assert fault == 0 and obs.tobytes() == rows["obs"].tobytes() and obs.shape == (40, 12)
        assert value.tobytes() == rows["value"].tobytes() and variance.tobytes() == rows["variance"].tobytes()
        assert weight.dtype == np.float32 and weight.tobytes() == want[wmode].astype(np.float32).tobytes(), wmode
    assert want[1][1] == np.float32(1) / np.float32(EPS), "a variance of 0 is no fault: eps keeps the weight finite"
    with pytest.raises(ValueError):
        node_targets_numpy(rows, 4, EPS)
    # the fault cases: such a row gets weight 0 in every mode, the others keep theirs, the bits of value and variance are copied
    nan, inf = np.float32("nan"), np.float32("inf")
    for col, v in (("value", nan), ("value", inf), ("value", -inf), ("variance", nan), ("variance", inf), ("visit", 0.0),
                   ("visit", 0.5), ("visit", -3.0), ("visit", nan)):
        bad = K.synthetic_rows(40, 5, faults=[(17, col, v)])
        for wmode in range(4):
            _, value, variance, weight, fault = node_targets_numpy(bad, wmode, EPS)
            assert fault == 1 and weight[17] == 0, (col, v, wmode)
            keep = np.arange(40) != 17
            assert weight[keep].tobytes() == want[wmode][keep].astype(np.float32).tobytes(), (col, v, wmode)
            assert value.tobytes() == bad["value"].tobytes() and variance.tobytes() == bad["variance"].tobytes()
    assert node_targets_numpy(rows[:0], 3, EPS)[4] == 0


def test_node_training_set_on_the_host(tmp_path):
    """the numpy route end to end: shards -> [observations, values, variances, weights], training rows first"""
    import torch
    from tetris_mcts_amd import nodes as N
    from tetris_mcts_amd import offline as O
    d = str(tmp_path) + "/"
    rows = K.synthetic_rows(50, 9)
    w = N.NodeShardWriter(d, "nodes", 0)
    w.write(rows[:30])
    w.write(rows[30:])
    data, info = O.node_training_set([d + "nodes*"], weighted=True, weighted_mode=1, device="cpu")
    assert (info["n"], info["n_val"], info["n_train"], info["validation_fraction"]) == (50, 0, 50, 0.0)
    assert data[0].dtype == torch.int32 and data[0].numpy().tobytes() == rows["obs"].tobytes()
    assert [tuple(x.shape) for x in data] == [(50, 12), (50, 1), (50, 1), (50, 1)]
    assert data[1].numpy().tobytes() == rows["value"].tobytes() and data[3].numpy().tobytes() == rows["visit"].tobytes()
    g = torch.Generator().manual_seed(3)
    data, info = O.node_training_set([d + "nodes*"], validation=True, val_set_size=0.2, generator=g, device="cpu")
    assert (info["n"], info["n_val"], info["n_train"]) == (50, 10, 40) and int(50 * info["validation_fraction"]) == 10
    # a permutation of the rows: every row once, values with their observations
    key = {r["obs"].tobytes(): r["value"] for r in rows}
    assert sorted(o.tobytes() for o in data[0].numpy().view(np.uint32)) == sorted(key)
    assert all(key[o.tobytes()] == v for o, v in zip(data[0].numpy().view(np.uint32), data[1].numpy().reshape(-1)))
    # a row no collection harvests is an error, not a weight of zero that meets a NaN in the loss
    w.write(K.synthetic_rows(5, 1, faults=[(0, "value", np.float32("nan"))]))
    with pytest.raises(RuntimeError, match="not finite"):
        O.node_training_set([d + "nodes*"], device="cpu")


def test_fit_nodes_refusals():
    from tetris_mcts_amd.offline import fit_nodes

    class Model_Dist:
        pass
    with pytest.raises(TypeError, match="Model_VV"):
        fit_nodes(Model_Dist(), ["nothing"])
    from tetris_mcts_amd.model import Model_VV
    model = Model_VV.__new__(Model_VV)              # (no device: the backend is refused before anything is touched)
    with pytest.raises(ValueError, match="fit_backend='hip'"):
        fit_nodes(model, ["nothing"], fit_backend="torch")


def test_the_agents_take_harvest_and_refuse_it_beside_an_online_fit():
    import inspect
    from tetris_mcts_amd import agents
    sig = inspect.signature(agents.ValueSim.__init__).parameters
    assert sig["harvest"].default is False
    for name in ("ValueSim", "ValueSimLP", "ValueSimC"):
        with pytest.raises(ValueError, match="harvest=True"):
            getattr(agents, name)(online=True, harvest=True)


@pytest.mark.parametrize("flags,words", [
    (["--save_nodes"], ["--save_nodes", "--agent_type"]),
    (["--save_nodes", "--agent_type", "Vanilla"], ["--save_nodes", "Vanilla", "untested"]),
    (["--save_nodes", "--agent_type", "VanillaC"], ["--save_nodes", "VanillaC", "untested"]),
    (["--save_nodes", "--agent_type", "DistValueSim"], ["--save_nodes", "DistValueSim", "another row shape"]),
    (["--save_nodes", "--agent_type", "ValueSim", "--online"], ["--save_nodes", "--online", "same harvest buffers"]),
    (["--save_nodes", "--agent_type", "ValueSim", "--valuenet_backend", "torch", "--dense_requests"],
     ["--save_nodes", "--dense_requests"]),
    (["--save_nodes_occupied", "--agent_type", "ValueSim"], ["--save_nodes_occupied", "--save_nodes"]),
    (["--save_nodes", "--agent_type", "ValueSim", "--min_visit", "0"], ["--min_visit", "--save_nodes"]),
    (["--save_nodes", "--save_tree", "--agent_type", "ValueSim"], ["--save_tree"]),
])
def test_play_save_nodes_refusals(flags, words):
    import play
    with pytest.raises(SystemExit) as e:
        play.main(flags)
    for word in words:
        assert word in str(e.value.code), (word, e.value.code)


def test_play_min_visit_keeps_its_help_and_default():
    import play
    p = play.build_parser()
    a = p.parse_args([])
    assert a.min_visit == 40 and a.save_nodes is False and a.save_nodes_occupied is False
    assert "Minimum visits for node storage" in p.format_help()


def _cli():
    spec = importlib.util.spec_from_file_location("tm_train_cli_nodes", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("flags,words", [
    (["--nodes"], ["--nodes", "--td"]),
    (["--nodes", "--td", "--td_lambda", "0.5"], ["--nodes", "--td_lambda"]),
    (["--nodes", "--td", "--bootstrap", "net"], ["--nodes", "--bootstrap net"]),
    (["--nodes", "--td", "--target_gamma", "0.999"], ["--nodes", "--target_gamma"]),
    (["--nodes", "--td", "--validation", "--val_mode", "1"], ["--nodes", "--val_mode 1"]),
    (["--nodes", "--td", "--head", "dist"], ["--nodes", "--head dist"]),
    (["--nodes", "--td", "--fit_backend", "torch"], ["--nodes", "--fit_backend torch"]),
    (["--nodes", "--td", "--validation", "--validation_backend", "torch"], ["--nodes", "--validation_backend hip"]),
])
def test_train_nodes_refusals(flags, words, monkeypatch):
    import sys
    cli = _cli()
    before = set(sys.modules)
    with pytest.raises(SystemExit) as e:
        cli.main(flags + ["--data_paths", "x"])
    for word in words:
        assert word in str(e.value.code), (word, e.value.code)
    assert not any(m.startswith("tetris_mcts_amd.offline") or m == "torch" for m in set(sys.modules) - before), \
        "refused before anything is imported"
