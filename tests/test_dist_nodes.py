"""Dist node records (csrc/node_records.hip: tm_nodes_drain_dist, tm_node_dist_targets; tetris_mcts_amd/nodes.py;
offline.dist_node_training_set / fit_dist_nodes), what holds without a GPU: the row layout against the header and the value
net's node row, the argument checks of the two calls, the shard writer with its sidecar and the loader, the numpy statement of
tm_node_dist_targets, and the refusals of the two command lines - the new ones, and the old ones with their pointer to the new
route."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

import dist_node_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from tetris_mcts_amd import _lib
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()


def test_dist_node_rows_have_the_headers_layout():
    from tetris_mcts_amd import nodes as N
    d, v = N.NODE_DIST_DTYPE, N.NODE_DTYPE
    assert d.itemsize == N.DIST_ROW_BYTES == int(re.search(r"#define\s+TM_NODE_DIST_ROW_BYTES\s+(\d+)", _header()).group(1)) == 320
    assert d.names == v.names + ("dist",)
    for n in v.names:                                   # the node row's five fields where the node row has them
        assert d.fields[n][:2] == v.fields[n][:2], n
    assert d.fields["dist"][1] == v.itemsize == 64
    dist_row = int(re.search(r"#define\s+TM_DIST_ROW\s+(\d+)", _header()).group(1))
    assert d.fields["dist"][0].base == np.dtype("<f4") and d.fields["dist"][0].shape == (dist_row,) == (K.DIST_ROW,)
    used = np.zeros(320, int)
    for n in d.names:
        f, off = d.fields[n][:2]
        used[off:off + f.itemsize] += 1
    assert used.tolist() == [1] * 320


def test_the_two_calls_are_declared_exported_and_bound():
    L = _lib()
    lib = L.lib()
    declared = set(re.findall(r"\bint\s+(tm_[a-z_0-9]+)\s*\(", _header()))
    for name in ("tm_nodes_drain_dist", "tm_node_dist_targets"):
        assert name in declared and hasattr(lib, name) and name in L.SYMBOLS, name
    assert len(L.SYMBOLS["tm_nodes_drain_dist"]) == 6 and len(L.SYMBOLS["tm_node_dist_targets"]) == 10


def test_the_calls_refuse_bad_arguments_before_any_hip_call():
    buf = (C.c_char * 64)()
    K.refused_dist_node_arguments(_lib(), (C.addressof(buf) + 15) // 16 * 16)


def _want_weight(rows, wmode):
    return rows["visit"].copy() if wmode == 2 else np.ones(len(rows), np.float32)


@pytest.mark.parametrize("atoms", [7, 50, 64])
def test_the_numpy_statement_of_node_dist_targets(atoms):
    from tetris_mcts_amd.nodes import node_dist_targets_numpy
    n = 40
    rows = K.synthetic_rows(n, 5, atoms)
    for wmode in (0, 2):
        obs, target, weight, fault = node_dist_targets_numpy(rows, atoms, wmode)
        assert fault == 0 and obs.tobytes() == rows["obs"].tobytes() and obs.shape == (n, 12)
        assert target.dtype == np.float32 and target.shape == (n, atoms)
        assert target.tobytes() == np.ascontiguousarray(rows["dist"][:, :atoms]).tobytes()
        assert weight.dtype == np.float32 and weight.tobytes() == _want_weight(rows, wmode).tobytes(), wmode
    for wmode in (1, 3, -1, 4):
        with pytest.raises(ValueError, match="weight_mode"):
            node_dist_targets_numpy(rows, atoms, wmode)
    for bad_atoms in (0, 65):
        with pytest.raises(ValueError, match="atoms"):
            node_dist_targets_numpy(rows, bad_atoms, 0)
    # every kind of fault by itself: that row gets weight 0 in both modes, the others keep theirs, the bits are copied all the same
    for kind in K.FAULT_KINDS:
        bad = K.synthetic_rows(n, 5, atoms)
        if not K.inject(bad, 17, kind, atoms):
            assert kind == "beyond" and atoms == 64
            continue
        for wmode in (0, 2):
            obs, target, weight, fault = node_dist_targets_numpy(bad, atoms, wmode)
            assert fault == 1 and weight[17] == 0, (kind, wmode)
            keep = np.arange(n) != 17
            assert weight[keep].tobytes() == _want_weight(bad, wmode)[keep].tobytes(), (kind, wmode)
            assert target.tobytes() == np.ascontiguousarray(bad["dist"][:, :atoms]).tobytes() and obs.tobytes() == bad["obs"].tobytes()
    assert node_dist_targets_numpy(rows[:0], atoms, 2)[3] == 0


def test_a_file_of_more_atoms_than_the_model_is_a_fault():
    from tetris_mcts_amd.nodes import node_dist_targets_numpy
    rows = K.synthetic_rows(10, 1, 50)
    assert node_dist_targets_numpy(rows, 50, 0)[3] == 0 and node_dist_targets_numpy(rows, 64, 0)[3] == 0
    assert node_dist_targets_numpy(rows, 7, 0)[3] == 1


def test_writer_sidecar_and_loader_round_trip(tmp_path):
    from tetris_mcts_amd import nodes as N
    d = str(tmp_path) + "/sub/"                       # (created by the writer)
    w = N.DistNodeShardWriter(d, "distnodes", 3, 50, 0.0, 5000.0)
    assert w.part == 0
    head = np.load(d + "distnodes3.head.npy")
    assert head.dtype == np.float64 and head.tolist() == [50.0, 0.0, 5000.0]
    a, b = K.synthetic_rows(7, 0, 50), K.synthetic_rows(4, 1, 50)
    assert os.path.basename(w.write(a)) == "distnodes3.part00000.npy"
    assert w.write(a[:0]) is None and w.part == 1, "a flush without rows writes no file"
    w.write(b)
    assert sorted(os.listdir(d)) == ["distnodes3.head.npy", "distnodes3.part00000.npy", "distnodes3.part00001.npy"]
    ld = N.DistNodeLoader(d + "distnodes3")
    assert ld.rows.dtype == N.NODE_DIST_DTYPE and ld.length == 11 and ld.rows.tobytes() == a.tobytes() + b.tobytes()
    for c in N.NODE_DIST_DTYPE.names:
        assert np.array_equal(getattr(ld, c), np.concatenate([a[c], b[c]])), c
    assert ld.dist.shape == (11, 64) and ld.dist.dtype == np.float32 and ld.obs.shape == (11, 12)
    assert (ld.atoms, ld.vmin, ld.vmax) == (50, 0.0, 5000.0) and isinstance(ld.atoms, int)
    assert N.DistNodeLoader([d + "distnodes3.part00001.npy", d + "distnodes3.part00000.npy"]).rows.tobytes() == ld.rows.tobytes()
    # opening over existing parts continues the numbering, under the same head
    w2 = N.DistNodeShardWriter(d, "distnodes", 3, 50, 0.0, 5000.0)
    assert w2.part == 2
    # ... and another head's harvest does not go to this stem
    for other in ((64, 0.0, 5000.0), (50, 1.0, 5000.0), (50, 0.0, 100.0)):
        with pytest.raises(ValueError, match="head"):
            N.DistNodeShardWriter(d, "distnodes", 3, *other)
    assert np.load(d + "distnodes3.head.npy").tolist() == [50.0, 0.0, 5000.0], "a refused writer leaves the sidecar alone"
    with pytest.raises(ValueError, match="NODE_DIST_DTYPE"):
        w2.write(np.zeros(3, N.NODE_DTYPE))
    with pytest.raises(ValueError):
        N.DistNodeShardWriter(d, "distnodes", 9, 65, 0.0, 5000.0)
    # the glob of a directory's dist node stems is not disturbed by the sidecar
    from tetris_mcts_amd.offline import choose_stems
    assert choose_stems([d + "distnodes*"], -1) == [d + "distnodes3"]
    # stems whose sidecars disagree, and a stem without one
    N.DistNodeShardWriter(d, "distnodes", 4, 64, 0.0, 5000.0).write(K.synthetic_rows(3, 2, 64))
    with pytest.raises(ValueError, match="disagree"):
        N.DistNodeLoader([d + "distnodes3", d + "distnodes4"])
    assert N.DistNodeLoader([d + "distnodes4"]).atoms == 64
    os.remove(d + "distnodes4.head.npy")
    with pytest.raises(ValueError, match="missing"):
        N.DistNodeLoader([d + "distnodes4"])
    # the two layouts do not load as each other
    import node_cases
    N.NodeShardWriter(d, "nodes", 3).write(node_cases.synthetic_rows(5, 0))
    np.save(d + "nodes3.head.npy", head)
    with pytest.raises(ValueError, match="another layout"):
        N.DistNodeLoader(d + "nodes3")
    with pytest.raises(ValueError, match="another layout"):
        N.NodeLoader(d + "distnodes3")


def test_dist_node_training_set_on_the_host(tmp_path):
    """the numpy route end to end: shards -> [observations, targets, weights], training rows first"""
    import torch
    from tetris_mcts_amd import nodes as N
    from tetris_mcts_amd import offline as O
    d = str(tmp_path) + "/"
    rows = K.synthetic_rows(50, 9, 50)
    w = N.DistNodeShardWriter(d, "distnodes", 0, 50, 0.0, 5000.0)
    w.write(rows[:30])
    w.write(rows[30:])
    data, info = O.dist_node_training_set([d + "distnodes*"], weighted=True, weighted_mode=1, device="cpu")
    assert (info["n"], info["n_val"], info["n_train"], info["validation_fraction"]) == (50, 0, 50, 0.0)
    assert (info["atoms"], info["vmin"], info["vmax"]) == (50, 0.0, 5000.0)
    assert data[0].dtype == torch.int32 and data[0].numpy().tobytes() == rows["obs"].tobytes()
    assert [tuple(x.shape) for x in data] == [(50, 12), (50, 50), (50, 1)]
    assert data[1].numpy().tobytes() == np.ascontiguousarray(rows["dist"][:, :50]).tobytes()
    assert data[2].numpy().tobytes() == rows["visit"].tobytes()
    assert O.dist_node_training_set([d + "distnodes*"], device="cpu")[0][2].numpy().tobytes() == np.ones(50, np.float32).tobytes()
    for mode in (0, 2):
        with pytest.raises(ValueError, match="weighted_mode"):
            O.dist_node_training_set([d + "distnodes*"], weighted=True, weighted_mode=mode, device="cpu")
    g = torch.Generator().manual_seed(3)
    data, info = O.dist_node_training_set([d + "distnodes*"], validation=True, val_set_size=0.2, generator=g, device="cpu")
    assert (info["n"], info["n_val"], info["n_train"]) == (50, 10, 40) and int(50 * info["validation_fraction"]) == 10
    # a permutation of the rows: every row once, distributions with their observations
    key = {r["obs"].tobytes(): r["dist"][:50].tobytes() for r in rows}
    assert sorted(o.tobytes() for o in data[0].numpy().view(np.uint32)) == sorted(key)
    assert all(key[o.tobytes()] == t.tobytes() for o, t in zip(data[0].numpy().view(np.uint32), data[1].numpy()))
    # a row no collection harvests is an error, not a weight of zero
    w.write(K.synthetic_rows(5, 1, 50, faults=[(0, "atom_nan")]))
    with pytest.raises(RuntimeError, match="not rows a collection"):
        O.dist_node_training_set([d + "distnodes*"], device="cpu")


def test_fit_dist_nodes_refusals(tmp_path):
    from tetris_mcts_amd import nodes as N
    from tetris_mcts_amd.offline import fit_dist_nodes

    class Model_VV:
        pass
    with pytest.raises(TypeError, match="Model_Dist"):
        fit_dist_nodes(Model_VV(), ["nothing"])
    from tetris_mcts_amd.model_distributional import Model_Dist
    model = Model_Dist.__new__(Model_Dist)          # (no device: these are refused before anything is touched)
    model.atoms = 64
    for backend in ("torch", "hip"):
        with pytest.raises(ValueError, match="fit_backend='hip_dist'"):
            fit_dist_nodes(model, ["nothing"], fit_backend=backend)
    d = str(tmp_path) + "/"
    N.DistNodeShardWriter(d, "distnodes", 0, 50, 0.0, 5000.0).write(K.synthetic_rows(8, 0, 50))
    with pytest.raises(ValueError, match="50 atoms, the model has 64"):
        fit_dist_nodes(model, [d + "distnodes*"])


def test_fit_nodes_still_refuses_the_head_and_names_the_new_fit():
    from tetris_mcts_amd.offline import fit_nodes

    class Model_Dist:
        pass
    with pytest.raises(TypeError, match="Model_VV") as e:
        fit_nodes(Model_Dist(), ["nothing"])
    assert "not a distribution" in str(e.value) and "fit_dist_nodes" in str(e.value)


def test_the_agent_takes_harvest_and_refuses_it_beside_an_online_fit():
    import inspect
    from tetris_mcts_amd import agents
    assert inspect.signature(agents.DistValueSim.__init__).parameters["harvest"].default is False
    with pytest.raises(ValueError, match="harvest=True"):
        agents.DistValueSim(online=True, harvest=True)


def test_the_recorder_has_no_sweep():
    """close(occupied=True) is refused before the recorder is touched (no GPU: the object is never built)"""
    from tetris_mcts_amd.nodes import DistNodeRecorder, NodeRecorder
    assert issubclass(DistNodeRecorder, NodeRecorder)
    for name in ("drain", "_drain", "_flush", "_write", "_head", "_store"):        # one copy of the scheme
        assert getattr(DistNodeRecorder, name) is getattr(NodeRecorder, name), name
    rec = DistNodeRecorder.__new__(DistNodeRecorder)
    with pytest.raises(ValueError, match="occupied"):
        rec.close(None, occupied=True)


@pytest.mark.parametrize("flags,words", [
    (["--save_dist_nodes"], ["--save_dist_nodes", "--agent_type DistValueSim"]),
    (["--save_dist_nodes", "--agent_type", "ValueSim"], ["--save_dist_nodes", "DistValueSim", "ValueSim"]),
    (["--save_dist_nodes", "--agent_type", "ValueSimLP"], ["--save_dist_nodes", "DistValueSim"]),
    (["--save_dist_nodes", "--agent_type", "ValueSimC"], ["--save_dist_nodes", "DistValueSim"]),
    (["--save_dist_nodes", "--agent_type", "Vanilla"], ["--save_dist_nodes", "DistValueSim"]),
    (["--save_dist_nodes", "--agent_type", "VanillaC"], ["--save_dist_nodes", "DistValueSim"]),
    (["--save_dist_nodes", "--agent_type", "DistValueSim", "--online"], ["--save_dist_nodes", "--online", "same harvest buffers"]),
    (["--save_dist_nodes", "--agent_type", "DistValueSim", "--save_nodes_occupied"], ["--save_dist_nodes", "--save_nodes_occupied",
                                                                                       "no sweep"]),
    (["--save_dist_nodes", "--agent_type", "DistValueSim", "--valuenet_backend", "torch", "--dense_requests"],
     ["--save_dist_nodes", "--dense_requests"]),
    (["--save_dist_nodes", "--agent_type", "DistValueSim", "--min_visit", "0"], ["--min_visit", "--save_dist_nodes"]),
    (["--save_dist_nodes", "--agent_type", "DistValueSim", "--min_visit", "-4"], ["--min_visit", "--save_dist_nodes"]),
    (["--save_dist_nodes", "--agent_type", "DistValueSim", "--save_nodes"], ["--save_dist_nodes", "--save_nodes"]),
    # the old refusal, with its words and the new route
    (["--save_nodes", "--agent_type", "DistValueSim"], ["--save_nodes", "DistValueSim", "another row shape", "--save_dist_nodes"]),
])
def test_play_save_dist_nodes_refusals(flags, words):
    import play
    before = set(sys.modules)
    with pytest.raises(SystemExit) as e:
        play.main(flags)
    for word in words:
        assert word in str(e.value.code), (word, e.value.code)
    assert not any(m == "torch" or m.startswith("tetris_mcts_amd.nodes") or m.startswith("agents.") for m in set(sys.modules) - before), \
        "refused before anything is imported"


def test_play_flag_defaults():
    import play
    a = play.build_parser().parse_args([])
    assert a.save_dist_nodes is False and a.save_nodes is False and a.min_visit == 40


def _cli():
    spec = importlib.util.spec_from_file_location("tm_train_cli_dist_nodes", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("flags,words", [
    (["--dist_nodes", "--nodes", "--td"], ["--dist_nodes", "--nodes"]),
    (["--dist_nodes", "--td", "--td_lambda", "0.5"], ["--dist_nodes", "--td_lambda"]),
    (["--dist_nodes", "--bootstrap", "net"], ["--dist_nodes", "--bootstrap net"]),
    (["--dist_nodes", "--target_gamma", "0.999"], ["--dist_nodes", "--target_gamma"]),
    (["--dist_nodes", "--validation", "--val_mode", "1"], ["--dist_nodes", "--val_mode 1"]),
    (["--dist_nodes", "--ewc", "--ewc_lambda", "1"], ["--dist_nodes", "--ewc"]),
    (["--dist_nodes", "--fit_backend", "torch"], ["--dist_nodes", "--fit_backend torch"]),
    (["--dist_nodes", "--validation", "--validation_backend", "torch"], ["--dist_nodes", "--validation_backend hip"]),
    (["--dist_nodes", "--weighted"], ["--dist_nodes", "--weighted_mode 1"]),
    (["--dist_nodes", "--weighted", "--weighted_mode", "0"], ["--dist_nodes", "--weighted_mode 1"]),
    (["--dist_nodes", "--weighted", "--weighted_mode", "2"], ["--dist_nodes", "--weighted_mode 1"]),
    # the old refusal, with its words and the new route
    (["--nodes", "--td", "--head", "dist"], ["--nodes", "--head dist", "--dist_nodes"]),
])
def test_train_dist_nodes_refusals(flags, words):
    cli = _cli()
    before = set(sys.modules)
    with pytest.raises(SystemExit) as e:
        cli.main(flags + ["--data_paths", "x"])
    for word in words:
        assert word in str(e.value.code), (word, e.value.code)
    assert not any(m.startswith("tetris_mcts_amd.offline") or m == "torch" for m in set(sys.modules) - before), \
        "refused before anything is imported"


@pytest.mark.parametrize("flag,value,have", [("--atoms", "64", "50"), ("--vmin", "1.5", "0.0"), ("--vmax", "4000", "5000.0")])
def test_train_dist_nodes_refuses_a_head_other_than_the_sidecars(tmp_path, flag, value, have):
    from tetris_mcts_amd import nodes as N
    d = str(tmp_path) + "/"
    N.DistNodeShardWriter(d, "distnodes", 0, 50, 0.0, 5000.0).write(K.synthetic_rows(8, 0, 50))
    with pytest.raises(SystemExit) as e:
        _cli().main(["--dist_nodes", "--data_paths", d + "distnodes*", flag, value])
    msg = str(e.value.code)
    assert flag in msg and value in msg and have in msg, msg
