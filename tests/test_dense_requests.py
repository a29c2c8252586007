"""The dense request path for evaluators the engine does not own (csrc/eval_requests.hip), what holds without a GPU: the three
entry points are declared, exported and bound; they check their arguments before the first HIP call; the agents' options are
refused where they mean nothing."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tm_eval_gather", "tm_eval_scatter", "tm_eval_scatter_dist")
INVALID = 1     # hipErrorInvalidValue


def _lib():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from tetris_mcts_amd import _lib
    return _lib


def test_the_three_calls_are_declared_exported_and_bound():
    L = _lib()
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(tm_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in L.SYMBOLS, name
    assert L.SYMBOLS["tm_eval_gather"] == [C.POINTER(L.TmStore), L.i32, L.i32, L.vp, L.vp, L.vp, L.vp]
    assert L.SYMBOLS["tm_eval_scatter"] == [C.POINTER(L.TmStore), L.vp, L.vp, L.vp, L.vp, L.vp]
    assert L.SYMBOLS["tm_eval_scatter_dist"] == [C.POINTER(L.TmStore), L.vp, L.vp, L.vp, L.i32, L.vp]
    share = int(re.search(r"#define\s+TM_EVAL_GATHER_SHARE\s+(\d+)", hdr).group(1))
    assert share >= 256 and share % 256 == 0
    import __graft_entry__ as ge
    assert "eval_requests.hip" in ge.SOURCES


def _store(L, kind=1, bins=50):
    """a store description whose pointers are never followed (every call below is refused before a launch)"""
    s = L.TmStore()
    s.n_games, s.max_nodes, s.eval_slots, s.kind, s.dist_bins = 8, 64, 7 if kind == 1 else 1, kind, bins
    for name in ("eval_obs", "obs_key", "node_game", "eval_v", "eval_var", "eval_dist"):
        setattr(s, name, 4096)
    return s


def test_the_calls_refuse_bad_arguments_before_any_hip_call():
    L = _lib()
    lib = L.lib()
    s, sd = _store(L), _store(L, kind=6)
    p, null = C.c_void_p(4096), C.c_void_p(0)
    g = lib.tm_eval_gather
    assert g(None, 8, 1, p, p, p, null) == INVALID
    assert g(C.byref(s), 8, 1, null, p, p, null) == INVALID
    assert g(C.byref(s), 8, 1, p, null, p, null) == INVALID
    assert g(C.byref(s), 8, 1, p, p, null, null) == INVALID
    for cap, pad in ((0, 1), (-3, 1), (8, 0), (8, -1)):
        assert g(C.byref(s), cap, pad, p, p, p, null) == INVALID, (cap, pad)
    assert g(C.byref(s), 8, 1, C.c_void_p(4098), p, p, null) == INVALID      # rows are stored as dwords
    sc = lib.tm_eval_scatter
    assert sc(None, p, p, p, p, null) == INVALID
    for hole in range(4):
        a = [p, p, p, p]
        a[hole] = null
        assert sc(C.byref(s), *a, null) == INVALID, hole
    sdist = lib.tm_eval_scatter_dist
    assert sdist(None, p, p, p, 64, null) == INVALID
    for hole in range(3):
        a = [p, p, p]
        a[hole] = null
        assert sdist(C.byref(sd), *a, 64, null) == INVALID, hole
    for kind in (0, 1, 2, 3, 4, 5):                                           # TM_KIND_DIST only
        assert sdist(C.byref(_store(L, kind=kind)), p, p, p, 64, null) == INVALID, kind
    assert sdist(C.byref(sd), p, p, p, 49, null) == INVALID                  # dist_stride < dist_bins
    assert sdist(C.byref(sd), p, p, p, 0, null) == INVALID


@pytest.mark.parametrize("name", ["Vanilla", "VanillaC"])
def test_evaluator_pure_is_refused_by_the_vanilla_agents_before_a_store_is_built(name, monkeypatch):
    _lib()
    from tetris_mcts_amd import agents, store as st

    def no_store(*a, **k):
        raise AssertionError("a store was built")
    monkeypatch.setattr(st, "TreeStore", no_store)
    with pytest.raises(ValueError, match="evaluator_pure"):
        getattr(agents, name)(sims=4, n_games=2, max_nodes=64, evaluator_pure=True)


def test_the_options_default_to_todays_path():
    _lib()
    import inspect
    from tetris_mcts_amd.agents.agent import TreeAgent
    sig = inspect.signature(TreeAgent.__init__).parameters
    assert sig["dense_requests"].default is False and sig["evaluator_pure"].default is False and sig["dense_pad"].default == 256
    a = TreeAgent(sims=1)       # (no n_games: no store, no GPU)
    assert (a.dense_requests, a.evaluator_pure, a.dense_pad) == (False, False, 256)
    with pytest.raises(ValueError, match="dense_pad"):
        TreeAgent(sims=1, dense_pad=0)


def test_play_refuses_the_flags_where_the_native_loop_runs():
    import play
    p = play.build_parser()
    assert p.parse_args([]).dense_requests is False and p.parse_args([]).evaluator_pure is False
    for flag in ("--dense_requests", "--evaluator_pure"):
        assert "[new]" in next(a.help for a in p._actions if flag in a.option_strings)
        for argv in (["--agent_type", "ValueSimLP", flag], ["--agent_type", "Vanilla", "--valuenet_backend", "torch", flag]):
            with pytest.raises(SystemExit) as e:
                play.main(argv)
            assert flag in str(e.value.code)
