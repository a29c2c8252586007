"""tm_sim_step's choice of tree kernel (tree.hip: one kernel per agent family) as the pure function of (kind, eval_cap) it is:
tm_sim_step_kernel, host code only.  Every kind the store knows maps to exactly one kernel, TM_KIND_DIST never to the capped one,
and a cap on a kind that can not carry one is refused - by the function (-1) and by tm_sim_step itself (hipErrorInvalidValue),
which returns before it touches a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1
TM_SIM_BACKUP, TM_SIM_FRONT = 1, 2


def _header():
    hdr = open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()
    val = lambda prefix: {n: int(v) for n, v in re.findall(r"#define (%s\w+) (\d+)" % prefix, hdr)}
    return val("TM_KIND_"), val("TM_SIM_KERNEL_")


def _lib():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from tetris_mcts_amd import _lib
    return _lib


def test_every_kind_has_exactly_one_kernel():
    kinds, kernels = _header()
    assert sorted(kinds.values()) == list(range(7)) and sorted(kernels.values()) == list(range(4))
    f = _lib().lib().tm_sim_step_kernel
    want = {"TM_KIND_VALUESIM": "TM_SIM_KERNEL_VALUE", "TM_KIND_VALUESIM_LP": "TM_SIM_KERNEL_VALUE", "TM_KIND_CPPAGENT_LP": "TM_SIM_KERNEL_VALUE",
            "TM_KIND_CPPAGENT": "TM_SIM_KERNEL_VALUE", "TM_KIND_VANILLA": "TM_SIM_KERNEL_ROLLOUT", "TM_KIND_VANILLA_C": "TM_SIM_KERNEL_ROLLOUT",
            "TM_KIND_DIST": "TM_SIM_KERNEL_DIST"}
    assert set(want) == set(kinds)
    for name, k in kinds.items():
        assert f(k, 0) == kernels[want[name]], name
        assert f(k, 0) == f(k, 0) and f(k, 0) in kernels.values()
    # the family's own kernel and no other: the value kinds never run TM_KIND_DIST's, TM_KIND_DIST never theirs
    assert {f(k, 0) for n, k in kinds.items() if n != "TM_KIND_DIST"} == {kernels["TM_SIM_KERNEL_VALUE"], kernels["TM_SIM_KERNEL_ROLLOUT"]}


def test_a_cap_selects_the_capped_kernel_only_where_a_store_can_carry_it():
    kinds, kernels = _header()
    f = _lib().lib().tm_sim_step_kernel
    carriers = {"TM_KIND_VALUESIM", "TM_KIND_CPPAGENT"}
    for cap in (1, 3, 4096, 2 ** 31 - 1):
        for name, k in kinds.items():
            got = f(k, cap)
            assert got == (kernels["TM_SIM_KERNEL_CAPPED"] if name in carriers else -1), (name, cap, got)
        assert f(kinds["TM_KIND_DIST"], cap) != kernels["TM_SIM_KERNEL_CAPPED"]
    for k in kinds.values():
        assert f(k, -1) == -1 and f(k, -(2 ** 31)) == -1
    for bad in (-1, 7, 100):
        assert f(bad, 0) == -1 and f(bad, 3) == -1


def test_tm_sim_step_still_refuses_a_cap_on_a_kind_that_cannot_carry_one():
    """a store complete in everything the refusal looks at before the kind (request list, counters, eval_served, one slot, a launch
    that backs up and starts simulations): only the kind is wrong, and nothing is launched"""
    L = _lib()
    kinds, _ = _header()
    lib = L.lib()
    dummy = (C.c_int32 * 16)()
    for name, k in kinds.items():
        s = L.TmStore()
        s.n_games, s.max_nodes, s.eval_slots, s.kind = 8, 64, 1, k
        s.eval_list = s.eval_cnt = s.eval_served = C.cast(dummy, C.c_void_p)
        s.eval_cap = 3
        if name in ("TM_KIND_VALUESIM", "TM_KIND_CPPAGENT"):
            continue            # (these would launch)
        assert lib.tm_sim_step(C.byref(s), TM_SIM_BACKUP | TM_SIM_FRONT, None) == HIP_ERROR_INVALID_VALUE, name
        s.eval_cap = -1
        assert lib.tm_sim_step(C.byref(s), TM_SIM_BACKUP | TM_SIM_FRONT, None) == HIP_ERROR_INVALID_VALUE, name
    s = L.TmStore()
    s.n_games, s.max_nodes, s.eval_slots, s.kind = 8, 64, 1, 7      # a kind the library does not know
    s.eval_list = s.eval_cnt = C.cast(dummy, C.c_void_p)
    assert lib.tm_sim_step(C.byref(s), TM_SIM_BACKUP | TM_SIM_FRONT, None) == HIP_ERROR_INVALID_VALUE
    assert lib.tm_gc_step(C.byref(s), None) == HIP_ERROR_INVALID_VALUE
