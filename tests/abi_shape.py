"""The shape of the leaf evaluators' C ABI, for the three test_library_exports_*_abi tests: `backend` (and for the value net
`fc1`) are arguments of one entry point each, not a suffix of its name."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry point -> number of arguments
VALUENET = {"tm_valuenet_check_mode": 2, "tm_valuenet_prepare": 5, "tm_valuenet_forward": 10, "tm_valuenet_forward_requests": 7, "tm_search_set_valuenet": 3}
DISTNET = {"tm_distnet_prepare": 4, "tm_distnet_forward": 10, "tm_distnet_forward_requests": 6}
# the entry points that carried a backend in their names
REMOVED = ("tm_valuenet_prepare_x3", "tm_valuenet_prepare_fc1_x3", "tm_valuenet_forward_x3", "tm_valuenet_forward_x3f",
           "tm_valuenet_forward_requests_x3", "tm_valuenet_forward_requests_x3f", "tm_distnet_prepare_x3", "tm_distnet_forward_x3",
           "tm_distnet_forward_requests_x3", "tm_search_set_valuenet_fc1")


def header():
    return open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()


def check(entry_points):
    """every entry point is declared with its argument count, in SYMBOLS with as many, and exported; none of the removed names
    is left in the header (its comments included), in SYMBOLS or among the library's exported symbols"""
    from tetris_mcts_amd import _lib
    hdr, lib = header(), _lib.lib()
    for name, n_args in entry_points.items():
        decl = re.findall(r"^int %s\(([^;]*)\);" % name, hdr, re.M)
        assert len(decl) == 1, name
        assert len(decl[0].split(",")) == n_args, (name, decl[0])
        assert len(_lib.SYMBOLS[name]) == n_args, name
        assert hasattr(lib, name), name
    assert len(REMOVED) == 10
    for name in REMOVED:
        assert not re.search(r"\b%s\b" % name, hdr), name
        assert name not in _lib.SYMBOLS, name
        assert not hasattr(lib, name), name


def check_defines(values):
    hdr = header()
    for name, value in values:
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == value, name


def check_setter(lib, handle, dist):
    """tm_search_set_valuenet over every (backend, fc1) in {-1, 0, 1, 2}^2, both values in one call: 0 for the three valid pairs,
    refused for every other one; a distributional store has no fc1 option.  Whatever was set or refused before, a pair gets the
    same answer (the grid is walked forwards and backwards)."""
    grid = [(b, f) for b in (-1, 0, 1, 2) for f in (-1, 0, 1, 2)]
    for backend, fc1 in grid + grid[::-1]:
        ok = (backend, fc1) in ((0, 0), (1, 0), (1, 1)) and not (dist and fc1 != 0)
        assert lib.tm_search_set_valuenet(handle, backend, fc1) == (0 if ok else 1), (dist, backend, fc1)      # hipErrorInvalidValue
