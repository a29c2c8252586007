"""The packed route of the HIP fits, as far as it goes without a GPU: the four entry points in the header and the binding, the
refusals of train_data(state_format=...) and of the agents' fit_states, the packing helper of the GPU tests against
dist.render_observations, and the command line."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import dist_fit_cases as DC  # noqa: E402
import fit_hip_cases as FC  # noqa: E402
import fit_packed_cases as PC  # noqa: E402

ENTRY_POINTS = ("tm_valuenet_fit_grad_packed", "tm_valuenet_fit_validate_packed", "tm_distnet_fit_grad_packed",
                "tm_distnet_fit_validate_packed")


def test_the_four_entry_points_are_declared_and_bound():
    from tetris_mcts_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()
    for name in ENTRY_POINTS:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert decl, name
        args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
        assert "const uint32_t *obs" in args, (name, args)
        twin = re.search(r"\bint %s\(([^;]*)\);" % name[:-len("_packed")], hdr)
        twin_args = [a.strip() for a in twin.group(1).replace("\n", " ").split(",")]
        assert [a for a in args if "obs" not in a] == [a for a in twin_args if "states" not in a], name      # the twin's other arguments
        assert len(_lib.SYMBOLS[name]) == len(args) == len(_lib.SYMBOLS[name[:-len("_packed")]])
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[name[:-len("_packed")]]
    assert "any 48 bytes are safe to read" in hdr.lower()


def test_the_library_exports_them():
    from tetris_mcts_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert getattr(L, name).argtypes == _lib.SYMBOLS[name]


def test_the_case_modules_boards_hold_exactly_four_piece_cells_and_round_trip():
    boards, _ = FC.boards(500, 7)
    dist_states = DC.dataset(300, 50, 7)[0]
    for x in (boards, dist_states):
        assert ((x == -1).sum(1) == 4).all()
        k = PC.pack(x)
        assert k.dtype == np.int32 and k.shape == (len(x), 12)
        assert (k[:, 11] == 0).all()
        codes = k[:, 10:11].view(np.uint8).reshape(-1, 4).astype(int)
        assert (np.diff(codes, axis=1) > 0).all() and codes.max() < 200
        assert (PC.render(k) == x).all()


def test_pack_round_trip_with_ended_rows_and_pieces_on_every_edge():
    x = np.concatenate([PC.edge_boards(), PC.mixed_value_case()["data"][0]])
    k = PC.pack(x)
    ended = (x == -1).sum(1) == 0
    assert ended.sum() >= 42 and (~ended).sum() >= 200
    assert (k[ended, 10].view(np.uint32) == 0xFFFFFFFF).all() and (k[ended, 11] == 1).all() and (k[~ended, 11] == 0).all()
    cells = {int(c) for c in np.nonzero(x[:8] == -1)[1]}
    assert {0, 9, 190, 199} <= cells                                    # the four corners are piece cells somewhere
    assert (PC.render(k) == x).all()
    with pytest.raises(AssertionError):
        PC.pack(np.where(np.arange(200) < 3, -1, 0).astype(np.int8).reshape(1, 200))      # three piece cells


def _value_fit():
    from tetris_mcts_amd import train as T
    from tetris_mcts_amd.model import Net
    torch.manual_seed(0)
    net = Net()
    return net, T.Yogi(net.parameters(), lr=1e-3)


def _dist_fit():
    from tetris_mcts_amd import train as T
    from tetris_mcts_amd.model_distributional import Net
    torch.manual_seed(0)
    net = Net(atoms=50)
    return net, T.FusedAdam(net.parameters(), lr=1e-3)


def _targets(head, n):
    rng = np.random.default_rng(0)
    col = lambda: torch.from_numpy(rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32))      # noqa: E731
    if head == "value":
        return [col(), col(), col()]
    return [torch.from_numpy(DC.targets(n, 50, 0)), col()]


KEYS = torch.from_numpy(PC.pack(FC.boards(40, 1)[0]))
REFUSALS = [
    ("the torch fit", dict(fit_backend="torch"), KEYS, "fit_backend"),
    ("torch validation with rows held out", dict(validation_backend="torch", validation_fraction=0.1), KEYS, "validation_backend"),
    ("float observations", dict(validation_backend="hip"), KEYS.float(), "int32"),
    ("rendered rows", dict(validation_backend="hip"), torch.zeros(40, 200, dtype=torch.int32), "12 words"),
    ("observations on the CPU", dict(validation_backend="hip"), KEYS, "on the GPU"),
    ("observations on the CPU, nothing held out", dict(validation_fraction=0.0), KEYS, "on the GPU"),
]


@pytest.mark.parametrize("head", ["value", "dist"])
@pytest.mark.parametrize("what,kw,states,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_train_data_refuses_before_anything_is_touched(head, what, kw, states, word):
    """every refusal is a ValueError that names the option, raised while the optimiser is still unflattened and the net's
    parameters are the objects (and the storage) they were"""
    from tetris_mcts_amd import train as T
    net, opt = _value_fit() if head == "value" else _dist_fit()
    params = [(p, p.data_ptr()) for p in net.parameters()]
    state = torch.get_rng_state()
    kw = dict(dict(fit_backend="hip" if head == "value" else "hip_dist"), **kw)
    with pytest.raises(ValueError, match="state_format") as e:
        T.train_data(net, opt, [states] + _targets(head, 40), state_format="packed", batch_size=8, max_iters=4, log=False, **kw)
    assert word in str(e.value), str(e.value)
    assert opt._flat is None
    assert all(p is q and p.data_ptr() == ptr for p, (q, ptr) in zip(net.parameters(), params))
    assert torch.equal(torch.get_rng_state(), state)                   # no sampling stream was touched


@pytest.mark.parametrize("head", ["value", "dist"])
def test_an_unknown_state_format_is_refused(head):
    from tetris_mcts_amd import train as T
    net, opt = _value_fit() if head == "value" else _dist_fit()
    with pytest.raises(ValueError, match="state_format"):
        T.train_data(net, opt, [KEYS] + _targets(head, 40), state_format="int8", log=False)
    assert opt._flat is None
    with pytest.raises(ValueError, match="state_format"):
        (T.HipFit if head == "value" else T.HipDistFit)(net, opt, [KEYS] + _targets(head, 40), 8, state_format="int8")
    assert opt._flat is None


def test_the_models_refuse_before_the_output_bounds_move():
    """Model_VV.train_data writes out_ubound from the targets before it calls train.train_data: a refused packed fit leaves it"""
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.model_distributional import Model_Dist
    mdl = Model_VV(backend="torch", seed=0, device="cpu")
    before = mdl.model.out_ubound.clone()
    with pytest.raises(ValueError, match="state_format"):
        mdl.train_data([KEYS] + _targets("value", 40), state_format="packed", fit_backend="hip", validation_backend="hip", log=False)
    assert torch.equal(mdl.model.out_ubound, before)
    md = Model_Dist(atoms=50, seed=0, backend="torch", device="cpu")
    with pytest.raises(ValueError, match="state_format"):
        md.train_data([KEYS] + _targets("dist", 40), state_format="packed", fit_backend="hip_dist", validation_backend="hip", log=False)


def test_the_agents_refuse_packed_states_without_the_hip_fit_and_validation():
    """the constructors check fit_states where they check validation_backend: before a store or a model exists"""
    from tetris_mcts_amd import agents
    for cls, hip in ((agents.ValueSim, "hip"), (agents.ValueSimLP, "hip"), (agents.ValueSimC, "hip"), (agents.DistValueSim, "hip_dist")):
        with pytest.raises(ValueError, match="fit_states"):
            cls(fit_states="packed", fit_backend="torch")
        with pytest.raises(ValueError, match="fit_states"):
            cls(fit_states="packed", fit_backend=hip, validation_backend="torch")
        with pytest.raises(ValueError, match="fit_states"):
            cls(fit_states="sparse", fit_backend=hip, validation_backend="hip")


def test_play_lists_the_option():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "play.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "--fit_states" in out.stdout
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "play.py"), "--agent_type", "ValueSim", "--fit_states", "packed"],
                         capture_output=True, text=True, cwd=ROOT)
    assert bad.returncode != 0 and "--fit_states packed" in bad.stderr
