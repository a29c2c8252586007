"""The HIP validation pass of the fits (tm_valuenet_fit_validate, tm_distnet_fit_validate, train_data(validation_backend="hip"))
- what can be checked without a GPU: the workspace arithmetic, the refusals (each leaving the parameters and a seeded generator
as they were), that the torch path keeps its bits, the pass-through of the option, and that the GPU tests' references are finite
with a non-zero denominator of the yardstick."""
import os
import re

import numpy as np
import pytest
import torch

import fit_validation_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from tetris_mcts_amd import _lib
    return _lib


def test_workspace_sizes_are_host_arithmetic_of_the_slab_alone():
    lib = _lib().lib()
    for bad in (0, -5, (1 << 20) + 1):
        assert lib.tm_valuenet_fit_validate_workspace(bad) == -1 and lib.tm_distnet_fit_validate_workspace(bad, 50) == -1
    for atoms in (0, -1, 65):
        assert lib.tm_distnet_fit_validate_workspace(64, atoms) == -1
    slabs = (1, 2, 31, 32, 33, 64, 1024, 4096, 1 << 20)
    for sizes, per_row in (([lib.tm_valuenet_fit_validate_workspace(s) for s in slabs], 9728),
                           ([lib.tm_distnet_fit_validate_workspace(s, 50) for s in slabs], 6528)):
        assert all(a < b for a, b in zip(sizes, sizes[1:]))                     # grows with the slab
        for s, n in zip(slabs, sizes):
            assert n % 4 == 0 and per_row * s + 2 * s <= n <= per_row * s + 2 * s + 3      # the activations and a double a row
    assert lib.tm_distnet_fit_validate_workspace(64, 1) == lib.tm_distnet_fit_validate_workspace(64, 64)
    # n is no argument of the workspace functions: a pass over any number of rows needs the slab's floats
    L = _lib()
    assert len(L.SYMBOLS["tm_valuenet_fit_validate_workspace"]) == 1 and len(L.SYMBOLS["tm_distnet_fit_validate_workspace"]) == 2
    assert lib.tm_valuenet_fit_validate_workspace(4096) * 4 < 256 * 2 ** 20      # the default slab: inside a quarter of a gigabyte


def test_header_declares_the_validation_pass_and_the_binding_knows_it():
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()
    for name in ("tm_valuenet_fit_validate_workspace", "tm_valuenet_fit_validate", "tm_distnet_fit_validate_workspace",
                 "tm_distnet_fit_validate"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in L.SYMBOLS and hasattr(L.lib(), name)
    assert len(L.SYMBOLS["tm_valuenet_fit_validate"]) == 14 and len(L.SYMBOLS["tm_distnet_fit_validate"]) == 13


def test_refused_arguments_without_a_gpu():
    """NULL pointers, n < 1, a refused chunk / slab / atoms / stride and a misaligned workspace: refused before the device is
    touched, rows_out as it was"""
    lib = _lib().lib()
    mem = np.zeros(256, np.float64)
    rows = np.full(12, 7.0)
    buf, out = mem.ctypes.data, rows.ctypes.data
    ok_v = [buf, buf, buf, buf, buf, buf, 33, 32, 64, 1, 0.1, out, buf, None]
    ok_d = [buf, buf, buf, 50, buf, 33, 32, 64, 50, 1, out, buf, None]

    def with_(args, k, v):
        a = list(args)
        a[k] = v
        return a
    for k in (0, 1, 2, 3, 4, 5, 11, 12):
        assert lib.tm_valuenet_fit_validate(*with_(ok_v, k, None)) == 1, k          # hipErrorInvalidValue
    for k in (0, 1, 2, 4, 10, 11):
        assert lib.tm_distnet_fit_validate(*with_(ok_d, k, None)) == 1, k
    for n, chunk, slab in ((0, 32, 64), (-1, 32, 64), (33, 0, 64), (33, -32, 64), (33, 32, 16), (33, 32, 48), (33, 32, 0),
                           (33, 3, 64), (33, 32, (1 << 20) + 32)):
        assert lib.tm_valuenet_fit_validate(*with_(with_(with_(ok_v, 6, n), 7, chunk), 8, slab)) == 1, (n, chunk, slab)
        assert lib.tm_distnet_fit_validate(*with_(with_(with_(ok_d, 5, n), 6, chunk), 7, slab)) == 1, (n, chunk, slab)
    for atoms, stride in ((0, 50), (65, 70), (-2, 50), (50, 49), (7, 6)):
        assert lib.tm_distnet_fit_validate(*with_(with_(ok_d, 8, atoms), 3, stride)) == 1, (atoms, stride)
    assert lib.tm_valuenet_fit_validate(*with_(ok_v, 12, buf + 4)) == 1             # a workspace off its 16 bytes
    assert lib.tm_distnet_fit_validate(*with_(ok_d, 11, buf + 8)) == 1
    assert (rows == 7.0).all()


def test_combine_chunk_rows_is_the_loop_validation_loss_ran():
    """the factored host combination: validation_loss's numbers through it are the numbers of the loop written out here, and a
    NaN std counts as 0"""
    import math
    from tetris_mcts_amd import train as T
    rows = [[3.5, 1.25, 0.5], [1.0, 2.0, float("nan")], [7.0, 0.75, 0.125]]
    tot_w, acc, acc2 = 0.0, 0.0, 0.0
    for w, mean, std in rows:
        std = 0.0 if math.isnan(std) else std
        tot_w += w
        acc += w * mean
        acc2 += w * (std * std + mean * mean)
    mean = acc / tot_w
    assert T.combine_chunk_rows(rows) == (mean, math.sqrt(max(acc2 / tot_w - mean * mean, 0.0)))
    case = VC.value_regime("fresh net, weighted")
    net, data, loss_fn = VC.torch_batches(case, 97, torch.float32)
    got = T.validation_loss(net, data, True, chunk=32)
    rows32, comb = VC.reference("value", "fresh net, weighted", 97, torch.float32)
    assert got == comb and len(rows32) == 4


def _state(net, gen):
    return [p.detach().clone() for p in net.parameters()], gen.get_state().clone(), torch.random.get_rng_state().clone()


def _unchanged(net, gen, before):
    ps, g, glob = before
    return (all(torch.equal(a, b) and a.grad is None for a, b in zip(net.parameters(), ps)) and torch.equal(gen.get_state(), g)
            and torch.equal(torch.random.get_rng_state(), glob))


def test_value_net_refusals_leave_the_parameters_and_the_generator_alone():
    from tetris_mcts_amd import model as M, train as T
    s, v, var, w = VC.value_regime("fresh net, weighted")["data"]
    data = [torch.from_numpy(s.reshape(-1, 1, 20, 10).astype(np.float32))] + [torch.from_numpy(a.reshape(-1, 1).copy()) for a in (v, var, w)]
    net = M.Net()
    opt = T.Yogi(net.parameters(), lr=1e-3, eps=1e-3, weight_decay=1e-3)
    gen = torch.Generator().manual_seed(11)
    kw = dict(batch_size=16, max_iters=2, iters_per_val=1, log=False, generator=gen)
    before = _state(net, gen)
    refused = [dict(validation_backend="hip"),                                            # fit_backend="torch"
               dict(validation_backend="hip", fit_backend="torch"),
               dict(validation_backend="hip", fit_backend="hip"),                         # CPU tensors
               dict(validation_backend="hip", fit_backend="hip", loss_fn=T.batch_loss),   # a custom loss_fn
               dict(validation_backend="hip", loss_fn=T.batch_loss),
               dict(validation_backend="HIP", fit_backend="hip"),                         # unknown spellings
               dict(validation_backend="triton"),
               dict(validation_backend=None),
               dict(validation_backend="hip", fit_backend="torch", validation_fraction=0.0)]
    for more in refused:
        with pytest.raises(ValueError):
            T.train_data(net, opt, data, **dict(kw, **more))
        assert _unchanged(net, gen, before), more
        assert getattr(opt, "_flat", None) is None, more
    with pytest.raises(ValueError, match="validation_backend"):
        T.train_data(net, opt, data, validation_backend="hip", **kw)
    with pytest.raises(ValueError, match="validation_backend"):
        T.train_data(net, opt, data, validation_backend="rocm", fit_backend="hip", **kw)
    # Model_VV refuses before it writes the output bounds
    mdl = M.Model_VV.__new__(M.Model_VV)
    mdl.device, mdl.backend, mdl.optimizer, mdl.model = torch.device("cpu"), "torch", None, net
    mdl._flat = mdl._prepared = mdl._scratch = None
    with pytest.raises(ValueError, match="validation_backend"):
        mdl.train_data(data, validation_backend="hip", **kw)
    assert _unchanged(net, gen, before)


def test_head_refusals_leave_the_parameters_and_the_generator_alone():
    from tetris_mcts_amd import model_distributional as MD, train as T
    import heads_numerics as HN
    s, t, w = VC.dist_regime("fixture")["data"]
    data = [HN.dn_input(s), torch.from_numpy(t), torch.from_numpy(w).reshape(-1, 1)]
    mdl = MD.Model_Dist(atoms=50, device="cpu", seed=0, backend="torch")
    old = mdl._optimizer()
    gen = torch.Generator().manual_seed(11)
    kw = dict(batch_size=16, max_iters=2, iters_per_val=1, log=False, generator=gen)
    before = _state(mdl.model, gen)
    for more in (dict(validation_backend="hip"), dict(validation_backend="hip", fit_backend="torch"),
                 dict(validation_backend="hip", fit_backend="hip_dist"), dict(validation_backend="torch ", fit_backend="hip_dist"),
                 dict(validation_backend="hip", fit_backend="hip")):
        with pytest.raises(ValueError):
            mdl.train_data(data, **dict(kw, **more))
        assert _unchanged(mdl.model, gen, before) and mdl.optimizer is old, more
    opt = T.FusedAdam(mdl.model.parameters(), lr=1e-4)
    for more in (dict(validation_backend="hip", fit_backend="hip_dist"),                                  # CPU tensors
                 dict(validation_backend="hip", fit_backend="hip_dist", loss_fn=lambda n, b, wt: (None, None)),
                 dict(validation_backend="hip", loss_fn=T.dist_batch_loss)):
        with pytest.raises(ValueError):
            T.train_data(mdl.model, opt, data, **dict(kw, **more))
        assert _unchanged(mdl.model, gen, before) and opt._flat is None, more


def test_the_torch_backend_is_the_path_without_the_keyword():
    """validation_backend="torch" and no keyword: the same bits and the same validation loss after the same fit"""
    from tetris_mcts_amd import model as M, train as T
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_training.npz"))
    batch = [torch.from_numpy(g[k].copy()) for k in ("tr_states", "tr_values", "tr_variances", "tr_weights")]
    torch.set_num_threads(1)
    out = []
    for kw in ({}, {"validation_backend": "torch"}):
        torch.manual_seed(0)
        net = M.Net()
        opt = T.Yogi(net.parameters(), lr=1e-3, eps=1e-3, weight_decay=1e-3)
        gen = torch.Generator().manual_seed(3)
        res = T.train_data(net, opt, batch, batch_size=16, max_iters=6, iters_per_val=3, generator=gen, log=False, **kw)
        out.append((torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy().tobytes(), res["best_validation"]))
    assert out[0] == out[1] and np.isfinite(out[0][1])


def test_the_agents_and_the_command_lines_pass_the_option_on():
    import inspect
    import play
    from tetris_mcts_amd.agents import DistValueSim, ValueSim
    p = play.build_parser()
    assert p.parse_args([]).validation_backend == "torch"
    assert p.parse_args(["--validation_backend", "hip"]).validation_backend == "hip"
    with pytest.raises(SystemExit):
        p.parse_args(["--validation_backend", "triton"])
    with pytest.raises(SystemExit) as e:          # refused with a message where --fit_backend is torch, before any engine is built
        play.main(["--agent_type", "ValueSim", "--validation_backend", "hip"])
    assert "--fit_backend" in str(e.value)
    for cls, fit in ((ValueSim, "hip"), (DistValueSim, "hip_dist")):
        assert inspect.signature(cls.__init__).parameters["validation_backend"].default == "torch"
        with pytest.raises(ValueError, match="validation_backend"):
            cls(validation_backend="hip")                          # fit_backend="torch"
        with pytest.raises(ValueError, match="validation_backend"):
            cls(validation_backend="triton", fit_backend=fit)
    for path in ("scripts/selfplay_online.py", "scripts/fit_timing.py"):
        assert "--validation_backend" in open(os.path.join(ROOT, path)).read(), path


@pytest.mark.parametrize("head,name", VC.ALL)
def test_references_are_finite_and_the_yardstick_has_a_denominator(head, name):
    torch.set_num_threads(8)
    for n in VC.ROWS + (1,):
        r64, c64 = VC.reference(head, name, n, torch.float64)
        r32, c32 = VC.reference(head, name, n, torch.float32)
        single = VC.one_row_chunks(n)
        assert r64.shape == r32.shape == ((n + VC.CHUNK - 1) // VC.CHUNK, 3) and single.sum() == 1
        assert np.isfinite(r64[:, :2]).all() and np.isfinite(r32[:, :2]).all() and np.isfinite(c64).all() and np.isfinite(c32).all()
        assert np.isfinite(r64[~single, 2]).all() and np.isfinite(r32[~single, 2]).all()
        # the exact part: a one-row chunk's std is 0 (population) or NaN (n - 1), in both precisions
        for r in (r64, r32):
            assert (np.isnan(r[single, 2]).all() if head == "dist" else (r[single, 2] == 0).all())
        case = VC.regime(head, name)
        if case["weighted"]:
            assert abs(r64[:, 0].sum() - np.asarray(case["data"][-1][:n], np.float64).sum()) < 1e-9
        else:
            assert (r64[:, 0] == [min(VC.CHUNK, n - c) for c in range(0, n, VC.CHUNK)]).all()
        if name.split(",")[0] in VC.EXACT_ZERO:
            assert (r64[:, 1] == 0).all() and (r32[:, 1] == 0).all() and c64 == (0.0, 0.0) and c32 == (0.0, 0.0)
            continue
        parts = [("chunk means", r32[:, 1], r64[:, 1]), ("combined mean", [c32[0]], [c64[0]])]
        if n > 1:
            parts += [("chunk stds", r32[~single, 2], r64[~single, 2]), ("combined std", [c32[1]], [c64[1]])]
        for what, a32, a64 in parts:
            a32, a64 = np.asarray(a32), np.asarray(a64)
            assert np.abs(a64).max() > 0, (what, n)
            own = np.abs(a32 - a64).max()
            print("%-6s %-34s n %3d  %-13s torch fp32 error %.3e at values up to %.3e" % (head, name, n, what, own, np.abs(a64).max()))
            assert own > 0, (head, name, n, what, "the rule's denominator")
