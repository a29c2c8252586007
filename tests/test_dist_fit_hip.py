"""The HIP gradient step of the distributional head's fit (csrc/distnet_fit.hip, tm_adam_step, train.FusedAdam,
train_data(fit_backend="hip_dist")) - what can be checked without a GPU: the ABI's host arithmetic, the fused Adam against
torch.optim.Adam on CPU tensors, the refusals, that the default path is untouched, the layout assumption, the command lines, the
kernels' register budget, and that the GPU tests' yardstick has a non-zero denominator and an honest kink filter."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from tetris_mcts_amd import _lib
    return _lib


def test_workspace_size_is_host_arithmetic():
    lib = _lib().lib()
    for b in (0, -5):
        assert lib.tm_distnet_fit_workspace(b, 50) == -1
    for a in (0, -1, 65, 1000):
        assert lib.tm_distnet_fit_workspace(32, a) == -1
    sizes = [lib.tm_distnet_fit_workspace(b, 50) for b in (1, 2, 3, 4, 5, 31, 32, 33, 255, 256, 257, 1000, 1024, 4096)]
    assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert sizes[12] * 4 < 256 * 2 ** 20            # a batch of 1 024: well inside a quarter of a gigabyte
    assert lib.tm_distnet_fit_workspace(32, 1) > 0 and lib.tm_distnet_fit_workspace(32, 64) > 0


def test_header_declares_the_symbols_and_the_binding_knows_them():
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()
    for name in ("tm_distnet_fit_workspace", "tm_distnet_fit_grad", "tm_adam_step"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in L.SYMBOLS and hasattr(L.lib(), name)
    assert len(L.SYMBOLS["tm_distnet_fit_grad"]) == 13 and len(L.SYMBOLS["tm_adam_step"]) == 14


def test_refused_arguments_without_a_gpu():
    """NULL pointers, batch < 1 and atoms outside 1..64 are refused before anything touches the device"""
    lib = _lib().lib()
    assert lib.tm_distnet_fit_grad(None, None, None, 50, None, None, 8, 50, 1, None, None, None, None) == 1      # hipErrorInvalidValue
    buf = np.zeros(64, np.float32).ctypes.data
    for b, a in ((0, 50), (-3, 50), (8, 0), (8, 65)):
        assert lib.tm_distnet_fit_grad(buf, buf, buf, 64, buf, None, b, a, 1, buf, buf, buf, None) == 1, (b, a)
    assert lib.tm_adam_step(None, None, None, None, None, None, 8, 1e-4, 0.9, 0.999, 1e-5, 0.0, 1, None) == 1


# ---------------------------------------------------------------------------------------------------------------- FusedAdam
def _pair(seed=0, **kw):
    from tetris_mcts_amd import train as T
    torch.manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    return ps, qs, torch.optim.Adam(ps, **kw), T.FusedAdam(qs, **kw)


def _steps(ps, qs, a, b, n, seed):
    g = torch.Generator().manual_seed(seed)
    for _ in range(n):
        for p, q in zip(ps, qs):
            gr = torch.randn(p.shape, generator=g)
            p.grad, q.grad = gr.clone(), gr.clone()
        a.step()
        b.step()


@pytest.mark.parametrize("kw", [dict(lr=1e-4, eps=1e-5, amsgrad=True), dict(lr=1e-3, eps=1e-8, amsgrad=False, weight_decay=1e-2)])
def test_fused_adam_on_cpu_tensors_is_torch_adam_bit_for_bit(kw):
    ps, qs, a, b = _pair(**kw)
    assert b.fused() is False and b.flat_grad() is None
    _steps(ps, qs, a, b, 6, 1)
    for p, q in zip(ps, qs):
        assert p.detach().numpy().tobytes() == q.detach().numpy().tobytes()
    # the state dict is torch.optim.Adam's, and loads in both directions
    import copy
    sa, sb = copy.deepcopy(a.state_dict()), copy.deepcopy(b.state_dict())      # (load_state_dict keeps the tensors it is given)
    assert set(sb["state"][0]) == set(sa["state"][0]) and float(sb["state"][0]["step"]) == 6.0
    if kw["amsgrad"]:
        assert set(sb["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    ps2, qs2, a2, b2 = _pair(**kw)
    with torch.no_grad():
        for src, dst in zip(ps + qs, ps2 + qs2):
            dst.copy_(src)
    a2.load_state_dict(sb)          # FusedAdam -> torch.optim.Adam
    b2.load_state_dict(sa)          # torch.optim.Adam -> FusedAdam
    _steps(ps, qs, a, b, 3, 2)
    _steps(ps2, qs2, a2, b2, 3, 2)
    for p, q, p2, q2 in zip(ps, qs, ps2, qs2):
        assert p.detach().numpy().tobytes() == q.detach().numpy().tobytes() == p2.detach().numpy().tobytes() == q2.detach().numpy().tobytes()
    assert float(b2.state_dict()["state"][0]["step"]) == 9.0


def test_fused_adam_flattened_on_the_cpu_still_takes_torchs_step():
    """flatten() on CPU tensors (the layout check does it) leaves an optimiser that steps as torch.optim.Adam and keeps the state"""
    kw = dict(lr=1e-4, eps=1e-5, amsgrad=True)
    ps, qs, a, b = _pair(**kw)
    _steps(ps, qs, a, b, 2, 1)
    F = b.flatten()
    assert F["t"] == 2 and F["n"] == 22
    _steps(ps, qs, a, b, 4, 2)
    for p, q in zip(ps, qs):
        assert p.detach().numpy().tobytes() == q.detach().numpy().tobytes()
    assert float(b.state_dict()["state"][0]["step"]) == 6.0


def _cpu_dist_model(atoms=50):
    from tetris_mcts_amd import model_distributional as MD
    mdl = MD.Model_Dist(atoms=atoms, device="cpu", seed=0, backend="torch")
    return mdl


def test_flat_order_is_param_order():
    """FusedAdam.flatten() lays the eight tensors out in model_distributional.PARAM_ORDER - what tm_distnet_fit_grad reads and writes"""
    from tetris_mcts_amd import model_distributional as MD, train as T
    mdl = _cpu_dist_model()
    opt = mdl._fused_optimizer()
    assert isinstance(opt, T.FusedAdam) and mdl._fused_optimizer() is opt and mdl._optimizer() is opt
    assert T.flat_order_is_dist_param_order(mdl.model, opt)
    F = opt.flatten()
    assert F["n"] == 279232 + 129 * 50 == 285682
    named = dict(mdl.model.named_parameters())
    assert list(named) == MD.PARAM_ORDER
    off = 0
    for k in MD.PARAM_ORDER:
        p = named[k]
        assert p.data_ptr() == F["p"].data_ptr() + 4 * off and p.grad.data_ptr() == F["g"].data_ptr() + 4 * off, k
        for buf, key in (("m", "exp_avg"), ("v", "exp_avg_sq"), ("vmax", "max_exp_avg_sq")):
            assert opt.state[p][key].data_ptr() == F[buf].data_ptr() + 4 * off, (k, key)
        off += p.numel()
    assert off == F["n"]
    net = MD.Net()
    rev = T.FusedAdam(list(net.parameters())[::-1], lr=1e-4)
    assert not T.flat_order_is_dist_param_order(net, rev)          # another order is noticed


def test_the_adam_state_is_carried_into_the_fused_optimizer():
    mdl = _cpu_dist_model(atoms=7)
    old = mdl._optimizer()
    assert type(old) is torch.optim.Adam
    x = torch.zeros(4, 1, 22, 10)
    t = torch.full((4, 7), 1.0 / 7)
    for _ in range(2):
        old.zero_grad()
        mdl.loss(x, t)[0].backward()
        old.step()
    ref = {k: v.clone() for k, v in old.state_dict()["state"][4].items()}
    new = mdl._fused_optimizer()
    got = new.state_dict()["state"][4]
    assert float(got["step"]) == 2.0 and new.param_groups[0]["lr"] == 1e-4 and new.param_groups[0]["amsgrad"] is True
    for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        assert torch.equal(got[k], ref[k]), k


# ----------------------------------------------------------------------------------------------------------------- refusals
def _data(n=24, atoms=50, seed=0):
    import dist_fit_cases as DC
    import heads_numerics as HN
    s, t, w = DC.dataset(n, atoms, seed)
    return [HN.dn_input(s), torch.from_numpy(t), torch.from_numpy(w).reshape(-1, 1)]


def test_hip_dist_refuses_what_it_cannot_do():
    from tetris_mcts_amd import model as M, model_distributional as MD, train as T
    mdl = _cpu_dist_model()
    data = _data()
    opt = mdl._fused_optimizer()
    kw = dict(batch_size=8, max_iters=2, iters_per_val=10, log=False, validation_fraction=0.0)

    def fit(d=data, net=mdl.model, o=opt, **more):
        return T.train_data(net, o, d, fit_backend="hip_dist", **dict(kw, **more))
    with pytest.raises(ValueError, match="CUDA"):                       # float32 CUDA data
        fit()
    with pytest.raises(ValueError, match="CUDA"):
        fit([d.double() for d in data])
    with pytest.raises(ValueError, match="loss_fn"):                    # a custom loss
        fit(loss_fn=lambda net, batch, weighted: (None, None))
    with pytest.raises(ValueError, match="oversampling"):
        fit(oversampling=True)
    with pytest.raises(ValueError, match=r"\[states, targets, weights\]"):
        fit(data + [data[2]])
    with pytest.raises(ValueError, match="22 x 10"):                    # the value net's 20 rows
        fit([data[0][:, :, 2:]] + data[1:])
    with pytest.raises(ValueError, match="int8"):
        fit([data[0] * 0.5] + data[1:])
    top = data[0].clone()
    top[3, 0, 1, 4] = 1.0
    with pytest.raises(ValueError, match="top rows"):
        fit([top] + data[1:])
    for bad in (float("nan"), float("inf"), -1e-3):
        t = data[1].clone()
        t[5, 7] = bad
        with pytest.raises(ValueError, match="finite targets"):
            fit([data[0], t, data[2]])
    with pytest.raises(ValueError, match="atoms"):                      # 49 columns for a net of 50 atoms
        fit([data[0], data[1][:, :49].contiguous(), data[2]])
    with pytest.raises(ValueError, match="one weight a row"):
        fit([data[0], data[1], data[2][:-1]])
    with pytest.raises(ValueError, match="model_distributional.Net"):   # the value net
        vn = M.Net()
        fit(net=vn, o=T.FusedAdam(vn.parameters(), lr=1e-4))
    with pytest.raises(ValueError, match="FusedAdam"):                  # torch's Adam, and Yogi
        fit(o=torch.optim.Adam(mdl.model.parameters(), lr=1e-4))
    with pytest.raises(ValueError, match="FusedAdam"):
        fit(o=T.Yogi(mdl.model.parameters(), lr=1e-4))
    net2 = MD.Net()
    with pytest.raises(ValueError, match="PARAM_ORDER"):
        fit(net=net2, o=T.FusedAdam(list(net2.parameters())[::-1], lr=1e-4))
    with pytest.raises(ValueError, match="fit_backend"):
        T.train_data(mdl.model, opt, data, fit_backend="triton", **kw)
    # "hip" stays the value net's: its own checks refuse the head's data and net
    with pytest.raises(ValueError):
        T.train_data(mdl.model, opt, data, fit_backend="hip", **kw)
    with pytest.raises(ValueError, match="fit_backend"):
        mdl.train_data(data, fit_backend="hip", **kw)
    with pytest.raises(ValueError, match="CUDA"):
        mdl.train_data(data, fit_backend="hip_dist", **kw)


def test_a_refused_hip_dist_fit_leaves_the_model_as_it_was():
    """no optimiser swap and no flattening before the checks have passed"""
    from tetris_mcts_amd import train as T
    mdl = _cpu_dist_model()
    old = mdl._optimizer()
    ptrs = [p.data_ptr() for p in mdl.model.parameters()]
    kw = dict(batch_size=8, max_iters=2, iters_per_val=10, log=False)
    with pytest.raises(ValueError, match="CUDA"):
        mdl.train_data(_data(), fit_backend="hip_dist", **kw)
    assert mdl.optimizer is old and type(old) is torch.optim.Adam
    assert [p.data_ptr() for p in mdl.model.parameters()] == ptrs and all(p.grad is None for p in mdl.model.parameters())
    opt = T.FusedAdam(mdl.model.parameters(), lr=1e-4)
    with pytest.raises(ValueError, match="CUDA"):
        T.train_data(mdl.model, opt, _data(), fit_backend="hip_dist", **kw)
    assert opt._flat is None and [p.data_ptr() for p in mdl.model.parameters()] == ptrs


def test_fused_adam_clears_gradients_as_torch_does_outside_the_fused_form():
    ps, qs, a, b = _pair(lr=1e-4)
    _steps(ps, qs, a, b, 1, 1)
    b.flatten()
    b.zero_grad()
    assert all(q.grad is None for q in qs)


def test_the_keyword_on_the_agents_and_on_the_value_net():
    import inspect
    from tetris_mcts_amd import agents, model as M
    from tetris_mcts_amd.agents.DistValueSim import DistValueSim
    assert inspect.signature(DistValueSim.__init__).parameters["fit_backend"].default == "torch"
    with pytest.raises(ValueError, match="fit_backend"):
        DistValueSim(fit_backend="hip")                                 # still the value net's name
    with pytest.raises(ValueError, match="fit_backend"):
        DistValueSim(fit_backend="cuda")
    for cls in (agents.ValueSim, agents.ValueSimLP, agents.ValueSimC):
        with pytest.raises(ValueError, match="fit_backend"):
            cls(fit_backend="hip_dist")
    mdl = M.Model_VV.__new__(M.Model_VV)
    mdl.device = torch.device("cpu")
    with pytest.raises(ValueError, match="hip_dist"):
        mdl.train_data([], fit_backend="hip_dist")


def test_command_lines_list_the_choice():
    import play
    p = play.build_parser()
    assert p.parse_args([]).fit_backend == "torch" and p.parse_args(["--fit_backend", "hip_dist"]).fit_backend == "hip_dist"
    assert "hip_dist" in p.format_help()
    with pytest.raises(SystemExit):
        p.parse_args(["--fit_backend", "hip_head"])
    with pytest.raises(SystemExit, match="DistValueSim only"):
        play.main(["--agent_type", "ValueSim", "--fit_backend", "hip_dist"])
    for script in ("selfplay_online.py", "fit_timing.py"):
        src = open(os.path.join(ROOT, "scripts", script)).read()
        assert re.search(r'add_argument\("--fit_backend"[^\n]*"hip_dist"', src), script
    assert "--head" in open(os.path.join(ROOT, "scripts", "fit_timing.py")).read()


def test_the_default_path_is_the_path_without_the_keyword():
    """Model_Dist.train_data with no keyword and with fit_backend="torch": the same optimiser class and the same bytes after the
    same seeded fit"""
    torch.set_num_threads(1)
    data = _data(48)
    flats = []
    for kw in ({}, {"fit_backend": "torch"}):
        mdl = _cpu_dist_model()
        gen = torch.Generator().manual_seed(3)
        res = mdl.train_data(data, batch_size=16, max_iters=6, iters_per_val=3, generator=gen, log=False, **kw)
        assert res["iters"] == 6 and res["graph_replay"] is False and type(mdl.optimizer) is torch.optim.Adam
        flats.append(mdl.flat_params().numpy().copy())
    assert flats[0].tobytes() == flats[1].tobytes()
    start = _cpu_dist_model().flat_params().numpy()
    assert np.abs(flats[0] - start).max() > 1e-4


# ----------------------------------------------------------------------------------------------------------- the yardstick
def test_the_kink_filter_keeps_its_cap():
    """the filter drops at most a quarter of the candidate rows, for every net of the cases and for every candidate set of the
    large-batch cases"""
    import dist_fit_cases as DC
    DC.cases(full=False)
    DC.large_cases()
    assert set(DC.KINK_KEPT) == set(DC.nets()) | set(DC.LARGE_SETS) and len(DC.KINK_KEPT) == len(DC.nets()) + len(DC.LARGE_NETS)
    for name, kept in DC.KINK_KEPT.items():
        print("off the kink: %-20s keeps %.1f %% of %d rows" % (name, 100 * kept, DC.candidates(name)))
        assert kept >= 1.0 - DC.KINK_CAP, (name, kept)
    assert {DC.candidates(n) for n in DC.LARGE_SETS} == {1400} and {DC.candidates(n) for n in DC.nets()} == {420}


def test_the_yardstick_has_a_denominator_in_every_regime():
    """torch's own fp32 gradients differ from its fp64 gradients in every tensor of every small case; at atoms = 1 the gradient is
    identically zero in both precisions (log p = 0)"""
    import dist_fit_cases as DC
    torch.set_num_threads(4)
    seen = 0
    for name, case in DC.cases(full=False).items():
        if case["batch"] > 128:
            continue
        g64, l64 = DC.reference(name, case, torch.float64)
        g32, l32 = DC.reference(name, case, torch.float32)
        seen += 1
        for t, a, b in zip(DC.TENSORS, g32, g64):
            assert np.isfinite(b).all() and np.isfinite(a).all(), (name, t)
            if case["atoms"] == 1:
                assert np.abs(a).max() == 0 and np.abs(b).max() == 0, (name, t)
            else:
                assert np.abs(b).max() > 0 and np.abs(a - b).max() > 0, (name, t)
        assert np.isfinite(l64[0]) and np.isfinite(l32[0])
        assert np.isfinite(l64[1]) == (case["batch"] > 1)          # torch.std_mean's n - 1: NaN for one sample
    assert seen >= 15


def _distinct(states, targets):
    """the number of distinct rows (a state with its target; empty boards under the same piece recur among the states alone)"""
    return len(np.unique(np.concatenate([np.asarray(states, np.float32), np.asarray(targets, np.float32).reshape(len(states), -1)], 1), axis=0))


def test_the_yardstick_has_a_denominator_in_the_large_batch_regimes():
    """the cases past dist_fit_cases.BATCHES (batch 480 - 1 025, on candidate sets of 1 400 rows): finite references, torch's fp32
    gradients differ from its fp64 gradients in every tensor, and every set has more distinct rows than the largest batch"""
    import dist_fit_cases as DC
    torch.set_num_threads(4)
    large = DC.large_cases()
    assert list(large) == DC.case_names()[-len(large):] == list(DC.large_cases(names_only=True)) and len(large) == 9
    assert sorted(c["batch"] for c in large.values()) == [480, 512, 513, 513, 513, 1000, 1024, 1024, 1025]
    null = large["fitted, batch 1024, unweighted, idx NULL"]
    assert null["idx"] is None and _distinct(null["data"][0][:1024], null["data"][1][:1024]) == 1024
    for name, case in large.items():
        assert _distinct(*case["data"][:2]) > max(DC.LARGE_BATCHES), name
        g64, l64 = DC.reference(name, case, torch.float64)
        g32, l32 = DC.reference(name, case, torch.float32)
        for t, a, b in zip(DC.TENSORS, g32, g64):
            assert np.isfinite(b).all() and np.isfinite(a).all() and np.abs(b).max() > 0 and np.abs(a - b).max() > 0, (name, t)
        assert all(np.isfinite(l64)) and all(np.isfinite(l32))
        assert l32[0] != l64[0] and l32[1] != l64[1], (name, "the loss outputs' denominators")


# ------------------------------------------------------------------------------------------------- code object and source
def test_fit_kernels_use_no_scratch_memory(tmp_path):
    """every kernel of csrc/distnet_fit.hip (csrc/fit_mma.h's shared ones included): no private segment, no spilled registers (read from the built code object)"""
    import shutil
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    obj = os.path.join(ROOT, "tetris_mcts_amd", "csrc", "_obj", "distnet_fit.o")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no llvm binutils")
    if not os.path.exists(obj):
        pytest.skip("HIP objects not built")
    local = str(tmp_path / "distnet_fit.o")
    shutil.copy(obj, local)
    subprocess.check_call([objdump, "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    cos = [f for f in os.listdir(tmp_path) if f.startswith("distnet_fit.o.") and "amdgcn" in f]
    assert cos, "no device code object in " + obj
    notes = subprocess.check_output([readelf, "--notes", str(tmp_path / cos[0])]).decode()
    found = re.findall(r"\.name:\s+(\S+)\s.*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", notes, re.S)
    names = [n for n, _, _, _ in found]
    for want in ("k_df_conv_fwd", "k_fit_fc1_fwd", "k_df_head", "k_df_head_part", "k_df_fc_dw", "k_fit_fc1_bwd_data", "k_df_conv_bwd_data",
                 "k_df_conv_dw", "k_df_conv_bias_part", "k_fit_reduce", "k_fit_loss", "k_fit_val_moments"):
        assert any(want in n for n in names), want
    assert len(found) >= 15
    for name, scratch, sspill, vspill in found:
        assert "k_df_" in name or "k_fit_" in name, name
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, (name, scratch, sspill, vspill)


def test_the_source_has_no_atomics():
    for f in ("distnet_fit.hip", "fit_mma.h"):
        src = open(os.path.join(ROOT, "tetris_mcts_amd", "csrc", f)).read().lower()
        code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
        assert "atomic" not in code and "hipmalloc" not in code and "synchronize" not in code and "memcpy" not in code, f
