"""The HIP gradient step of the fit (csrc/valuenet_fit.hip, train_data(fit_backend="hip")) - what can be checked without a GPU:
the ABI's host arithmetic, the refusals, that the default path is untouched, the layout assumption, the command line, the
kernels' register budget, and that the GPU tests' yardstick has a non-zero denominator in every regime."""
import os
import re
import subprocess
import sys

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
    assert lib.tm_valuenet_fit_workspace(0) == -1 and lib.tm_valuenet_fit_workspace(-5) == -1
    sizes = [lib.tm_valuenet_fit_workspace(b) for b in (1, 2, 31, 32, 33, 256, 512, 1000, 1024, 4096)]
    assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert sizes[8] * 4 < 256 * 2 ** 20            # a batch of 1 024: well inside a quarter of a gigabyte


def test_header_declares_the_fit_and_the_binding_knows_it():
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()
    for name in ("tm_valuenet_fit_workspace", "tm_valuenet_fit_grad"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in L.SYMBOLS and hasattr(L.lib(), name)
    assert len(L.SYMBOLS["tm_valuenet_fit_grad"]) == 14


def test_refused_arguments_without_a_gpu():
    """NULL pointers and batch < 1 are refused before anything touches the device"""
    lib = _lib().lib()
    assert lib.tm_valuenet_fit_grad(None, None, None, None, None, None, None, 8, 1, 0.1, None, None, None, None) == 1      # hipErrorInvalidValue
    buf = np.zeros(64, np.float32).ctypes.data
    assert lib.tm_valuenet_fit_grad(buf, buf, buf, buf, buf, buf, None, 0, 1, 0.1, buf, buf, buf, None) == 1
    assert lib.tm_valuenet_fit_grad(buf, buf, buf, buf, buf, buf, None, -3, 1, 0.1, buf, buf, buf, None) == 1


def _cpu_model():
    from tetris_mcts_amd import model as M
    mdl = M.Model_VV.__new__(M.Model_VV)
    mdl.device, mdl.backend = torch.device("cpu"), "torch"
    mdl._flat = mdl._prepared = mdl._scratch = None
    mdl.optimizer = None
    mdl.model = M.Net()
    return mdl


def _gold_batch():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_training.npz"))
    return g, [torch.from_numpy(g[k].copy()) for k in ("tr_states", "tr_values", "tr_variances", "tr_weights")]


def test_hip_fit_refuses_what_it_cannot_do():
    from tetris_mcts_amd import train as T
    g, batch = _gold_batch()
    mdl = _cpu_model()
    opt = mdl._optimizer()
    kw = dict(batch_size=16, max_iters=2, iters_per_val=10, log=False)
    with pytest.raises(ValueError, match="CUDA"):
        T.train_data(mdl.model, opt, batch, fit_backend="hip", **kw)
    with pytest.raises(ValueError, match="loss_fn"):
        T.train_data(mdl.model, opt, batch, fit_backend="hip", loss_fn=T.batch_loss, **kw)
    with pytest.raises(ValueError, match="oversampling"):
        T.train_data(mdl.model, opt, batch, fit_backend="hip", oversampling=True, **kw)
    half = [batch[0] * 0.5] + batch[1:]
    with pytest.raises(ValueError, match="int8"):
        T.train_data(mdl.model, opt, half, fit_backend="hip", **kw)
    with pytest.raises(ValueError, match="fit_backend"):
        T.train_data(mdl.model, opt, batch, fit_backend="triton", **kw)


def test_the_torch_backend_is_the_path_without_the_keyword():
    """fit_backend="torch" and no keyword: the same bits after the same fit (weights of tests/golden/ref_training.npz)"""
    from tetris_mcts_amd import train as T
    g, batch = _gold_batch()
    torch.set_num_threads(1)
    flats = []
    for kw in ({}, {"fit_backend": "torch"}):
        mdl = _cpu_model()
        mdl.set_flat_params(g["tr_params0"])
        gen = torch.Generator().manual_seed(3)
        res = T.train_data(mdl.model, mdl._optimizer(), batch, batch_size=16, max_iters=6, iters_per_val=3, generator=gen, log=False, **kw)
        assert res["iters"] == 6 and res["graph_replay"] is False
        mdl._flat = None
        flats.append(mdl.flat_params().numpy().copy())
    assert flats[0].tobytes() == flats[1].tobytes()
    assert np.abs(flats[0] - g["tr_params0"]).max() > 1e-4


def test_flat_order_is_param_order():
    """Yogi.flatten() lays the learnable tensors out in model.PARAM_ORDER[:10] - what tm_valuenet_fit_grad reads and writes"""
    from tetris_mcts_amd import model as M, train as T
    mdl = _cpu_model()
    opt = mdl._optimizer()
    assert T.flat_order_is_param_order(mdl.model, opt)
    F = opt.flatten()
    assert F["n"] == T.HipFit.N_PARAMS == 478338
    named = dict(mdl.model.named_parameters())
    off = 0
    for k in M.PARAM_ORDER[:10]:
        p = named[k]
        assert p.data_ptr() == F["p"].data_ptr() + 4 * off and p.grad.data_ptr() == F["g"].data_ptr() + 4 * off, k
        off += p.numel()
    assert [k for k in M.PARAM_ORDER[10:]] == ["out_ubound", "out_lbound"] and not named["out_ubound"].requires_grad
    # another order is noticed
    net = M.Net()
    rev = T.Yogi(list(net.parameters())[::-1], lr=1e-3)
    assert not T.flat_order_is_param_order(net, rev)


def test_agents_take_the_keyword():
    import inspect
    from tetris_mcts_amd import agents
    from tetris_mcts_amd.agents.DistValueSim import DistValueSim
    assert "fit_backend" in inspect.signature(agents.ValueSim.__init__).parameters
    with pytest.raises(ValueError, match="fit_backend"):
        agents.ValueSim(fit_backend="cuda")
    with pytest.raises(ValueError, match="fit_backend"):
        DistValueSim(fit_backend="hip")


def test_command_lines_list_the_flag():
    import play
    p = play.build_parser()
    assert p.parse_args([]).fit_backend == "torch" and p.parse_args(["--fit_backend", "hip"]).fit_backend == "hip"
    assert "--fit_backend" in p.format_help()
    with pytest.raises(SystemExit):
        p.parse_args(["--fit_backend", "triton"])
    for script in ("selfplay_online.py", "fit_timing.py"):
        assert "--fit_backend" in open(os.path.join(ROOT, "scripts", script)).read(), script


def test_fit_kernels_use_no_scratch_memory(tmp_path):
    """every kernel of csrc/valuenet_fit.hip (csrc/fit_mma.h's shared ones included): no private segment, no spilled registers (read from the built code object)"""
    import shutil
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    obj = os.path.join(ROOT, "tetris_mcts_amd", "csrc", "_obj", "valuenet_fit.o")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no llvm binutils")
    if not os.path.exists(obj):
        pytest.skip("HIP objects not built")
    local = str(tmp_path / "valuenet_fit.o")
    shutil.copy(obj, local)
    subprocess.check_call([objdump, "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    cos = [f for f in os.listdir(tmp_path) if f.startswith("valuenet_fit.o.") and "amdgcn" in f]
    assert cos, "no device code object in " + obj
    notes = subprocess.check_output([readelf, "--notes", str(tmp_path / cos[0])]).decode()
    found = re.findall(r"\.name:\s+(\S+)\s.*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", notes, re.S)
    names = [n for n, _, _, _ in found]
    for want in ("k_vf_conv_fwd", "k_fit_fc1_fwd", "k_vf_head", "k_vf_fc1_dw", "k_fit_fc1_bwd_data", "k_vf_conv_bwd_data", "k_vf_conv_dw",
                 "k_fit_reduce", "k_fit_loss", "k_fit_val_moments"):
        assert any(want in n for n in names), want
    assert len(found) >= 15
    for name, scratch, sspill, vspill in found:
        assert ("k_vf_" in name or "k_fit_" in name) and "k_vn_conv" not in name and "k_vn_fc1" not in name, name
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, (name, scratch, sspill, vspill)


def test_the_source_has_no_atomics():
    for f in ("valuenet_fit.hip", "fit_mma.h"):
        src = open(os.path.join(ROOT, "tetris_mcts_amd", "csrc", f)).read().lower()
        code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
        assert "atomic" not in code and "hipmalloc" not in code and "synchronize" not in code and "memcpy" not in code, f


def test_the_yardstick_has_a_denominator_in_every_regime():
    """torch's own fp32 gradients differ from its fp64 gradients in every tensor of the small cases (the large batches are
    checked on the GPU box, where the references are computed anyway); the dead-ReLU case's upstream gradients are identically
    zero in fp64 and in fp32"""
    import fit_hip_cases as FC
    torch.set_num_threads(4)
    for name, case in FC.cases(full=False).items():
        if case["batch"] > 128:
            continue
        g64, l64 = FC.reference(case, torch.float64)
        g32, l32 = FC.reference(case, torch.float32)
        for t, a, b in zip(FC.TENSORS, g32, g64):
            assert np.isfinite(b).all() and np.abs(b).max() > 0 and np.abs(a - b).max() > 0, (name, t)
        assert all(np.isfinite(l64)) and l64[0] != 0
    case = FC.dead_relu_case()
    for dt in (torch.float64, torch.float32):
        g, _ = FC.reference(case, dt)
        for t, a in zip(FC.TENSORS, g):
            zero = t in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias", "fc1.weight")
            assert (np.abs(a).max() == 0) == zero, (t, dt)


def test_the_yardstick_has_a_denominator_in_the_large_batch_regimes():
    """the cases past fit_hip_cases.BATCHES (batch 257 and 1 025: more splits of fc1's weight gradient than its second stage has
    groups): finite references, and torch's fp32 gradients differ from its fp64 gradients in every tensor"""
    import fit_hip_cases as FC
    torch.set_num_threads(4)
    large = FC.large_cases()
    assert sorted(c["batch"] for c in large.values()) == [257, 1025, 1025, 1025]
    null = large["fresh net, batch 1025, unweighted, idx NULL"]
    rows = np.concatenate([null["data"][0][:1025].astype(np.float32), null["data"][1][:1025].reshape(-1, 1)], 1)
    assert null["idx"] is None and len(np.unique(rows, axis=0)) == 1025          # 1 025 distinct rows (a state with its value)
    for name, case in large.items():
        g64, l64 = FC.reference(case, torch.float64)
        g32, l32 = FC.reference(case, torch.float32)
        for t, a, b in zip(FC.TENSORS, g32, g64):
            assert np.isfinite(a).all() and np.isfinite(b).all() and np.abs(b).max() > 0 and np.abs(a - b).max() > 0, (name, t)
        assert all(np.isfinite(l64)) and all(np.isfinite(l32)) and l64[0] != 0
        assert l32[0] != l64[0] and l32[1] != l64[1], (name, "the loss outputs' denominators")
