"""The split-precision fc1 of the value net (fc1="bf16x3" of the "hip_bf16x3" backend, valuenet_fc1_x3.inc) on the build machine: a
numpy emulation of its numerics contract at the hidden layer, where a dropped plane shows, and at the
outputs; the C ABI declares and exports it; play.py and the agents pass it on; the build recipe names the kernel's file; and the
built code object shows k_vn_fc1_x3 without private segment or spills."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_split_precision import OFF, PRODUCTS, _tol, forward, split3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fc1(P, a3, mode):
    """ReLU(fc1) of a3 [n, 1792] (fp32 values): "f64", "f32" (this host's BLAS order) or one of PRODUCTS - each plane product
    summed over k in fp32, the products added in fp32 in the kernel's order, then the bias (the kernel starts from it)"""
    P = np.asarray(P, np.float32)
    W, b = P[OFF["f1w"]:OFF["f1w"] + 458752].reshape(256, 1792), P[OFF["f1b"]:OFF["f1b"] + 256]
    if mode == "f64":
        return np.maximum(a3.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64), 0)
    a3 = a3.astype(np.float32)
    if mode == "f32":
        return np.maximum((a3 @ W.T + b).astype(np.float32), 0)
    wp, xp = split3(W), split3(a3)
    y = np.zeros((a3.shape[0], 256), np.float32)
    for i, j in PRODUCTS[mode]:
        y = (y + xp[j] @ wp[i].T).astype(np.float32)
    return np.maximum((y + b).astype(np.float32), 0)


def _outputs(P, h):
    """the output layer of test_split_precision.forward on hidden units h (fp32)"""
    P = np.asarray(P, np.float32)
    g = lambda k, n: P[OFF[k]:OFF[k] + n]
    o = (h.astype(np.float32) @ g("fow", 512).reshape(2, 256).T + g("fob", 2)).astype(np.float64)
    sg = 1.0 / (1.0 + np.exp(-o))
    return (sg.astype(np.float32) * g("ub", 2) + g("lb", 2)).astype(np.float64)


@pytest.mark.parametrize("pk,ok", [("params", "out"), ("params2", "out2")])
def test_emulated_fc1_split_holds_the_contract(pk, ok):
    z = np.load(os.path.join(GOLDEN, "ref_valuenet.npz"))
    P, S = z[pk], z["states"]
    a3 = forward(P, S, "x3", a3_only=True).astype(np.float32)      # what k_vn_conv_x3 hands to fc1 (fp32 values)
    h64 = _fc1(P, a3, "f64")
    e32 = np.abs(_fc1(P, a3, "f32") - h64).max()
    hx = _fc1(P, a3, "x3")
    ex = np.abs(hx - h64).max()
    print("fc1 alone %s: fp32 %.3e x3 %.3e (%.2fx)" % (pk, e32, ex, ex / e32))
    assert ex <= 2 * e32, (pk, ex, e32)
    for drop in ("x3_nolo", "x3_nomidmid"):
        ed = np.abs(_fc1(P, a3, drop) - h64).max()
        print("   %s %.3e (%.2fx)" % (drop, ed, ed / e32))
        assert ed > 3 * e32, (pk, drop, ed, e32)
    out, tol = _outputs(P, hx), _tol(P)
    assert np.all(np.abs(out - z[ok]).max(axis=0) <= tol), pk
    assert np.all(np.abs(out - forward(P, S, "f64")).max(axis=0) <= tol), pk


def test_library_exports_the_fc1_abi():
    import abi_shape
    from tetris_mcts_amd import model
    abi_shape.check(abi_shape.VALUENET)
    abi_shape.check_defines((("TM_VALUENET_PREPARED_FC1_X3", 688128), ("TM_VALUENET_FC1_FP32", 0), ("TM_VALUENET_FC1_BF16X3", 1),
                             ("TM_VALUENET_PREPARED_X3", 27648)))
    assert 3 * 256 * 1792 // 2 == 688128 == model.PREPARED_FC1_X3
    assert model.VALUENET_FC1 == {"fp32": 0, "bf16x3": 1}
    assert model.VALUENET_BACKEND == {"hip": 0, "hip_bf16x3": 1} and model.HIP_BACKENDS == ("hip", "hip_bf16x3")


def test_play_cli_takes_the_fc1_option():
    import play
    p = play.build_parser()
    assert p.parse_args([]).valuenet_fc1 == "fp32"
    assert p.parse_args(["--valuenet_fc1", "bf16x3"]).valuenet_fc1 == "bf16x3"
    with pytest.raises(SystemExit):
        p.parse_args(["--valuenet_fc1", "bf16"])
    # refused with a message for the distributional head and for the other backends, before anything is built
    for argv in (["--agent_type", "DistValueSim", "--valuenet_backend", "hip_bf16x3", "--valuenet_fc1", "bf16x3"],
                 ["--agent_type", "ValueSimLP", "--valuenet_fc1", "bf16x3"],
                 ["--agent_type", "ValueSim", "--valuenet_backend", "torch", "--valuenet_fc1", "bf16x3"],
                 ["--agent_type", "Vanilla", "--valuenet_fc1", "bf16x3"]):
        with pytest.raises(SystemExit) as e:
            play.main(argv)
        assert "--valuenet_fc1" in str(e.value.code), argv


def test_agents_take_the_fc1_keyword(monkeypatch):
    """the keyword reaches the model the agent builds, and a model with the split fc1 still goes to the native search loop"""
    import inspect
    import tetris_mcts_amd.agents as A
    import sys
    VS = sys.modules["tetris_mcts_amd.agents.ValueSim"]
    assert inspect.signature(A.ValueSim.__init__).parameters["valuenet_fc1"].default == "fp32"
    seen = []

    class FakeModel:
        def __init__(self, **kw):
            seen.append(kw)
            self.backend, self.fc1 = kw.get("backend"), kw.get("fc1", "fp32")

        def load(self):
            pass

        def training(self, mode):
            pass
    from tetris_mcts_amd.agents.agent import TreeAgent
    monkeypatch.setattr(VS, "Model", FakeModel)
    monkeypatch.setattr(TreeAgent, "__init__", lambda self, **kw: None)
    for name in ("ValueSim", "ValueSimLP", "ValueSimC"):
        cls = getattr(A, name)
        del seen[:]
        a = cls(valuenet_backend="hip_bf16x3", valuenet_fc1="bf16x3")
        assert seen == [dict(backend="hip_bf16x3", fc1="bf16x3")], (name, seen)
        assert a.search_model() is a.model, name
        del seen[:]
        cls(valuenet_backend="hip_bf16x3")
        assert seen[0].get("fc1", "fp32") == "fp32", (name, seen)


def test_model_refuses_the_split_fc1_on_other_backends():
    src = open(os.path.join(ROOT, "tetris_mcts_amd", "model.py")).read()
    assert re.search(r'def __init__\(self, backend="hip", device="cuda", seed=None, fc1="fp32"', src)
    from tetris_mcts_amd.model import Model_VV
    for backend in ("hip", "torch", "hip_plain"):
        with pytest.raises(ValueError):
            Model_VV(backend=backend, fc1="bf16x3", device="cpu")
    with pytest.raises(ValueError):
        Model_VV(backend="hip_bf16x3", fc1="x3", device="cpu")


def test_build_rebuilds_valuenet_when_the_fc1_kernel_changes():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "valuenet_fc1_x3.inc" in src
    vn = open(os.path.join(ROOT, "tetris_mcts_amd", "csrc", "valuenet.hip")).read()
    assert re.search(r'#include\s+"valuenet_fc1_x3.inc"', vn)
    assert vn.index('#include "valuenet_x3.inc"') < vn.index('#include "valuenet_fc1_x3.inc"')


def test_fc1_x3_kernels_use_no_scratch_memory(tmp_path):
    """k_vn_fc1_x3 (both shapes) and its prepare kernel: no private segment, no spilled registers - the built code object's
    metadata, as tests/test_fit_hip.py reads the fit's"""
    import shutil
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    obj = os.path.join(ROOT, "tetris_mcts_amd", "csrc", "_obj", "valuenet.o")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no llvm binutils")
    if not os.path.exists(obj):
        pytest.skip("HIP objects not built")
    local = str(tmp_path / "valuenet.o")
    shutil.copy(obj, local)
    subprocess.check_call([objdump, "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    cos = [f for f in os.listdir(tmp_path) if f.startswith("valuenet.o.") and "amdgcn" in f]
    assert cos, "no device code object in " + obj
    notes = subprocess.check_output([readelf, "--notes", str(tmp_path / cos[0])]).decode()
    found = re.findall(r"\.name:\s+(\S+)\s.*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", notes, re.S)
    mine = [f for f in found if "k_vn_fc1_x3" in f[0] or "k_vn_prepare_fc1_x3" in f[0]]
    assert sum("k_vn_fc1_x3" in f[0] for f in mine) == 2 and any("k_vn_prepare_fc1_x3" in f[0] for f in mine), [f[0] for f in found]
    for name, scratch, sspill, vspill in mine:
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, (name, scratch, sspill, vspill)
