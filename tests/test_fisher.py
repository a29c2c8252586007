"""Elastic weight consolidation without a GPU: the command line's flag and exits, the C refusals, the workspace arithmetic, the
yardstick's denominators, the numpy statement of the penalty, train_data's refusals and the new kernels' register notes."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import fisher_cases as K
import fit_hip_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    spec_ = importlib.util.spec_from_file_location("tm_train_cli_ewc", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


def test_train_cli_has_ewc_lambda():
    cli = _cli()
    d = vars(cli.build_parser().parse_args([]))
    assert d["ewc"] is False and d["ewc_lambda"] is None
    a = cli.build_parser().parse_args(["--ewc", "--ewc_lambda", "2.5"])
    assert a.ewc is True and a.ewc_lambda == 2.5 and type(a.ewc_lambda) is float
    # accepted by the checks: --ewc with a lambda, with and without --new (0 is a lambda too)
    for flags in (["--ewc", "--ewc_lambda", "1"], ["--ewc", "--ewc_lambda", "0"], ["--ewc", "--ewc_lambda", "1", "--new"]):
        args = cli.build_parser().parse_args(flags + ["--data_paths", "x"])
        cli.check_args(args)


@pytest.mark.parametrize("flags,words", [
    (["--ewc"], ("Fisher", "--ewc_lambda", "scale of the loss", "default of 1")),
    (["--head", "dist", "--ewc"], ("Fisher", "value net only")),
    (["--head", "dist", "--ewc", "--ewc_lambda", "1"], ("Fisher", "value net only")),
    (["--ewc_lambda", "1"], ("needs --ewc",)),
    (["--ewc", "--ewc_lambda", "-0.5"], ("--ewc_lambda", "at least 0")),
    (["--ewc", "--ewc_lambda", "nan"], ("--ewc_lambda", "finite")),
    (["--ewc", "--ewc_lambda", "inf"], ("--ewc_lambda", "finite")),
    (["--ewc", "--ewc_lambda", "1", "--fit_backend", "torch"], ("--fit_backend hip",))])
def test_train_cli_exits_before_anything_is_imported(flags, words, monkeypatch):
    cli = _cli()
    import builtins
    real = builtins.__import__

    def no_package(name, *a, **k):
        assert not name.startswith("tetris_mcts_amd"), "imported before the refusal"
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_package)
    with pytest.raises(SystemExit) as e:
        cli.main(["--data_paths", "x"] + flags)
    for w in words:
        assert w in str(e.value.code), (w, e.value.code)


def _aligned(n_bytes=256):
    buf = (C.c_char * (n_bytes + 16))()
    return buf, (C.addressof(buf) + 15) // 16 * 16


def test_refused_arguments_without_a_gpu():
    """refused before anything touches the device: the pointers are never dereferenced"""
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    keep, b = _aligned()
    for fn in (lib.tm_valuenet_fit_fisher, lib.tm_valuenet_fit_fisher_packed):
        good = [b, b, b, b, b, b, None, 8, 4, 1, 0.1, b, b, None]
        for k in (0, 1, 2, 3, 4, 5, 11, 12):                     # every pointer but idx
            bad = list(good)
            bad[k] = None
            assert fn(*bad) == 1, (fn, k)                           # hipErrorInvalidValue
        for n in (0, -5):
            assert fn(*(good[:7] + [n] + good[8:])) == 1
        for slab in (0, -1, (1 << 20) + 1):
            assert fn(*(good[:8] + [slab] + good[9:])) == 1
        for off in (4, 8):                                          # a workspace that is not 16-byte aligned
            assert fn(*(good[:12] + [b + off] + good[13:])) == 1
    good = [b, b, b + 2, b, b, b, None, 8, 4, 1, 0.1, b, b, None]    # packed observations that are not 4-byte aligned
    assert lib.tm_valuenet_fit_fisher_packed(*good) == 1
    pen = [b, b, b, 16, 1.0, b, b, b, None]
    for k in (0, 1, 2, 5, 6, 7):
        bad = list(pen)
        bad[k] = None
        assert lib.tm_ewc_penalty(*bad) == 1, k
    for n in (0, -1):
        assert lib.tm_ewc_penalty(*(pen[:3] + [n] + pen[4:])) == 1
    for lam in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert lib.tm_ewc_penalty(*(pen[:4] + [lam] + pen[5:])) == 1, lam
    assert lib.tm_ewc_penalty(*(pen[:7] + [b + 4] + pen[8:])) == 1
    del keep


def test_workspace_arithmetic():
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    assert K.FISHER_EXTRA == (K.N_LEARN + 3) // 4 * 4 + 2 * K.N_LEARN and (2 * K.N_LEARN) % 4 == 0
    for slab in (1, 3, 32, 33, 64, 257, 1024, 4096, 1 << 20):
        base = lib.tm_valuenet_fit_workspace(slab)
        assert base > 0 and base % 4 == 0
        assert lib.tm_valuenet_fit_fisher_workspace(slab) == base + K.FISHER_EXTRA, slab
    for slab in (0, -1, (1 << 20) + 1):
        assert lib.tm_valuenet_fit_fisher_workspace(slab) == -1
    for n in (1, 255, 256, 257, K.N_LEARN):
        w = lib.tm_ewc_penalty_workspace(n)
        assert w % 4 == 0 and 2 * -(-n // 256) <= w < 2 * -(-n // 256) + 4, n
    assert lib.tm_ewc_penalty_workspace(0) == -1 and lib.tm_ewc_penalty_workspace(-7) == -1


@pytest.mark.parametrize("name", ["n 1, weighted, idx", "n 3, unweighted, idx NULL"])
def test_the_rule_has_a_denominator(name):
    case = K.cases()[name]
    f64, f32 = K.references(name, case)
    for t, a, b in zip(FC.TENSORS, f32, f64):
        assert a.shape == b.shape and (b >= 0).all() and np.isfinite(b).all()
        own = np.abs(a - b).max()
        print("%-30s %-14s max F64 %.3e  torch fp32 error %.3e (%.2e of the maximum)" % (name, t, b.max(), own, own / b.max()))
        assert b.max() > 0 and own > 0, (name, t, "the rule's denominator")
    assert sum(len(a) for a in f64) == K.N_LEARN


def test_the_cases_cover_what_they_say():
    cs = K.cases()
    assert sorted((c["n"], c["slab"]) for c in cs.values()) == sorted(
        [(1, 1024), (3, 1024), (5, 1024), (33, 1024), (257, 1024), (129, 64), (70, 32), (64, 1024)])
    assert any(c["weighted"] for c in cs.values()) and any(not c["weighted"] for c in cs.values())
    assert any(c["idx"] is None for c in cs.values())
    assert any(c["idx"] is not None and len(set(c["idx"].tolist())) < c["n"] for c in cs.values()), "an idx with repeats"
    assert (FC.SPW, FC.HEAD_CHUNK, FC.FC_KC) == (4, 32, 256)


def test_penalty_statement_in_numpy():
    """the float32 statement the GPU test compares against: the gradient is grad + fl(fl(lam F) d) with d = fl(p - anchor), the
    loss is the fp64 sum; F = 0 and p = anchor leave the gradient equal by value"""
    p, anchor, fisher, grad = K.penalty_case(1000, 3)
    out, loss = K.penalty_numpy(p, anchor, fisher, grad, 0.75)
    assert out.dtype == np.float32
    d = p - anchor
    k = 123
    assert out[k] == np.float32(grad[k] + np.float32(np.float32(np.float32(0.75) * fisher[k]) * d[k]))
    exact = 0.5 * 0.75 * math.fsum(float(f) * float(x) * float(x) for f, x in zip(fisher, d))
    assert abs(loss - exact) <= 1e-12 * exact and loss > 0
    # the gradient of the loss statement, in fp64, is what the float32 statement adds (to float32 rounding)
    add = out.astype(np.float64) - grad
    want = 0.75 * fisher.astype(np.float64) * d
    assert np.abs(add - want).max() <= 2.0 ** -22 * np.abs(want).max() + 2.0 ** -24 * np.abs(grad).max()
    for kw in (dict(zero_fisher=True), dict(at_anchor=True)):
        p, anchor, fisher, grad = K.penalty_case(300, 4, **kw)
        out, loss = K.penalty_numpy(p, anchor, fisher, grad, 2.0)
        assert (out == grad).all() and loss == 0.0
    out, _ = K.penalty_numpy(p, anchor, fisher, grad, 0.0)
    assert (out == grad).all()


def _cpu_model():
    from tetris_mcts_amd import model as M
    mdl = M.Model_VV.__new__(M.Model_VV)
    mdl.device, mdl.backend = torch.device("cpu"), "torch"
    mdl._flat = mdl._prepared = mdl._scratch = None
    mdl.optimizer = None
    mdl.fisher = mdl.ewc_anchor = None
    mdl.model = M.Net()
    return mdl


def test_train_data_refuses_a_bad_ewc_before_the_optimiser_is_flattened():
    from tetris_mcts_amd import train as T
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_training.npz"))
    batch = [torch.from_numpy(g[k].copy()) for k in ("tr_states", "tr_values", "tr_variances", "tr_weights")]
    mdl = _cpu_model()
    opt = mdl._optimizer()
    kw = dict(batch_size=16, max_iters=2, iters_per_val=10, log=False)
    good = torch.zeros(T.EWC_PARAMS)
    assert T.EWC_PARAMS == K.N_LEARN

    class OnGpu:
        """stands for a float32 CUDA tensor of the right length where there is no GPU"""
    bad = [
        (dict(fisher=good, anchor=good, lam=1.0), "torch", "fit_backend='hip'"),
        (dict(fisher=good, anchor=good, lam=1.0), "hip_dist", "fit_backend='hip'"),
        (dict(fisher=good, anchor=good, lam=1.0), "hip", "CUDA"),                      # CPU tensors
        (dict(fisher=good.double(), anchor=good, lam=1.0), "hip", "fisher"),
        (dict(fisher=good[:-1], anchor=good, lam=1.0), "hip", "fisher"),
        (dict(fisher=None, anchor=good, lam=1.0), "hip", "fisher"),
        (dict(fisher=good, lam=1.0), "hip", "dict"),
        ("yes", "hip", "dict"),
    ]
    for ewc, backend, word in bad:
        with pytest.raises(ValueError, match=word):
            T.train_data(mdl.model, opt, batch, fit_backend=backend, ewc=ewc, **kw)
        assert opt._flat is None, "refused before the optimiser is flattened"
    # lam: checked after the tensors; with tensors that pass, through check_ewc itself

    class Fake(torch.Tensor):
        is_cuda = True
    fake = good.as_subclass(Fake)
    assert fake.is_cuda and fake.dtype == torch.float32
    for lam in (-1.0, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError, match="lam"):
            T.check_ewc(dict(fisher=fake, anchor=fake, lam=lam), "hip")
    assert T.check_ewc(None, "torch") is None
    f, a, lam = T.check_ewc(dict(fisher=fake, anchor=fake, lam=3), "hip")
    assert lam == 3.0 and f.numel() == K.N_LEARN
    # the model's wrapper: a bad lambda, a backend that cannot; and without a Fisher the fit is the unpenalised one
    for lam in (-1.0, float("nan"), True, "1"):
        with pytest.raises(ValueError, match="ewc_lambda"):
            mdl.train_data(batch, ewc_lambda=lam, fit_backend="hip", **kw)
    with pytest.raises(ValueError, match="fit_backend='hip'"):
        mdl.train_data(batch, ewc_lambda=1.0, **kw)
    assert opt._flat is None


def test_checkpoint_keys_without_and_with_a_fisher(tmp_path):
    """a model without a Fisher writes exactly the two keys it always wrote; with one, two more, shaped like the parameters, and
    load() restores them (host tensors: the round trip needs no GPU)"""
    from tetris_mcts_amd.model import PARAM_ORDER
    mdl = _cpu_model()
    path = str(tmp_path / "pytorch_model" / "model_checkpoint")
    mdl.save(path, verbose=False)
    assert sorted(torch.load(path, map_location="cpu")) == ["model_state_dict", "optimizer_state_dict"]
    rng = torch.Generator().manual_seed(5)
    mdl.fisher, mdl.ewc_anchor = torch.rand(K.N_LEARN, generator=rng), torch.randn(K.N_LEARN, generator=rng)
    mdl.save(path, verbose=False)
    ck = torch.load(path, map_location="cpu")
    assert sorted(ck) == ["ewc_anchor", "fisher", "model_state_dict", "optimizer_state_dict"]
    sd = mdl.model.state_dict()
    for key in ("fisher", "ewc_anchor"):
        assert list(ck[key]) == PARAM_ORDER[:10]
        assert all(ck[key][k].shape == sd[k].shape and ck[key][k].device.type == "cpu" for k in PARAM_ORDER[:10])
    other = _cpu_model()
    other.load(path, verbose=False)
    assert torch.equal(other.fisher, mdl.fisher) and torch.equal(other.ewc_anchor, mdl.ewc_anchor)
    plain = str(tmp_path / "plain")
    _cpu_model().save(plain, verbose=False)
    other.load(plain, verbose=False)
    assert other.fisher is None and other.ewc_anchor is None
    ck["fisher"]["head.conv2.bias"] = torch.zeros(31)
    torch.save(ck, path)
    with pytest.raises(ValueError, match="fisher"):
        other.load(path, verbose=False)


def test_new_kernels_use_no_scratch_memory(tmp_path):
    """the squared forms of the weight-gradient kernels keep two sets of accumulators in registers: no private segment, no
    spills, read from the code object inside the built HIP object"""
    import shutil
    import subprocess
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no llvm binutils")
    want = {"k_vf_conv_dwILi32ELi16ELi6ELi3EN9tmcts_fit11DenseStatesELb1E", "k_vf_conv_dwILi32ELi18ELi8ELi3EN9tmcts_fit11DenseStatesELb1E",
            "k_vf_conv_dwILi1ELi20ELi10ELi1EN9tmcts_fit11DenseStatesELb1E", "k_vf_conv_dwILi1ELi20ELi10ELi1EN9tmcts_fit12PackedStatesELb1E",
            "k_vf_fc1_dwILi2ELb1E", "k_vf_head_partILb1E", "k_vf_conv_bias_partILb1E", "k_vf_fisher_add", "k_ewc_penalty", "k_ewc_loss"}
    seen = set()
    for src in ("valuenet_fit", "yogi"):
        obj = os.path.join(ROOT, "tetris_mcts_amd", "csrc", "_obj", src + ".o")
        if not os.path.exists(obj):
            pytest.skip("HIP objects not built")
        local = str(tmp_path / (src + ".o"))
        shutil.copy(obj, local)
        subprocess.check_call([objdump, "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        cos = [f for f in os.listdir(tmp_path) if f.startswith(src + ".o.") and "amdgcn" in f]
        assert cos, "no device code object in " + obj
        notes = subprocess.check_output([readelf, "--notes", str(tmp_path / cos[0])]).decode()
        for name, scratch, spills in re.findall(r"\.name:\s+(\S+)\s.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", notes, re.S):
            for w in want:
                if w in name:
                    seen.add(w)
                    assert int(scratch) == 0 and int(spills) == 0, (name, scratch, spills)
    assert seen == want, want - seen
