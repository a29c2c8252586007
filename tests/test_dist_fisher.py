"""Elastic weight consolidation for the distributional head without a GPU: the C refusals of the Fisher pass
(csrc/distnet_fit.hip: tm_distnet_fit_fisher), its workspace arithmetic, the cases and the yardstick's denominators
(tests/dist_fisher_cases.py), train_data's and Model_Dist's refusals, the checkpoint's keys, the command line's flag and exits, and
the new kernels' register notes."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import dist_fisher_cases as K
import dist_fit_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    spec_ = importlib.util.spec_from_file_location("tm_train_cli_ewc_dist", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


# ---- the command line ----
def test_train_cli_accepts_ewc_dist_with_the_head_and_with_dist_nodes():
    cli = _cli()
    d = vars(cli.build_parser().parse_args([]))
    assert d["ewc_dist"] is False and d["ewc"] is False and d["ewc_lambda"] is None
    for flags in (["--head", "dist", "--ewc_dist", "--ewc_lambda", "1"],
                  ["--head", "dist", "--ewc_dist", "--ewc_lambda", "0", "--new"],
                  ["--head", "dist", "--td", "--td_lambda", "0.9", "--bootstrap", "net", "--ewc_dist", "--ewc_lambda", "2.5"],
                  ["--head", "dist", "--td", "--bootstrap", "search", "--ewc_dist", "--ewc_lambda", "1"],
                  ["--head", "dist", "--td", "--td_lambda", "0.5", "--bootstrap", "search", "--ewc_dist", "--ewc_lambda", "1"],
                  ["--dist_nodes", "--ewc_dist", "--ewc_lambda", "1"],
                  ["--dist_nodes", "--weighted", "--weighted_mode", "1", "--ewc_dist", "--ewc_lambda", "0.25"]):
        argv = flags + ["--data_paths", "x"]
        args = cli.build_parser().parse_args(argv)
        cli.check_args(args, argv)
        assert args.ewc_dist is True and type(args.ewc_lambda) is float


@pytest.mark.parametrize("flags,words", [
    (["--ewc_dist", "--ewc_lambda", "1"], ("--ewc_dist", "--head dist", "--dist_nodes", "--ewc")),
    (["--nodes", "--td", "--ewc_dist", "--ewc_lambda", "1"], ("--ewc_dist", "--head dist", "--ewc")),
    (["--head", "dist", "--ewc_dist"], ("--ewc_dist", "--ewc_lambda", "scale of the loss")),
    (["--dist_nodes", "--ewc_dist"], ("--ewc_dist", "--ewc_lambda")),
    (["--head", "dist", "--ewc_dist", "--ewc_lambda", "-0.5"], ("--ewc_lambda", "at least 0")),
    (["--head", "dist", "--ewc_dist", "--ewc_lambda", "nan"], ("--ewc_lambda", "finite")),
    (["--dist_nodes", "--ewc_dist", "--ewc_lambda", "inf"], ("--ewc_lambda", "finite")),
    (["--head", "dist", "--ewc_dist", "--ewc_lambda", "1", "--fit_backend", "torch"], ("--ewc_dist", "--fit_backend hip")),
    # --ewc stays the value net's: its present words, and now the flag that does it for the head
    (["--head", "dist", "--ewc"], ("Fisher", "value net only", "--ewc_dist")),
    (["--head", "dist", "--ewc", "--ewc_lambda", "1"], ("Fisher", "value net only", "--ewc_dist")),
    (["--dist_nodes", "--ewc", "--ewc_lambda", "1"], ("Fisher", "value net only", "--dist_nodes", "--ewc", "--ewc_dist")),
    (["--ewc_lambda", "1"], ("needs --ewc",)),
    (["--head", "dist", "--ewc_lambda", "1"], ("needs --ewc",))])
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


# ---- the C entry points ----
def _aligned(n_bytes=256):
    buf = (C.c_char * (n_bytes + 16))()
    return buf, (C.addressof(buf) + 15) // 16 * 16


def test_refused_arguments_without_a_gpu():
    """refused before anything touches the device: the pointers are never dereferenced"""
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    keep, b = _aligned()
    # params, states, target, target_stride, weight, idx, n, slab, atoms, weighted, fisher, workspace, stream
    good = [b, b, b, 50, b, None, 8, 4, 50, 1, b, b, None]
    for fn in (lib.tm_distnet_fit_fisher, lib.tm_distnet_fit_fisher_packed):
        for k in (0, 1, 2, 4, 10, 11):                               # every pointer but idx
            bad = list(good)
            bad[k] = None
            assert fn(*bad) == 1, (fn, k)                           # hipErrorInvalidValue
        for n in (0, -5):
            assert fn(*(good[:6] + [n] + good[7:])) == 1
        for slab in (0, -1, (1 << 20) + 1):
            assert fn(*(good[:7] + [slab] + good[8:])) == 1
        for atoms in (0, -1, 65):
            assert fn(*(good[:8] + [atoms] + good[9:])) == 1
        for stride in (49, 0, -64):                                 # target_stride < atoms
            assert fn(*(good[:3] + [stride] + good[4:])) == 1
        for off in (4, 8):                                          # a workspace, or parameters, not 16-byte aligned
            assert fn(*(good[:11] + [b + off] + good[12:])) == 1
            assert fn(*([b + off] + good[1:])) == 1
    assert lib.tm_distnet_fit_fisher_packed(*(good[:1] + [b + 2] + good[2:])) == 1      # observations not 4-byte aligned
    del keep


def test_workspace_arithmetic():
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    for atoms in (1, 7, 17, 50, 64):
        p = DC.n_params(atoms)
        assert p == 279232 + 129 * atoms and K.fisher_extra(atoms) == (p + 3) // 4 * 4 + (2 * p + 3) // 4 * 4
        for slab in (1, 3, 32, 33, 64, 257, 1024, 4096, 1 << 20):
            base = lib.tm_distnet_fit_workspace(slab, atoms)
            assert base > 0 and base % 4 == 0
            assert lib.tm_distnet_fit_fisher_workspace(slab, atoms) == base + K.fisher_extra(atoms), (slab, atoms)
    assert K.fisher_extra(1) % 4 == 0 and (2 * DC.n_params(1)) % 4 != 0, "an odd P: the accumulator's size is rounded up too"
    for slab, atoms in ((0, 50), (-1, 50), ((1 << 20) + 1, 50), (64, 0), (64, 65), (64, -3)):
        assert lib.tm_distnet_fit_fisher_workspace(slab, atoms) == -1


# ---- the cases and the rule ----
def test_the_cases_cover_what_they_say():
    cs = K.cases()
    assert list(cs) == K.case_names()
    fixture = sorted((c["n"], c["slab"]) for k, c in cs.items() if k.startswith("fixture, n"))
    assert fixture == sorted([(1, 1024), (3, 1024), (4, 1024), (5, 1024), (33, 1024), (257, 1024), (129, 64), (70, 32)])
    assert (K.SPW, K.HEAD_CHUNK, K.FC_KC) == (4, 32, 256)
    others = {k.split(",")[0]: (c["n"], c["atoms"], c["tstride"]) for k, c in cs.items() if not k.startswith("fixture, n")}
    assert others == {"seed1": (5, 1, 1), "seed7": (33, 7, 64), "seed17": (33, 17, 17), "seed64": (33, 64, 64),
                      "peaked50_50": (33, 50, 50), "fitted": (64, 50, 50), "fixture": (33, 50, 50)}
    assert any(c["weighted"] for c in cs.values()) and any(not c["weighted"] for c in cs.values())
    assert cs["fixture, n 70, slab 32, unweighted, idx NULL"]["idx"] is None
    big = cs[K.THREE_SLABS]
    assert big["idx"] is not None and len(set(big["idx"].tolist())) < big["n"], "an idx with repeats"
    assert -(-big["n"] // big["slab"]) == 3 and big["n"] % big["slab"] == 1, "three slabs, the last of one row"
    off = cs["fixture, targets off 1, n 33, weighted, idx"]
    sums = off["data"][1][K.rows_of(off)].sum(1)
    assert np.abs(sums - 1).max() > 0.2 and np.abs(cs[K.N33]["data"][1].sum(1) - 1).max() < 1e-5
    for c in cs.values():      # every row a case names exists among the kept rows of DC's candidate set
        assert len(c["data"][0]) >= (1 - DC.KINK_CAP) * DC.CANDIDATES and K.rows_of(c).max() < len(c["data"][0])


@pytest.mark.parametrize("name", [K.ONE_ROW, "fixture, n 3, unweighted, idx NULL", "seed7, n 33, stride 64, weighted, idx"])
def test_the_rule_has_a_denominator(name):
    case = K.cases()[name]
    f64, f32 = K.references(name, case)
    for t, a, b, size in zip(K.TENSORS, f32, f64, DC.sizes(case["atoms"])):
        assert a.shape == b.shape == (size,) and (b >= 0).all() and np.isfinite(b).all()
        own = np.abs(a - b).max()
        print("%-44s %-14s max F64 %.3e  torch fp32 error %.3e (%.2e of the maximum)" % (name, t, b.max(), own, own / b.max()))
        assert b.max() > 0 and own > 0, (name, t, "the rule's denominator")
    assert sum(len(a) for a in f64) == DC.n_params(case["atoms"])


def test_one_atom_gives_a_fisher_of_exact_zeros():
    """atoms = 1: log p = 0 whatever the weights are, every gradient is 0, and so is every square"""
    case = K.cases()[K.ZERO_CASE]
    f64, f32 = K.references(K.ZERO_CASE, case)
    assert all((a == 0).all() and (b == 0).all() for a, b in zip(f32, f64))


# ---- Python: train_data, Model_Dist ----
def _cpu_model(atoms=50, seed=0):
    from tetris_mcts_amd.model_distributional import Model_Dist
    return Model_Dist(atoms=atoms, device="cpu", seed=seed, backend="torch")


def _cpu_batch(n=40, atoms=50):
    s, t, w = DC.dataset(n, atoms, 3)
    states = torch.zeros(n, 1, 22, 10)
    states[:, 0, 2:] = torch.from_numpy(s.reshape(n, 20, 10).astype(np.float32))
    return [states, torch.from_numpy(t), torch.from_numpy(w).reshape(n, 1)]


def test_train_data_refuses_a_bad_ewc_dist_before_the_optimiser_is_flattened():
    from tetris_mcts_amd import train as T
    mdl = _cpu_model()
    opt = mdl._fused_optimizer(commit=False)
    batch = _cpu_batch()
    kw = dict(batch_size=16, max_iters=2, iters_per_val=10, log=False)
    n = DC.n_params(50)
    good = torch.zeros(n)
    bad = [
        (dict(fisher=good, anchor=good, lam=1.0), "torch", "fit_backend='hip_dist'"),
        (dict(fisher=good, anchor=good, lam=1.0), "hip", "fit_backend='hip_dist'"),
        (dict(fisher=good, anchor=good, lam=1.0), "hip_dist", "CUDA"),                 # CPU tensors
        (dict(fisher=good.double(), anchor=good, lam=1.0), "hip_dist", "fisher"),
        (dict(fisher=good[:-1], anchor=good, lam=1.0), "hip_dist", "fisher"),
        (dict(fisher=torch.zeros(T.EWC_PARAMS), anchor=good, lam=1.0), "hip_dist", "fisher"),      # the value net's length
        (dict(fisher=None, anchor=good, lam=1.0), "hip_dist", "fisher"),
        (dict(fisher=good, lam=1.0), "hip_dist", "dict"),
        ("yes", "hip_dist", "dict"),
    ]
    for ewc_dist, backend, word in bad:
        with pytest.raises(ValueError, match=word):
            T.train_data(mdl.model, opt, batch, fit_backend=backend, ewc_dist=ewc_dist, **kw)
        assert opt._flat is None, "refused before the optimiser is flattened"
    # both penalties at once; ewc itself stays the value net's, with its message
    vv = torch.zeros(T.EWC_PARAMS)
    with pytest.raises(ValueError, match="not both"):
        T.train_data(mdl.model, opt, batch, fit_backend="hip_dist", ewc=dict(fisher=vv, anchor=vv, lam=1.0),
                     ewc_dist=dict(fisher=good, anchor=good, lam=1.0), **kw)
    with pytest.raises(ValueError, match="fit_backend='hip'"):
        T.train_data(mdl.model, opt, batch, fit_backend="hip_dist", ewc=dict(fisher=vv, anchor=vv, lam=1.0), **kw)
    assert opt._flat is None

    # lam: checked after the tensors; with tensors that pass, through check_ewc_dist itself
    class Fake(torch.Tensor):
        is_cuda = True
    fake = good.as_subclass(Fake)
    assert fake.is_cuda and fake.dtype == torch.float32
    for lam in (-1.0, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError, match="lam"):
            T.check_ewc_dist(dict(fisher=fake, anchor=fake, lam=lam), "hip_dist", mdl.model)
    assert T.check_ewc_dist(None, "torch", mdl.model) is None
    f, a, lam = T.check_ewc_dist(dict(fisher=fake, anchor=fake, lam=3), "hip_dist", mdl.model)
    assert lam == 3.0 and f.numel() == a.numel() == n
    # the length follows the net's atoms; a net that is no head is refused
    with pytest.raises(ValueError, match="fisher"):
        T.check_ewc_dist(dict(fisher=fake, anchor=fake, lam=1.0), "hip_dist", _cpu_model(atoms=7).model)
    from tetris_mcts_amd.model import Net
    with pytest.raises(ValueError, match="model_distributional.Net"):
        T.check_ewc_dist(dict(fisher=fake, anchor=fake, lam=1.0), "hip_dist", Net())


def test_model_dist_train_data_refuses_a_bad_ewc_lambda():
    mdl = _cpu_model()
    batch = _cpu_batch()
    kw = dict(batch_size=16, max_iters=2, iters_per_val=10, log=False)
    assert mdl.fisher is None and mdl.ewc_anchor is None
    for lam in (-1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="ewc_lambda"):
            mdl.train_data(batch, fit_backend="hip_dist", ewc_lambda=lam, **kw)
    with pytest.raises(ValueError, match="fit_backend='hip_dist'"):
        mdl.train_data(batch, ewc_lambda=1.0, **kw)
    with pytest.raises(ValueError, match="not both"):
        mdl.train_data(batch, fit_backend="hip_dist", ewc_lambda=1.0, ewc_dist=dict(), **kw)
    assert getattr(mdl, "optimizer", None) is None, "a refused fit leaves the model as it was"
    with pytest.raises(ValueError, match="GPU"):
        mdl.compute_fisher(batch)


def test_offline_fits_refuse_ewc_lambda_with_another_backend():
    from tetris_mcts_amd import offline as O
    with pytest.raises(ValueError, match="ewc_lambda needs fit_backend='hip_dist'"):
        O.fit_episodes_dist(_cpu_model(), ["nowhere"], fit_backend="torch", ewc_lambda=1.0)
    with pytest.raises(ValueError, match="fit_backend='hip_dist'"):
        O.fit_dist_nodes(_cpu_model(), ["nowhere"], fit_backend="torch", ewc_lambda=1.0)


def test_checkpoint_keys_without_and_with_a_fisher(tmp_path):
    """a model without a Fisher writes exactly the two keys it always wrote; with one, two more, shaped like the parameters, and
    load() restores them (host tensors: the round trip needs no GPU)"""
    from tetris_mcts_amd.model_distributional import PARAM_ORDER
    mdl = _cpu_model(atoms=17)
    n = DC.n_params(17)
    path = str(tmp_path / "pytorch_model" / "model_checkpoint_dist")
    mdl.save(path, verbose=False)
    assert sorted(torch.load(path, map_location="cpu")) == ["model_state_dict", "optimizer_state_dict"]
    rng = torch.Generator().manual_seed(5)
    mdl.fisher, mdl.ewc_anchor = torch.rand(n, generator=rng), torch.randn(n, generator=rng)
    mdl.save(path, verbose=False)
    ck = torch.load(path, map_location="cpu")
    assert sorted(ck) == ["ewc_anchor", "fisher", "model_state_dict", "optimizer_state_dict"]
    sd = mdl.model.state_dict()
    for key in ("fisher", "ewc_anchor"):
        assert list(ck[key]) == PARAM_ORDER
        assert all(ck[key][k].shape == sd[k].shape and ck[key][k].device.type == "cpu" for k in PARAM_ORDER)
    other = _cpu_model(atoms=17, seed=1)
    other.load(path, verbose=False)
    assert torch.equal(other.fisher, mdl.fisher) and torch.equal(other.ewc_anchor, mdl.ewc_anchor)
    assert torch.equal(other.flat_params(), mdl.flat_params())
    plain = str(tmp_path / "plain")
    _cpu_model(atoms=17, seed=2).save(plain, verbose=False)
    other.load(plain, verbose=False)
    assert other.fisher is None and other.ewc_anchor is None, "a file without a Fisher clears the model's"
    # one of the two keys alone restores neither
    half = dict(ck)
    del half["ewc_anchor"]
    torch.save(half, path)
    other.fisher = other.ewc_anchor = torch.zeros(n)
    other.load(path, verbose=False)
    assert other.fisher is None and other.ewc_anchor is None
    for key in ("fisher", "ewc_anchor"):
        wrong = {k: dict(v) if k in ("fisher", "ewc_anchor") else v for k, v in ck.items()}
        wrong[key]["seq.conv2.bias"] = torch.zeros(31)
        torch.save(wrong, path)
        with pytest.raises(ValueError, match=repr(key)):
            other.load(path, verbose=False)
    # another atom count is refused as before, whatever else the file carries
    with pytest.raises(ValueError, match="17 atoms"):
        _cpu_model(atoms=50).load(plain, verbose=False)


# ---- the kernels' register notes ----
def test_new_kernels_use_no_scratch_memory(tmp_path):
    """the squared forms of the weight-gradient kernels (conv2's holds three sets of accumulators) and k_df_fisher_add: no private
    segment, no spills, read from the code object inside the built HIP object"""
    import shutil
    import subprocess
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no llvm binutils")
    want = {"k_df_conv_dwILi32ELi7ELi136ELi4ELi64ELi64ELi4EN9tmcts_fit11DenseStatesELb1E",
            "k_df_conv_dwILi1ELi10ELi0ELi7ELi133ELi136ELi1EN9tmcts_fit11DenseStatesELb1E",
            "k_df_conv_dwILi1ELi10ELi0ELi7ELi133ELi136ELi1EN9tmcts_fit12PackedStatesELb1E",
            "k_df_fc_dwILi64ELi128ELi2ELb1E", "k_df_fc_dwILi128ELi2048ELi2ELb1E", "k_df_head_partILb1E", "k_df_conv_bias_partILb1E",
            "k_df_fisher_add"}
    obj = os.path.join(ROOT, "tetris_mcts_amd", "csrc", "_obj", "distnet_fit.o")
    if not os.path.exists(obj):
        pytest.skip("HIP objects not built")
    local = str(tmp_path / "distnet_fit.o")
    shutil.copy(obj, local)
    subprocess.check_call([objdump, "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    cos = [f for f in os.listdir(tmp_path) if f.startswith("distnet_fit.o.") and "amdgcn" in f]
    assert cos, "no device code object in " + obj
    notes = subprocess.check_output([readelf, "--notes", str(tmp_path / cos[0])]).decode()
    seen = set()
    for name, scratch, spills in re.findall(r"\.name:\s+(\S+)\s.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", notes, re.S):
        for w in want:
            if w in name:
                seen.add(w)
                assert int(scratch) == 0 and int(spills) == 0, (name, scratch, spills)
    assert seen == want, want - seen
