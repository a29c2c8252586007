"""Cases and references for the Fisher pass of the distributional head's fit (csrc/distnet_fit.hip: tm_distnet_fit_fisher), shared
by tests/test_dist_fisher.py (CPU: the references alone) and tests/test_gpu_dist_fisher.py (GPU: the kernels against them).

Built on dist_fit_cases (DC): its nets, its dataset, its kink filter and its candidate sets (420 rows, seed 7; the filter's cap of
25 % is asserted by tests/test_dist_fit_hip.py, so 315 rows are kept at the least: every n below fits).

The reference is per-row CPU autograd of model_distributional.Net.log_prob + Model_Dist.loss on ONE row at a time, g^2 / n
accumulated in the dtype, in fp64 (F64) and in fp32 (F32).  The yardstick is measure B of DESIGN.md section 6 as fisher_cases
states it, per parameter tensor:
    max|F_hip - F64| <= 8 max|F32 - F64| + 4 u max|F64|,   u = 2^-24.
A tensor whose F64 is identically zero (every tensor at atoms = 1: log p = 0) is compared for exact zeros instead.

The shapes are the smallest at which each blocking constant of the pass can go wrong: SPW = 4 samples per partial of the
convolutions, the 32-sample chunks of the FC weight gradients' K and HEAD_CHUNK = 32 samples per partial of the bias sums,
FC_KC = 256 samples per split of the FC weight gradients, and the slab.

Run as a program (`python tests/dist_fisher_cases.py digest`) it prints the SHA-256 of one case's Fisher: the second process of the
determinism test."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import dist_fit_cases as DC  # noqa: E402
import heads_numerics as HN  # noqa: E402

TENSORS, U, measure = DC.TENSORS, DC.U, DC.measure
SPW, HEAD_CHUNK, FC_KC = DC.SPW, DC.TILE, DC.FC_KC


def up4(x):
    return (x + 3) // 4 * 4


def fisher_extra(atoms):
    """the floats of tm_distnet_fit_fisher_workspace beyond tm_distnet_fit_workspace: the temporary [P] and the accumulator [P]
    doubles, each rounded up to four floats"""
    p = DC.n_params(atoms)
    return up4(p) + up4(2 * p)


# (name, net, n, slab, weighted, idx: "random" / "repeats" / None, target stride (None: atoms), targets that sum to 1)
_TABLE = (
    ("fixture, n 1, weighted, idx", "fixture", 1, 1024, True, "random", None, True),
    ("fixture, n 3, unweighted, idx NULL", "fixture", 3, 1024, False, None, None, True),
    ("fixture, n 4, weighted, idx", "fixture", 4, 1024, True, "random", None, True),
    ("fixture, n 5, weighted, repeats", "fixture", 5, 1024, True, np.array([7, 2, 7, 7, 2]), None, True),
    ("fixture, n 33, weighted, idx NULL", "fixture", 33, 1024, True, None, None, True),
    ("fixture, n 257, unweighted, idx", "fixture", 257, 1024, False, "random", None, True),
    ("fixture, n 129, slab 64, weighted, repeats", "fixture", 129, 64, True, "repeats", None, True),
    ("fixture, n 70, slab 32, unweighted, idx NULL", "fixture", 70, 32, False, None, None, True),
    ("seed1, n 5, weighted, idx", "seed1", 5, 1024, True, "random", None, True),
    ("seed7, n 33, stride 64, weighted, idx", "seed7", 33, 1024, True, "random", 64, True),
    ("seed17, n 33, unweighted, idx", "seed17", 33, 1024, False, "random", None, True),
    ("seed64, n 33, weighted, idx", "seed64", 33, 1024, True, "random", None, True),
    ("peaked50_50, n 33, weighted, idx", "peaked50_50", 33, 1024, True, "random", None, True),
    ("fitted, n 64, unweighted, idx", "fitted", 64, 1024, False, "random", None, True),
    ("fixture, targets off 1, n 33, weighted, idx", "fixture", 33, 1024, True, "random", None, False),
)
ZERO_CASE = "seed1, n 5, weighted, idx"
ONE_ROW = "fixture, n 1, weighted, idx"
N33 = "fixture, n 33, weighted, idx NULL"
N257 = "fixture, n 257, unweighted, idx"
THREE_SLABS = "fixture, n 129, slab 64, weighted, repeats"


def case_names():
    """the names of cases(), without building any data (for pytest's parametrisation)"""
    return [row[0] for row in _TABLE]


_CASES = None


def cases():
    """name -> dict(W, atoms, data = (states, targets, weights), idx (array or None), n, batch (= n), slab, weighted, tstride);
    built once, at the first use"""
    global _CASES
    if _CASES is not None:
        return _CASES
    N = DC.nets()
    rng = np.random.default_rng(41)
    data, out = {}, {}
    for name, net, n, slab, weighted, idx, tstride, normalised in _TABLE:
        a, W = N[net]
        if (net, normalised) not in data:
            data[net, normalised] = DC._restrict(net, DC.dataset(DC.CANDIDATES, a, 7, normalised=normalised), W)
        d = data[net, normalised]
        m = len(d[0])
        assert n <= m
        if isinstance(idx, str):
            idx = rng.integers(0, 40 if idx == "repeats" else m, n)
        out[name] = dict(W=W, atoms=a, data=d, idx=idx, n=n, batch=n, slab=slab, weighted=weighted, tstride=tstride or a)
    _CASES = out
    return out


def rows_of(case):
    return np.arange(case["n"]) if case["idx"] is None else np.asarray(case["idx"])


def reference(case, dtype):
    """[8 arrays, float64]: sum over the case's rows of (gradient of that row's loss)^2 / n, one backward per row, the squares and
    the sum in `dtype`"""
    from tetris_mcts_amd.model_distributional import PARAM_ORDER, Model_Dist
    (states, target, weight), weighted, n = case["data"], case["weighted"], case["n"]
    mdl = Model_Dist.__new__(Model_Dist)
    mdl.model = DC.make_net(case["W"]).to(dtype).train()
    named = dict(mdl.model.named_parameters())
    params = [named[k] for k in PARAM_ORDER]
    acc = [torch.zeros_like(p) for p in params]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (std_mean of one row: the standard deviation is not used)
        for r in rows_of(case):
            x = HN.dn_input(states[r:r + 1]).to(dtype)
            t = torch.from_numpy(target[r:r + 1].astype(np.float64)).to(dtype)
            w = torch.from_numpy(weight[r:r + 1].astype(np.float64)).to(dtype).reshape(-1, 1)
            for p in params:
                p.grad = None
            mean, _ = mdl.loss(x, t, w if weighted else None)
            mean.backward()
            with torch.no_grad():
                for a, p in zip(acc, params):
                    a += p.grad * p.grad / n
    return [a.detach().double().numpy().reshape(-1).copy() for a in acc]


_REF = {}


def references(name, case):
    """(F64, F32) of a case, computed once per session and left unchanged"""
    if name not in _REF:
        torch.set_num_threads(16)
        _REF[name] = (reference(case, torch.float64), reference(case, torch.float32))
    return _REF[name]


# ---- the device side (imported lazily: the CPU tests use the references alone) ----
def fisher_inputs(case, device="cuda", packed=False):
    """the device tensors a call reads, as a dict (idx: None when the case passes NULL); the targets' padding is NaN"""
    (states, target, weight), idx, atoms, stride = case["data"], case["idx"], case["atoms"], case["tstride"]
    dev = torch.device(device)
    P = torch.from_numpy(HN.dn_flat(case["W"])).to(dev).contiguous()
    assert P.numel() == DC.n_params(atoms) and stride >= atoms
    if packed:
        import fit_packed_cases as PK
        obs = PK.pack(states)
        assert (PK.render(obs) == np.asarray(states, np.int8)).all()
        s = torch.from_numpy(np.ascontiguousarray(obs)).to(dev)
    else:
        s = torch.from_numpy(np.ascontiguousarray(states, dtype=np.int8)).to(dev)
    tp = np.full((len(target), stride), np.nan, np.float32)
    tp[:, :atoms] = target
    t, w = torch.from_numpy(tp).to(dev), torch.from_numpy(np.ascontiguousarray(weight, dtype=np.float32)).to(dev)
    if idx is not None:
        assert len(idx) == case["n"] and 0 <= int(np.min(idx)) and int(np.max(idx)) < len(states)
        idx_t = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev)
    else:
        assert case["n"] <= len(states)
        idx_t = None
    return dict(params=P, states=s, targets=t, weight=w, idx=idx_t)


def hip_fisher(case, device="cuda", fill=None, place=None, packed=False, slab=None):
    """one tm_distnet_fit_fisher (or _packed) call for a case: the Fisher as a float32 array [279232 + 129 atoms].  `place`: as
    dist_fit_cases.hip_grad's (fit_hip_cases.Arena: the workspace of exactly the stated floats, the Fisher, and two spare floats)."""
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    dev = torch.device(device)
    inp = fisher_inputs(case, device, packed)
    atoms, np_ = case["atoms"], DC.n_params(case["atoms"])
    slab = case["slab"] if slab is None else slab
    n_ws = lib.tm_distnet_fit_fisher_workspace(slab, atoms)
    assert n_ws > 0
    if place is None:
        ws, fisher = (torch.empty(n, dtype=torch.float32, device=dev) for n in (n_ws, np_))
    else:
        ws, fisher, _ = place(n_ws, np_, inp)
        assert (ws.numel(), fisher.numel()) == (n_ws, np_)
    ws.fill_(float("nan"))                                                         # no initial contents required
    fisher.fill_(float("nan") if fill is None else fill)
    fn = lib.tm_distnet_fit_fisher_packed if packed else lib.tm_distnet_fit_fisher
    idx_t = inp["idx"]
    _lib.check(fn(inp["params"].data_ptr(), inp["states"].data_ptr(), inp["targets"].data_ptr(), case["tstride"], inp["weight"].data_ptr(),
                  idx_t.data_ptr() if idx_t is not None else None, case["n"], slab, atoms, int(case["weighted"]), fisher.data_ptr(),
                  ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "tm_distnet_fit_fisher")
    torch.cuda.synchronize()
    return fisher.cpu().numpy()


def digest_case():
    return cases()[N33]


if __name__ == "__main__":
    if sys.argv[1:] == ["digest"]:
        import hashlib
        print("DIGEST " + hashlib.sha256(hip_fisher(digest_case()).tobytes()).hexdigest(), flush=True)
