"""Cases and references for the Fisher pass of the value net's fit (csrc/valuenet_fit.hip: tm_valuenet_fit_fisher) and for the
penalty of elastic weight consolidation (csrc/yogi.hip: tm_ewc_penalty), shared by tests/test_fisher.py (CPU: the references
alone) and tests/test_gpu_fisher.py (GPU: the kernels against them).

The reference is per-sample CPU autograd of model.Net + train.batch_loss on ONE row at a time, g^2 / n accumulated in the dtype,
in fp64 (F64) and in fp32 (F32: the arithmetic of the reference project's own loop, model_vv.py:188-208).  The yardstick is
measure B of DESIGN.md section 6, as for gradients (fit_hip_cases.measure), per parameter tensor:
    max|F_hip - F64| <= 8 max|F32 - F64| + 4 u max|F64|,   u = 2^-24.
A tensor whose F64 is identically zero is compared for exact zeros instead.  All rows keep clear of the ReLU kinks
(fit_hip_cases.off_the_kink, computed from the reference alone).

The shapes are the smallest at which each blocking constant of the pass can go wrong: SPW = 4 samples per partial of the
convolutions, HEAD_CHUNK = 32 samples per partial of the small sums, FC1_KC = 256 samples per split of fc1, and the slab.

Run as a program (`python tests/fisher_cases.py digest`) it prints the SHA-256 of one case's Fisher: the second process of the
determinism test."""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import fit_hip_cases as FC  # noqa: E402

N_LEARN = FC.N_LEARN
FISHER_EXTRA = 478340 + 956676      # the temporary [478338] rounded up to four floats, the accumulator [478338] doubles
CLIP = 0.1


def _fresh_rows():
    data = FC._restrict(FC.dataset(400, 7), FC.fresh_net(0))
    assert len(data[0]) >= 257
    return data


_CASES = None


def cases():
    """name -> dict(net, data = (states, value, variance, weight), idx (array or None), n, batch (= n), slab, weighted)"""
    global _CASES
    if _CASES is not None:
        return _CASES
    data = _fresh_rows()
    m = len(data[0])
    rng = np.random.default_rng(31)
    out = {}

    def add(name, n, slab, weighted, idx, net=None, rows=None):
        out[name] = dict(net=net or FC.fresh_net(0), data=rows or data, idx=idx, n=n, batch=n, slab=slab, weighted=weighted)
    add("n 1, weighted, idx", 1, 1024, True, rng.integers(0, m, 1))
    add("n 3, unweighted, idx NULL", 3, 1024, False, None)
    add("n 5, weighted, repeats", 5, 1024, True, np.array([7, 2, 7, 7, 2]))
    add("n 33, weighted, idx NULL", 33, 1024, True, None)
    add("n 257, unweighted, idx", 257, 1024, False, rng.integers(0, m, 257))
    add("n 129, slab 64, weighted, repeats", 129, 64, True, rng.integers(0, 40, 129))
    add("n 70, slab 32, unweighted, idx NULL", 70, 32, False, None)
    ck = "value_net_online_r06.pt"
    big = FC.dataset(160, 21, scale=40.0)
    big = FC._restrict(big, FC.net_from_checkpoint(ck, big[1], big[2]))
    add("%s, x40 targets, n 64" % ck, 64, 1024, True, rng.integers(0, len(big[0]), 64), net=FC.net_from_checkpoint(ck, big[1], big[2]),
        rows=big)
    _CASES = out
    return out


def dead_case():
    """fit_hip_cases.dead_relu_case's net (a3 = 0 everywhere), 16 of its rows: the Fishers of conv1, conv2, conv3 and fc1.weight
    are exactly 0"""
    c = FC.dead_relu_case()
    return dict(net=c["net"], data=c["data"], idx=np.asarray(c["idx"][:16]), n=16, batch=16, slab=1024, weighted=True)


def rows_of(case):
    return np.arange(case["n"]) if case["idx"] is None else np.asarray(case["idx"])


def reference(case, dtype):
    """[10 arrays, float64]: sum over the case's rows of (gradient of that row's loss)^2 / n, one backward per row, the squares
    and the sum in `dtype`"""
    from tetris_mcts_amd import train as T
    (states, value, variance, weight), weighted, n = case["data"], case["weighted"], case["n"]
    net = copy.deepcopy(case["net"]).to(dtype).train()
    params = FC.learnable(net)
    acc = [torch.zeros_like(p) for p in params]
    for r in rows_of(case):
        batch = [torch.from_numpy(states[r:r + 1].reshape(1, 1, 20, 10).astype(np.float64)).to(dtype)] + \
                [torch.from_numpy(a[r:r + 1].reshape(1, 1).astype(np.float64)).to(dtype) for a in (value, variance, weight)]
        for p in net.parameters():
            p.grad = None
        mean, _ = T.batch_loss(net, batch, weighted, variance_clip=CLIP)
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


def penalty_numpy(p, anchor, fisher, grad, lam):
    """The float32 statement of tm_ewc_penalty: (the gradient after the call, the loss in fp64).  Per element, in float, in this
    order: d = p - anchor, t = ((float)lam F) d, grad = grad + t; loss = 0.5 lam sum F d d in double, F and the float d converted
    first."""
    p, anchor, fisher, grad = (np.asarray(a, np.float32) for a in (p, anchor, fisher, grad))
    d = (p - anchor).astype(np.float32)
    t = ((np.float32(lam) * fisher).astype(np.float32) * d).astype(np.float32)
    out = (grad + t).astype(np.float32)
    d64 = d.astype(np.float64)
    return out, 0.5 * float(lam) * float(np.sum(fisher.astype(np.float64) * d64 * d64))


def penalty_case(n, seed, zero_fisher=False, at_anchor=False):
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 0.05, n).astype(np.float32)
    anchor = p.copy() if at_anchor else (p + rng.normal(0, 0.01, n)).astype(np.float32)
    fisher = np.zeros(n, np.float32) if zero_fisher else (rng.random(n) ** 4 * 30).astype(np.float32)
    grad = rng.normal(0, 0.1, n).astype(np.float32)
    grad[::7] = np.float32(-0.0)
    return p, anchor, fisher, grad


# ---- the device side (imported lazily: the CPU tests use the references alone) ----
def fisher_inputs(case, device="cuda", packed=False):
    """the device tensors a call reads, as a dict (idx: None when the case passes NULL)"""
    net, (states, value, variance, weight), idx = case["net"], case["data"], case["idx"]
    dev = torch.device(device)
    P = torch.cat([p.detach().reshape(-1).float() for p in FC.learnable(net)]).to(dev).contiguous()
    assert P.numel() == N_LEARN
    bounds = torch.cat([net.out_ubound.detach(), net.out_lbound.detach()]).float().to(dev).contiguous()
    if packed:
        import fit_packed_cases as PK
        obs = PK.pack(states)
        assert (PK.render(obs) == np.asarray(states, np.int8)).all()
        s = torch.from_numpy(np.ascontiguousarray(obs)).to(dev)
    else:
        s = torch.from_numpy(np.ascontiguousarray(states, dtype=np.int8)).to(dev)
    val, var, w = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (value, variance, weight))
    if idx is not None:
        assert len(idx) == case["n"] and 0 <= int(np.min(idx)) and int(np.max(idx)) < len(states)
        idx_t = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev)
    else:
        assert case["n"] <= len(states)
        idx_t = None
    return dict(params=P, bounds=bounds, states=s, value=val, variance=var, weight=w, idx=idx_t)


def hip_fisher(case, device="cuda", fill=None, place=None, packed=False, slab=None):
    """one tm_valuenet_fit_fisher (or _packed) call for a case: the Fisher as a float32 array [478338].  `place`: as
    fit_hip_cases.hip_grad's (an Arena: the workspace of exactly the stated floats, the Fisher, and two spare floats)."""
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    dev = torch.device(device)
    inp = fisher_inputs(case, device, packed)
    slab = case["slab"] if slab is None else slab
    n_ws = lib.tm_valuenet_fit_fisher_workspace(slab)
    assert n_ws > 0
    if place is None:
        ws, fisher = (torch.empty(n, dtype=torch.float32, device=dev) for n in (n_ws, N_LEARN))
    else:
        ws, fisher, _ = place(n_ws, N_LEARN, inp)
        assert (ws.numel(), fisher.numel()) == (n_ws, N_LEARN)
    ws.fill_(float("nan"))                                                         # no initial contents required
    fisher.fill_(float("nan") if fill is None else fill)
    fn = lib.tm_valuenet_fit_fisher_packed if packed else lib.tm_valuenet_fit_fisher
    idx_t = inp["idx"]
    _lib.check(fn(inp["params"].data_ptr(), inp["bounds"].data_ptr(), inp["states"].data_ptr(), inp["value"].data_ptr(),
                  inp["variance"].data_ptr(), inp["weight"].data_ptr(), idx_t.data_ptr() if idx_t is not None else None, case["n"], slab,
                  int(case["weighted"]), CLIP, fisher.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               "tm_valuenet_fit_fisher")
    torch.cuda.synchronize()
    return fisher.cpu().numpy()


def hip_penalty(p, anchor, fisher, grad, lam, device="cuda", place=None):
    """one tm_ewc_penalty call: (the gradient after it, float32 array; the loss, a Python float)"""
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    dev, n = torch.device(device), len(p)
    P, A, F = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (p, anchor, fisher))
    n_ws = lib.tm_ewc_penalty_workspace(n)
    assert n_ws >= 2 * ((n + 255) // 256) and n_ws % 4 == 0
    if place is None:
        ws, g, loss = (torch.empty(k, dtype=torch.float32, device=dev) for k in (n_ws, n, 2))
    else:
        ws, g, loss = place(n_ws, n, dict(p=P, anchor=A, fisher=F))
    ws.fill_(float("nan"))
    loss.fill_(float("nan"))
    g.copy_(torch.from_numpy(np.ascontiguousarray(grad, dtype=np.float32)))
    _lib.check(lib.tm_ewc_penalty(P.data_ptr(), A.data_ptr(), F.data_ptr(), n, float(lam), g.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream), "tm_ewc_penalty")
    torch.cuda.synchronize()
    return g.cpu().numpy(), float(loss.view(torch.float64).cpu()[0])


def digest_case():
    return cases()["n 33, weighted, idx NULL"]


if __name__ == "__main__":
    if sys.argv[1:] == ["digest"]:
        import hashlib
        print("DIGEST " + hashlib.sha256(hip_fisher(digest_case()).tobytes()).hexdigest(), flush=True)
