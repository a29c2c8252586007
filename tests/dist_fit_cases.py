"""Cases and references for the HIP gradient step of the distributional head's fit (csrc/distnet_fit.hip), shared by
tests/test_dist_fit_hip.py (CPU: the references alone - that the yardstick's denominators are non-zero, that the kink filter
keeps its cap) and tests/test_gpu_dist_fit_hip.py (GPU: the kernels against them).

The reference's arithmetic is torch autograd of model_distributional.Net.log_prob + Model_Dist.loss on the CPU, in fp64 (g64) and
in fp32 (g32).  The yardstick is measure B of DESIGN.md section 6 applied to gradients, per parameter tensor and for the two loss
outputs (tests/fit_hip_cases.py `measure`):
    max|g_hip - g64| <= M max|g32 - g64| + 4 u max|g64|,   M = 8, u = 2^-24.
A tensor whose fp64 gradient is identically zero (every tensor at atoms = 1: log p = 0) is compared for exact zeros instead.

Run as a program (`python tests/dist_fit_cases.py digest`) it prints the SHA-256 of one case's gradient and loss bytes: the
second process of the determinism test."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import fit_hip_cases as FC  # noqa: E402  (boards, measure, U: the value net's cases)
import heads_numerics as HN  # noqa: E402

U, M_CAP, measure = FC.U, FC.M_CAP, FC.measure
# the blocking constants of csrc/distnet_fit.hip along the batch, and the batches around each of them
SPW = 4             # samples per wave of the convolutions' weight-gradient partials
TILE = 32           # the matrix core's tile (fc1 forward and data gradient: 32 samples a wave), HEAD_CHUNK (samples per partial of the
                    # FC bias sums) and the 32-sample chunks of the FC weight gradients' K
FC_KC = 256         # samples per split of the FC weight gradients; also the threads of the loss kernel's strided sum
RED_G = 16          # k_fit_reduce<16> adds its S partials in 16 interleaved groups: S = B (the convolutions' bias sums) passes 16
                    # at B = 16, S = ceil(B / SPW) (their weight gradients) at B = 64, S = ceil(B / TILE) (the FC bias sums) at
                    # B = 512 (LARGE_BATCHES: 480 / 512 / 513)
RED_G_FC = 4        # k_fit_reduce<4> adds the s1 = ceil(B / FC_KC) splits of the two FC weight gradients in 4 groups: s1 passes
                    # 4 at B = 1 025 (LARGE_BATCHES: 1 000 / 1 024 / 1 025; 1 024 is the batch every DistValueSim fit uses)
# (k_df_head's four samples a workgroup is SPW's 3 / 4 / 5 again)
BATCHES = (1, 2, SPW - 1, SPW, SPW + 1, RED_G - 1, RED_G, RED_G + 1, TILE - 1, TILE, TILE + 1, RED_G * SPW - SPW, RED_G * SPW,
           RED_G * SPW + 1, FC_KC - 1, FC_KC, FC_KC + 1)
# past the candidate rows of the cases above: hchunks = ceil(B / TILE) at 15 / 16 / 17, and s1 at 3 (with a split of one sample),
# at 4 (with a ragged last split of 232 = 7 K chunks and 8 samples; and full) and at 5 (the last split of one sample)
LARGE_BATCHES = (RED_G * TILE - TILE, RED_G * TILE, RED_G * TILE + 1, 1000, RED_G_FC * FC_KC, RED_G_FC * FC_KC + 1)
KINK_CAP = 0.25     # the filter may drop at most this share of the candidate rows
CANDIDATES = 420
LARGE_CANDIDATES = 1400                                    # a second candidate set for the nets of the large batches
LARGE_NETS = ("fixture", "seed7", "seed64", "fitted")
LARGE_SETS = tuple("%s, %d rows" % (k, LARGE_CANDIDATES) for k in LARGE_NETS)          # their names in KINK_KEPT


def n_params(atoms):
    return 279232 + 129 * atoms


def sizes(atoms):
    return (512, 32, 16384, 32, 262144, 128, 128 * atoms, atoms)


TENSORS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias", "fc_v.weight", "fc_v.bias")


def split(flat, atoms):
    out, off = [], 0
    for n in sizes(atoms):
        out.append(np.asarray(flat[off:off + n], dtype=np.float64))
        off += n
    assert off == n_params(atoms) == len(flat)
    return out


def make_net(W):
    """model_distributional.Net holding the eight arrays W (PARAM_ORDER)"""
    from tetris_mcts_amd.model_distributional import Net, PARAM_ORDER
    net = Net(atoms=int(W[6].shape[0]))
    sd = net.state_dict()
    for k, w in zip(PARAM_ORDER, W):
        sd[k].copy_(torch.from_numpy(np.asarray(w, np.float32)).reshape(sd[k].shape))
    return net


def targets(n, atoms, seed, normalised=True):
    """[n, atoms] fp32 >= 0: a bump at a random place plus noise; the three lowest bins of every second row are exactly zero (the
    search's shifted distributions); rows sum to 1, or (normalised=False) to a factor in [0.3, 1.7]"""
    rng = np.random.default_rng(seed + 2000)
    c = rng.uniform(0, atoms, (n, 1))
    a = np.arange(atoms).reshape(1, -1)
    t = np.exp(-0.5 * ((a - c) / max(1.0, atoms / 10.0)) ** 2) + 0.02 * rng.random((n, atoms))
    t[::2, :min(3, atoms - 1)] = 0.0
    t /= t.sum(1, keepdims=True)
    if not normalised:
        t *= rng.uniform(0.3, 1.7, (n, 1))
    return t.astype(np.float32)


def dataset(n, atoms, seed, normalised=True):
    """(states int8 [n,200], targets fp32 [n,atoms], weights fp32 [n])"""
    rng = np.random.default_rng(seed + 1000)
    s, _ = FC.boards(n, seed)
    w = rng.integers(3, 50, n).astype(np.float32)
    w /= w.mean()
    return s, targets(n, atoms, seed, normalised), w


def off_the_kink(W, states):
    """Rows whose every LeakyReLU pre-activation z keeps clear of zero, where the slope jumps from 0.01 to 1:
    |z| >= 64 u (|bias| + sum_k |w_k a_k|), from an fp64 forward of conv1, conv2 and fc1 (fit_hip_cases.off_the_kink has the
    reasoning: K <= 2 048 here, sqrt(K) <= 46 < 64)."""
    import torch.nn.functional as F
    x = HN.dn_input(states).double()
    keep = torch.ones(x.shape[0], dtype=torch.bool)
    with torch.no_grad():
        for L in HN.dn_layers(W)[:3]:
            w, b = L.tensors(torch.float64)
            z = HN.lin(L, x, w, b)
            S = HN.lin(L, x.abs(), w.abs(), b.abs())
            keep &= (z.abs() >= 64 * U * S).flatten(1).all(1)
            x = F.leaky_relu(z, 0.01)
    return keep.numpy()


KINK_KEPT = {}      # candidate set (a net's name, or one of LARGE_SETS) -> share of its rows the filter kept
                    # (tests/test_dist_fit_hip.py asserts the cap)


def candidates(name):
    return LARGE_CANDIDATES if name in LARGE_SETS else CANDIDATES


def _restrict(name, data, W):
    keep = off_the_kink(W, data[0])
    KINK_KEPT[name] = float(keep.mean())
    assert keep.mean() >= 1.0 - KINK_CAP, (name, keep.mean())
    return tuple(a[keep] for a in data)


def nets():
    """name -> (atoms, [8 arrays]): the fixture net, seeded nets at the ends and around the 16-atom tile, a peaked net (logit
    spread 50) and the fitted net of tests/golden/ref_heads_trained.npz"""
    r = {"fixture": (50, HN.fixture_dist_net())}
    for a in (1, 7, 16, 17, 50, 64):
        r["seed%d" % a] = (a, HN.seeded_dist_net(a))
    r["peaked50_50"] = (50, HN.peaked(HN.seeded_dist_net(50), 50))
    r["fitted"] = (50, HN.fitted_dist_net())
    return r


_CASES = {}


def cases(full=True):
    """name -> dict(W, atoms, data = (states, targets, weights), idx (array or None), batch, weighted, tstride); built once, at
    the first use (not at collection: a run that deselects the GPU tests pays nothing)"""
    if full not in _CASES:
        _CASES[full] = _build_cases(full)
    return _CASES[full]


def case_names(full=True):
    """the names of cases(full), without building any data (for pytest's parametrisation)"""
    return list(_build_cases(full, names_only=True))


def large_cases(names_only=False):
    """the regimes past BATCHES, on candidate sets of LARGE_CANDIDATES rows (same dataset / off_the_kink rule, same cap); their
    indices come from a generator of their own.  Built once; names_only builds no data."""
    if names_only:
        return _build_large(None, True)
    if "large" not in _CASES:
        _CASES["large"] = _build_large(nets(), False)
    return _CASES["large"]


def _build_large(N, names_only):
    out = {}
    rng = np.random.default_rng(12)
    data = {} if names_only else {k: _restrict(s, dataset(LARGE_CANDIDATES, N[k][0], 7), N[k][1]) for k, s in zip(LARGE_NETS, LARGE_SETS)}

    def add(name, net, batch, weighted=True, idx="random", tstride=None):
        if names_only:
            out[name] = None
            return
        a, W = N[net]
        d = data[net]
        n = len(d[0])
        assert batch <= n
        ix = rng.integers(0, n, batch) if isinstance(idx, str) else idx
        out[name] = dict(W=W, atoms=a, data=d, idx=ix, batch=batch, weighted=weighted, tstride=tstride or a)

    for b in LARGE_BATCHES:
        add("fixture, batch %d" % b, "fixture", b)
    b3 = RED_G * TILE + 1                                     # s1 = 3: fc_v's partial stride (64 x 128) against atoms x 128 outputs
    add("seed7, batch %d, stride 64" % b3, "seed7", b3, tstride=64)
    add("seed64, batch %d" % b3, "seed64", b3)
    add("fitted, batch %d, unweighted, idx NULL" % (RED_G_FC * FC_KC), "fitted", RED_G_FC * FC_KC, weighted=False, idx=None)
    return out


def _build_cases(full, names_only=False):
    out, N = {}, nets()
    rng = np.random.default_rng(11)
    data = {} if names_only else {k: _restrict(k, dataset(CANDIDATES, a, 7), W) for k, (a, W) in N.items()}

    def add(name, net, batch, weighted=True, idx="random", tstride=None, d=None):
        if names_only:
            out[name] = None
            return
        a, W = N[net]
        d = data[net] if d is None else d() if callable(d) else d
        n = len(d[0])
        ix = rng.integers(0, n, batch) if isinstance(idx, str) else idx
        assert batch <= n
        out[name] = dict(W=W, atoms=a, data=d, idx=ix, batch=batch, weighted=weighted, tstride=tstride or a)

    for b in (BATCHES if full else (1, 2, SPW + 1, TILE + 1)):
        add("fixture, batch %d" % b, "fixture", b)
    add("fixture, unweighted, idx NULL", "fixture", 256 if full else 40, weighted=False, idx=None)
    add("fixture, weighted, idx NULL, stride 64", "fixture", 100 if full else 34, idx=None, tstride=64)
    add("fixture, unweighted, repeats", "fixture", 256 if full else 48, weighted=False, idx=rng.integers(0, 40, 256 if full else 48))
    for a in (1, 7, 16, 17, 50, 64):
        add("seed%d, batch 33, stride %d" % (a, 64 if a % 2 else a), "seed%d" % a, 33, tstride=64 if a % 2 else a)
    add("seed64, batch 65, unweighted", "seed64", 65, weighted=False)
    for weighted in (True, False):
        add("peaked50_50, batch 65, %s" % ("weighted" if weighted else "unweighted"), "peaked50_50", 65, weighted=weighted)
    add("fitted, batch 65", "fitted", 65)
    if full:
        add("fitted, batch 256, unweighted, stride 64", "fitted", 256, weighted=False, tstride=64)
    # targets that do not sum to 1 (the search's distributions are not renormalised): the factor sum_a t stays in the gradient
    add("fixture, targets off 1, batch 65", "fixture", 65,
        d=lambda: _restrict("fixture", dataset(CANDIDATES, 50, 7, normalised=False), N["fixture"][1]))
    add("fitted, targets off 1, batch 33, unweighted", "fitted", 33, weighted=False,
        d=lambda: _restrict("fitted", dataset(CANDIDATES, 50, 7, normalised=False), N["fitted"][1]))
    if full:          # last, with candidate rows and a generator of their own: every case above keeps its rows and its index draw
        large = large_cases(names_only)
        assert not set(large) & set(out)
        out.update(large)
    return out


_REF = {}


def reference(name, case, dtype):
    """autograd of Net.log_prob + Model_Dist.loss on the CPU in `dtype`: ([8 gradients as float64 arrays], (mean, std));
    computed once per (case, dtype) and shared"""
    key = (name, dtype)
    if key not in _REF:
        from tetris_mcts_amd.model_distributional import Model_Dist
        (states, target, weight), weighted = case["data"], case["weighted"]
        mdl = Model_Dist.__new__(Model_Dist)
        mdl.model = make_net(case["W"]).to(dtype).train()
        idx = np.arange(case["batch"]) if case["idx"] is None else np.asarray(case["idx"])
        x = HN.dn_input(states[idx]).to(dtype)
        t = torch.from_numpy(target[idx].astype(np.float64)).to(dtype)
        w = torch.from_numpy(weight[idx].astype(np.float64)).to(dtype).reshape(-1, 1)
        mean, std = mdl.loss(x, t, w if weighted else None)
        mean.backward()
        named = dict(mdl.model.named_parameters())
        from tetris_mcts_amd.model_distributional import PARAM_ORDER
        grads = [named[k].grad.detach().double().numpy().copy() for k in PARAM_ORDER]
        _REF[key] = (grads, (float(mean.detach().double()), float(std.detach().double())))
    return _REF[key]


# ---- the device side (imported lazily: the CPU tests use the references alone) ----
def hip_grad(case, device="cuda", grad_fill=None, place=None):
    """one tm_distnet_fit_grad call for a case: (flat gradient float32 array, loss [2] float32 array).  The targets' padding
    (target_stride > atoms), the workspace and the outputs start as NaN: nothing of them may be read.

    `place(n_workspace, n_grad, inputs)` may supply the three buffers the call writes, as float32 views (workspace, grad, loss)
    of storage of its own (fit_hip_cases.Arena: guard bands around each); `inputs` is the dict of the device tensors the call
    reads, handed over before the launch.  The buffers are filled as without `place`.  A read past an input cannot be seen
    this way (a stray read changes nothing); stray stores within 64 KiB of a buffer and stores into an input can."""
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    (states, target, weight), idx, B, atoms, stride = case["data"], case["idx"], case["batch"], case["atoms"], case["tstride"]
    dev = torch.device(device)
    P = torch.from_numpy(HN.dn_flat(case["W"])).to(dev).contiguous()
    assert P.numel() == n_params(atoms) and stride >= atoms
    s8 = torch.from_numpy(np.ascontiguousarray(states, dtype=np.int8)).to(dev)
    tp = np.full((len(target), stride), np.nan, np.float32)
    tp[:, :atoms] = target
    t, w = torch.from_numpy(tp).to(dev), torch.from_numpy(np.ascontiguousarray(weight, dtype=np.float32)).to(dev)
    if idx is not None:
        assert len(idx) == B and 0 <= int(np.min(idx)) and int(np.max(idx)) < len(states)
        idx_t = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev)
    else:
        assert B <= len(states)
        idx_t = None
    n_ws = lib.tm_distnet_fit_workspace(B, atoms)
    assert n_ws > 0
    if place is None:
        ws, grad, loss = (torch.empty(n, dtype=torch.float32, device=dev) for n in (n_ws, n_params(atoms), 2))
    else:
        ws, grad, loss = place(n_ws, n_params(atoms), dict(params=P, states=s8, targets=t, weight=w, idx=idx_t))
        assert (ws.numel(), grad.numel(), loss.numel()) == (n_ws, n_params(atoms), 2) and all(b.dtype == torch.float32 for b in (ws, grad, loss))
    ws.fill_(float("nan"))
    grad.fill_(float("nan") if grad_fill is None else grad_fill)
    loss.fill_(float("nan"))
    _lib.check(lib.tm_distnet_fit_grad(P.data_ptr(), s8.data_ptr(), t.data_ptr(), stride, w.data_ptr(),
                                       idx_t.data_ptr() if idx_t is not None else None, B, atoms, int(case["weighted"]),
                                       grad.data_ptr(), loss.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               "tm_distnet_fit_grad")
    torch.cuda.synchronize()
    return grad.cpu().numpy(), loss.cpu().numpy()


DIGEST_CASE = "fixture, batch 33"


def digest_case():
    return cases(full=False)[DIGEST_CASE]


if __name__ == "__main__":
    if sys.argv[1:] == ["digest"]:
        import hashlib
        g, l = hip_grad(digest_case())
        print("DIGEST " + hashlib.sha256(g.tobytes() + l.tobytes()).hexdigest(), flush=True)
