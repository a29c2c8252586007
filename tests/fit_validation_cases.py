"""Cases and references for the HIP validation pass of the fits (tm_valuenet_fit_validate in csrc/valuenet_fit.hip,
tm_distnet_fit_validate in csrc/distnet_fit.hip), shared by tests/test_fit_validation.py (CPU: the references alone) and
tests/test_gpu_fit_validation.py (GPU: the kernels against them).

A case is a regime (a net, rows, weighted or not) at one of ROWS row counts, validated in chunks of CHUNK rows, SLAB rows
forwarded at a time:
    33   a ragged last chunk of one row
    97   a slab of two chunks, then a ragged slab (one chunk and one row)
    161  three slabs, the last one a single row
The reference is what train.validation_loss does on the CPU, in fp64 and in fp32: train.batch_loss / train.dist_batch_loss per
chunk (torch.std_mean: the population std for the value net, the n - 1 std for the head, NaN for a chunk of one row), the
chunk's weight, and train.combine_chunk_rows over the chunks.  The yardstick is measure B of DESIGN.md section 6
(fit_hip_cases.measure) on the vector of the chunks' means, on the vector of their stds, on their weights and on the combined
(mean, std):
    max|hip - f64| <= 8 max|torch32 - f64| + 4 u max|f64|.
Exact cases are compared exactly, not by the rule: seed1 (one atom: every loss is 0) and the std of a one-row chunk (0 for the
value net, NaN for the head)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import dist_fit_cases as DC  # noqa: E402
import fit_hip_cases as FC  # noqa: E402
import heads_numerics as HN  # noqa: E402

measure, U = FC.measure, FC.U
ROWS, CHUNK, SLAB = (33, 97, 161), 32, 64
N_MAX = max(ROWS)
CLIP = 0.1          # train.variance_bound, as fit_hip_cases.hip_grad passes it

VALUE_REGIMES = ("fresh net, weighted", "fresh net, unweighted", "r05 checkpoint, scale 40", "r06 checkpoint, scale 40",
                 "targets below the variance clip", "saturated sigmoids")
DIST_REGIMES = ("fixture", "seed1", "seed7, targets off 1, stride 64", "seed64, unweighted", "fitted")
EXACT_ZERO = ("seed1",)          # one atom: log p = 0 and t log t = 0 at t = 1, every per-sample loss is exactly 0

_CACHE = {}


def value_regime(name):
    """dict(net, data = (states int8 [161,200], value, variance, weight), weighted)"""
    key = ("value", name)
    if key not in _CACHE:
        weighted = name != "fresh net, unweighted"
        if "checkpoint" in name:
            data = FC.dataset(N_MAX, 21, scale=40.0)
            net = FC.net_from_checkpoint("value_net_online_%s.pt" % name[:3], data[1], data[2])
        else:
            data = FC.dataset(N_MAX, 7)
            net = FC.fresh_net(0)
            if name == "targets below the variance clip":
                data = tuple(a.copy() for a in data)
                data[2][:] = np.float32(0.003)
            if name == "saturated sigmoids":
                with torch.no_grad():
                    net.head.fc_out.bias.copy_(torch.tensor([12.0, -12.0]))
        _CACHE[key] = dict(head="value", net=net, data=data, weighted=weighted)
    return _CACHE[key]


def dist_regime(name):
    """dict(W, atoms, data = (states int8 [161,200], targets [161,atoms], weights), weighted, tstride)"""
    key = ("dist", name)
    if key not in _CACHE:
        atoms, W = DC.nets()[name.split(",")[0]]
        data = DC.dataset(N_MAX, atoms, 7, normalised="targets off 1" not in name)
        _CACHE[key] = dict(head="dist", W=W, atoms=atoms, data=data, weighted="unweighted" not in name,
                           tstride=64 if "stride 64" in name else atoms)
    return _CACHE[key]


def regime(head, name):
    return value_regime(name) if head == "value" else dist_regime(name)


ALL = [("value", r) for r in VALUE_REGIMES] + [("dist", r) for r in DIST_REGIMES]


def torch_batches(case, n, dtype):
    """(net in dtype, the first n rows as train_data's tensors in dtype, loss_fn)"""
    import copy
    from tetris_mcts_amd import train as T
    d = case["data"]
    f = lambda a, shape: torch.from_numpy(np.asarray(a[:n], np.float64).reshape(shape)).to(dtype)      # noqa: E731
    if case["head"] == "value":
        net = copy.deepcopy(case["net"]).to(dtype)
        return net, [f(d[0], (-1, 1, 20, 10)), f(d[1], (-1, 1)), f(d[2], (-1, 1)), f(d[3], (-1, 1))], T.batch_loss
    net = DC.make_net(case["W"]).to(dtype)
    return net, [HN.dn_input(d[0][:n]).to(dtype), f(d[1], (n, -1)), f(d[2], (-1, 1))], T.dist_batch_loss


_REF = {}


def reference(head, name, n, dtype, chunk=CHUNK):
    """(rows [ceil(n / chunk), 3] float64 = the chunks' {w, mean, std} as train.validation_loss collects them on the CPU in
    `dtype`, (mean, std) of train.combine_chunk_rows over them); computed once and shared"""
    key = (head, name, n, dtype, chunk)
    if key not in _REF:
        from tetris_mcts_amd import train as T
        case = regime(head, name)
        net, data, loss_fn = torch_batches(case, n, dtype)
        rows = []
        with torch.no_grad():
            for c in range(0, n, chunk):
                b = [t[c:c + chunk] for t in data]
                mean, std = loss_fn(net, b, case["weighted"])
                w = float(b[-1].sum().double()) if case["weighted"] else float(b[0].shape[0])
                rows.append([w, float(mean.double()), float(std.double())])
        _REF[key] = (np.asarray(rows, np.float64), T.combine_chunk_rows(rows))
    return _REF[key]


def one_row_chunks(n, chunk=CHUNK):
    """mask over the chunks of n rows: True where the chunk holds exactly one row"""
    counts = np.asarray([min(chunk, n - c) for c in range(0, n, chunk)])
    return counts == 1


def compare(head, name, n, got_rows, chunk=CHUNK, log=print):
    """hold `got_rows` ([chunks, 3] float64 from the device) to the rule; returns (failures, the largest multiple needed)"""
    from tetris_mcts_amd import train as T
    r64, c64 = reference(head, name, n, torch.float64, chunk)
    r32, c32 = reference(head, name, n, torch.float32, chunk)
    got_rows = np.asarray(got_rows, np.float64)
    assert got_rows.shape == r64.shape
    single = one_row_chunks(n, chunk)
    bad, worst = [], 0.0
    # the exact part: the std of a one-row chunk
    for c in np.nonzero(single)[0]:
        s = got_rows[c, 2]
        if not (np.isnan(s) if head == "dist" else s == 0.0):
            bad.append(("std of the one-row chunk %d" % c, s))
    if name.split(",")[0] in EXACT_ZERO:
        if not ((got_rows[:, 1] == 0).all() and (got_rows[~single, 2] == 0).all()):
            bad.append(("losses that are exactly zero", got_rows[:, 1:].tolist()))
        parts = [("w", got_rows[:, 0], r32[:, 0], r64[:, 0])]
    else:
        parts = [("w", got_rows[:, 0], r32[:, 0], r64[:, 0]), ("chunk means", got_rows[:, 1], r32[:, 1], r64[:, 1])]
        if (~single).any():
            parts.append(("chunk stds", got_rows[~single, 2], r32[~single, 2], r64[~single, 2]))
        got_c = T.combine_chunk_rows(got_rows.tolist())
        parts.append(("combined mean", [got_c[0]], [c32[0]], [c64[0]]))
        # (n = 1: the row's own std is compared exactly above; the combined std is then the host loop's
        #  sqrt(w (0 + mean^2) / w - mean^2), zero or the square root of a rounding of mean^2 by the last bit of w alone - the
        #  same Python lines for both backends, and nothing a kernel computes)
        if n > 1:
            parts.append(("combined std", [got_c[1]], [c32[1]], [c64[1]]))
    for what, g, a32, a64 in parts:
        assert np.isfinite(np.asarray(a64, np.float64)).all()
        err, bound, need = measure(g, a32, a64)
        worst = max(worst, need)
        log("%-6s %-34s n %3d  %-13s err %.3e  bound %.3e  needs M = %.2f" % (head, name, n, what, err, bound, need))
        if not err <= bound:
            bad.append((what, err, bound, need))
    return bad, worst


# ---- the device side (imported lazily: the CPU tests use the references alone) ----
def device_inputs(case, n, device="cuda"):
    """the device tensors a validation call reads for the first n rows of a case, by name"""
    dev = torch.device(device)
    d = case["data"]
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a[:n], dtype=t)).to(dev)      # noqa: E731
    if case["head"] == "value":
        net = case["net"]
        P = torch.cat([p.detach().reshape(-1).float() for p in FC.learnable(net)]).to(dev).contiguous()
        bounds = torch.cat([net.out_ubound.detach(), net.out_lbound.detach()]).float().to(dev).contiguous()
        return dict(params=P, bounds=bounds, states=up(d[0], np.int8), value=up(d[1], np.float32), variance=up(d[2], np.float32),
                    weight=up(d[3], np.float32))
    atoms, stride = case["atoms"], case["tstride"]
    tp = np.full((n, stride), np.nan, np.float32)          # the padding past the atoms is never read
    tp[:, :atoms] = d[1][:n]
    return dict(params=torch.from_numpy(HN.dn_flat(case["W"])).to(dev).contiguous(), states=up(d[0], np.int8),
                targets=torch.from_numpy(tp).to(dev), weight=up(d[2], np.float32))


def workspace_floats(case, slab):
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    return (lib.tm_valuenet_fit_validate_workspace(slab) if case["head"] == "value"
            else lib.tm_distnet_fit_validate_workspace(slab, case["atoms"]))


def call(case, inp, n, chunk, slab, rows_out, ws, weighted=None):
    """the C call alone (no synchronisation): its return code"""
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    weighted = case["weighted"] if weighted is None else weighted
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    if case["head"] == "value":
        return lib.tm_valuenet_fit_validate(ptr(inp["params"]), ptr(inp["bounds"]), ptr(inp["states"]), ptr(inp["value"]),
                                            ptr(inp["variance"]), ptr(inp["weight"]), n, chunk, slab, int(weighted), CLIP,
                                            ptr(rows_out), ptr(ws), st)
    return lib.tm_distnet_fit_validate(ptr(inp["params"]), ptr(inp["states"]), ptr(inp["targets"]), case["tstride"],
                                       ptr(inp["weight"]), n, chunk, slab, case["atoms"], int(weighted), ptr(rows_out), ptr(ws), st)


def hip_validate(case, n, chunk=CHUNK, slab=SLAB, device="cuda", place=None, weighted=None):
    """one validation call on the first n rows of a case: rows_out as a [ceil(n / chunk), 3] float64 array.  The workspace and
    rows_out start as NaN: no initial contents are required.  `place(n_workspace, 6 * chunks, inputs)` may supply the storage, as
    fit_hip_cases.Arena does for the gradient step: float32 views (workspace, rows_out's 6 floats a chunk, two spare floats)."""
    from tetris_mcts_amd import _lib
    inp = device_inputs(case, n, device)
    nch = (n + chunk - 1) // chunk
    n_ws = workspace_floats(case, slab)
    assert n_ws > 0
    if place is None:
        ws = torch.empty(n_ws, dtype=torch.float32, device=device)
        rows = torch.empty(nch, 3, dtype=torch.float64, device=device)
    else:
        ws, rows32, _spare = place(n_ws, 6 * nch, inp)
        assert ws.numel() == n_ws and rows32.numel() == 6 * nch
        rows = rows32.view(torch.float64).view(nch, 3)
    ws.fill_(float("nan"))
    rows.fill_(float("nan"))
    _lib.check(call(case, inp, n, chunk, slab, rows, ws, weighted), "fit_validate")
    torch.cuda.synchronize()
    return rows.cpu().numpy()
