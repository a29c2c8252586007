"""Packed observations for the tests of the fits' packed route (tm_*_fit_grad_packed, tm_*_fit_validate_packed,
train_data(state_format="packed")), shared by tests/test_fit_packed.py (CPU) and tests/test_gpu_fit_packed.py (GPU).

`pack` is the inverse of dist.render_observations on the boards the case modules build (fit_hip_cases.boards, dist_fit_cases.dataset:
a stack of locked cells and a falling piece of exactly four cells), so their data is reused as it is: the packed calls are compared
with the int8 calls on the same rows, bytes against bytes.  ENGINE_SPEC section 7 has the layout: words 0..9 hold two board rows
of 16 bits each (bit c = column c locked), word 10 the four cell codes 10 r + c of the piece, word 11 the ended flag in its low
byte."""
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

CLIP = 0.1          # train.variance_bound, as fit_hip_cases.hip_grad passes it


def pack(boards):
    """int8 [n,200] boards (0 empty, 1 locked, -1 the falling piece: four cells, or none) -> int32 [n,12] observations.  A board
    with a piece: its cell codes ascending in word 10, word 11 = 0.  A board without one: an ended observation (word 10 =
    0xFFFFFFFF, word 11 = 1)."""
    b = np.asarray(boards).reshape(-1, 20, 10)
    assert np.isin(b, (-1, 0, 1)).all()
    n = b.shape[0]
    piece = (b == -1).reshape(n, 200)
    count = piece.sum(1)
    assert np.isin(count, (0, 4)).all(), "a board holds a piece of four cells or none"
    rows = ((b == 1).astype(np.uint32) << np.arange(10, dtype=np.uint32)).sum(2).astype(np.uint32)      # [n,20], 10 bits each
    out = np.zeros((n, 12), np.uint32)
    out[:, :10] = rows[:, 0::2] | (rows[:, 1::2] << np.uint32(16))
    out[:, 10] = 0xFFFFFFFF
    out[:, 11] = 1
    live = np.nonzero(count == 4)[0]
    codes = np.nonzero(piece[live])[1].reshape(-1, 4).astype(np.uint32)                                  # ascending by construction
    out[live, 10] = codes[:, 0] | (codes[:, 1] << np.uint32(8)) | (codes[:, 2] << np.uint32(16)) | (codes[:, 3] << np.uint32(24))
    out[live, 11] = 0
    return out.view(np.int32)


def render(obs):
    """dist.render_observations on the CPU: int32 [n,12] -> int8 [n,200]"""
    from tetris_mcts_amd import dist as tdist
    return tdist.render_observations(torch.from_numpy(np.ascontiguousarray(obs))).reshape(-1, 200).numpy().astype(np.int8)


def edge_boards():
    """boards whose piece touches row 0, row 19, column 0 and column 9 (next to locked cells), one with a piece over the whole
    top-left corner block, and two without a piece (ended observations), one of them full of locked cells"""
    rng = np.random.default_rng(3)
    b = (rng.random((8, 20, 10)) < 0.4).astype(np.int8)
    b[0, 0, 0:4] = -1                    # row 0, column 0
    b[1, 0, 6:10] = -1                   # row 0, column 9
    b[2, 19, 0:4] = -1                   # row 19, column 0
    b[3, 19, 6:10] = -1                  # row 19, column 9
    b[4, 0:4, 0] = -1                    # a column of four at column 0
    b[5, 16:20, 9] = -1                  # a column of four at column 9, down to row 19
    b[6] = 1                             # no piece, every cell locked
    b[7, :10] = 0                        # no piece
    return b.reshape(8, 200)


def mixed_value_case():
    """300 rows: fit_hip_cases' boards with 40 ended rows and the edge boards mixed in; batch 33, idx out of order and with repeats"""
    states, value, variance, weight = FC.dataset(300, 31)
    states = states.copy()
    rng = np.random.default_rng(32)
    ended = rng.choice(300, 40, replace=False)
    states[ended] = np.where(states[ended] == -1, 0, states[ended])
    edges = edge_boards()
    where = np.setdiff1d(np.arange(300), ended)[:len(edges)]
    states[where] = edges
    idx = np.concatenate([ended[:9], where, rng.integers(0, 300, 12), where[:4]])[::-1].copy()
    assert len(idx) == 33 and len(np.unique(idx)) < 33
    return dict(net=FC.fresh_net(0), data=(states, value, variance, weight), idx=idx, batch=33, weighted=True)


_VALUE = {}


def value_cases():
    """fit_hip_cases.cases(), built once"""
    if not _VALUE:
        _VALUE.update(FC.cases())
    return _VALUE


# ---- the device side ----
def _idx(idx, dev):
    return None if idx is None else torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev)


def value_grad_packed(case, device="cuda", place=None):
    """fit_hip_cases.hip_grad with tm_valuenet_fit_grad_packed on pack(states): (gradient, loss, the key tensor after the call, its
    bytes before the call)"""
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    net, (states, value, variance, weight), idx, B = case["net"], case["data"], case["idx"], case["batch"]
    dev = torch.device(device)
    P = torch.cat([p.detach().reshape(-1).float() for p in FC.learnable(net)]).to(dev).contiguous()
    bounds = torch.cat([net.out_ubound.detach(), net.out_lbound.detach()]).float().to(dev).contiguous()
    keys_host = pack(states)
    keys = torch.from_numpy(keys_host).to(dev)
    val, var, w = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (value, variance, weight))
    idx_t = _idx(idx, dev)
    assert idx is None or (len(idx) == B and 0 <= int(np.min(idx)) and int(np.max(idx)) < len(states))
    n_ws = lib.tm_valuenet_fit_workspace(B)
    if place is None:
        ws, grad, loss = (torch.empty(n, dtype=torch.float32, device=dev) for n in (n_ws, FC.N_LEARN, 2))
    else:
        ws, grad, loss = place(n_ws, FC.N_LEARN, dict(params=P, bounds=bounds, states=keys, value=val, variance=var, weight=w, idx=idx_t))
    for t in (ws, grad, loss):
        t.fill_(float("nan"))
    _lib.check(lib.tm_valuenet_fit_grad_packed(P.data_ptr(), bounds.data_ptr(), keys.data_ptr(), val.data_ptr(), var.data_ptr(),
                                               w.data_ptr(), idx_t.data_ptr() if idx_t is not None else None, B,
                                               int(case["weighted"]), CLIP, grad.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream), "tm_valuenet_fit_grad_packed")
    torch.cuda.synchronize()
    return grad.cpu().numpy(), loss.cpu().numpy(), keys, keys_host.tobytes()


def dist_grad_packed(case, device="cuda", place=None):
    """dist_fit_cases.hip_grad with tm_distnet_fit_grad_packed on pack(states)"""
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    (states, target, weight), idx, B, atoms, stride = case["data"], case["idx"], case["batch"], case["atoms"], case["tstride"]
    dev = torch.device(device)
    P = torch.from_numpy(HN.dn_flat(case["W"])).to(dev).contiguous()
    keys_host = pack(states)
    keys = torch.from_numpy(keys_host).to(dev)
    tp = np.full((len(target), stride), np.nan, np.float32)
    tp[:, :atoms] = target
    t, w = torch.from_numpy(tp).to(dev), torch.from_numpy(np.ascontiguousarray(weight, dtype=np.float32)).to(dev)
    idx_t = _idx(idx, dev)
    assert idx is None or (len(idx) == B and 0 <= int(np.min(idx)) and int(np.max(idx)) < len(states))
    n_ws = lib.tm_distnet_fit_workspace(B, atoms)
    if place is None:
        ws, grad, loss = (torch.empty(n, dtype=torch.float32, device=dev) for n in (n_ws, DC.n_params(atoms), 2))
    else:
        ws, grad, loss = place(n_ws, DC.n_params(atoms), dict(params=P, states=keys, targets=t, weight=w, idx=idx_t))
    for b in (ws, grad, loss):
        b.fill_(float("nan"))
    _lib.check(lib.tm_distnet_fit_grad_packed(P.data_ptr(), keys.data_ptr(), t.data_ptr(), stride, w.data_ptr(),
                                              idx_t.data_ptr() if idx_t is not None else None, B, atoms, int(case["weighted"]),
                                              grad.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream), "tm_distnet_fit_grad_packed")
    torch.cuda.synchronize()
    return grad.cpu().numpy(), loss.cpu().numpy(), keys, keys_host.tobytes()


def validation_case(head, n):
    """a fit_validation_cases case of n rows: the fresh value net, or the fixture head at 50 atoms"""
    if head == "value":
        return dict(head="value", net=FC.fresh_net(0), data=FC.dataset(n, 7), weighted=True)
    atoms, W = 50, HN.fixture_dist_net()
    return dict(head="dist", W=W, atoms=atoms, data=DC.dataset(n, atoms, 7), weighted=True, tstride=atoms)


def validate_packed(case, inp, keys, n, chunk, slab, rows_out, ws):
    """the packed validation call on the inputs of fit_validation_cases.device_inputs, the states replaced by `keys`"""
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    if case["head"] == "value":
        return lib.tm_valuenet_fit_validate_packed(inp["params"].data_ptr(), inp["bounds"].data_ptr(), keys.data_ptr(),
                                                   inp["value"].data_ptr(), inp["variance"].data_ptr(), inp["weight"].data_ptr(), n,
                                                   chunk, slab, int(case["weighted"]), CLIP, rows_out.data_ptr(), ws.data_ptr(), st)
    return lib.tm_distnet_fit_validate_packed(inp["params"].data_ptr(), keys.data_ptr(), inp["targets"].data_ptr(), case["tstride"],
                                              inp["weight"].data_ptr(), n, chunk, slab, case["atoms"], int(case["weighted"]),
                                              rows_out.data_ptr(), ws.data_ptr(), st)
