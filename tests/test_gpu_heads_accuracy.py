"""Accuracy of the value net and the distributional head on the GPU at trained-scale weights (tests/heads_numerics.py has the
weight regimes, the board families and the derivations; tests/test_heads_accuracy.py the CPU side and the measured tables).

Every regime x family: the fp32 kernels equal the oracle's bits; measure A (a derived rounding bound, up to three layers deep)
on the activations the kernels leave in their scratch rows and on the outputs; measure B (a multiple M of the reference's own
fp32 error against an fp64 forward, plus a floor of 4 ulp of the largest output) end to end.  M: heads_numerics.M_* (8 for
every kernel; the reasoning for the split-precision kernels stands there).  Largest needed M measured on the MI355X, with the
GPU machine's own torch CPU fp32 as the yardstick: value net hip 3.72 (x4 / ternary), hip_bf16x3 5.29 (out_ubound from data /
uniform); head hip 6.30, hip_bf16x3 4.96 (both: spread 150, 7 atoms / one-hot).  Largest measure A ratios: value conv1 0.29,
conv2 0.023, conv3 0.041, fc1 0.012, a3 three deep 0.0070 (hip_bf16x3 0.0012), outputs 0.18; head a2 0.020 (hip_bf16x3 0.0041),
log p 0.0006.  profiles/heads_accuracy_pytest_gpu.log has every figure.
"""
import functools

import numpy as np
import pytest
import torch

import heads_numerics as H
from heads_numerics import (DIST_REGIMES, M_DN_FP32, M_DN_X3, M_VN_FP32, M_VN_X3, VALUE_REGIMES, orc_dn, orc_vn)

pytestmark = pytest.mark.gpu
X3_VN = [None, H.c_x3(288), H.c_x3(288), None]        # measure A's constants: conv2 and conv3 are the split layers
X3_DN = [None, H.c_x3(512), None, None]                # conv2 is the split layer
INVALID = 1                                            # hipErrorInvalidValue


@functools.lru_cache(None)
def all_boards():
    """every family in one batch, and each family's slice of it"""
    fam = H.board_families()
    cuts, lo = {}, 0
    for k, b in fam.items():
        cuts[k] = slice(lo, lo + len(b))
        lo += len(b)
    return np.concatenate(list(fam.values())), cuts


def vn_model(backend, P):
    from tetris_mcts_amd.model import Model_VV
    m = Model_VV(backend=backend)
    m.set_flat_params(P)
    return m


def dn_model(backend, atoms, W):
    from tetris_mcts_amd.model_distributional import Model_Dist
    m = Model_Dist(atoms=atoms, backend=backend)
    m.set_flat_params(H.dn_flat(W))
    return m


def vn_run(m, st):
    v, var = m.inference_device(st)
    return torch.stack([v, var], 1).cpu()


def vn_scratch(m, n):
    """the activations a backend leaves behind: {layer index: tensor} (heads_numerics.VN_*_OFF)"""
    if m.backend == "hip_plain":
        s, o = m._scratch_plain[:n].cpu(), H.VN_PLAIN_OFF
        return {0: s[:, o[0]:o[1]], 1: s[:, o[1]:o[2]], 2: s[:, o[2]:o[3]], 3: s[:, o[3]:o[3] + 256]}
    s = m._scratch[:n].cpu()
    return {2: s[:, :1792], 3: s[:, 1792:2048]}


def vn_refs(P, boards):
    """the fp64 forward and the reference's fp32 arithmetic: measure B's two sides"""
    return H.vn_forward(P, boards, torch.float64)[1].numpy(), H.vn_forward(P, boards, torch.float32)[1].numpy()


def vn_measures(P, boards, cuts, out, scratch, cs, M, what, refs=None):
    """measure A on the scratch rows and the outputs, measure B per family; prints every figure before it asserts"""
    rA = H.vn_check_A(P, boards, {**scratch, 4: out}, cs)
    print("A %s: %s" % (what, {k: round(v, 5) for k, v in rA.items()}))
    assert max(rA.values()) <= 1, (what, rA)
    o64, o32 = refs or vn_refs(P, boards)
    for fam, sl in cuts.items():
        e, e_ref, floor = H.errs_B(out.numpy()[sl], o32[sl], o64[sl], per_column=True)
        m = H.needed_M(e, e_ref, floor)
        print("B %s %-8s err %s ref32 %s floor %s needed M %.2f" % (what, fam, e, e_ref, floor, m))
        assert m <= M, (what, fam, e, e_ref, floor)


# ------------------------------------------------------------------------------------------------------------ value net
@pytest.mark.parametrize("regime", VALUE_REGIMES)
def test_value_net_regimes(oracle, regime):
    """hip == hip_plain == oracle bit for bit (outputs, and a3 / the hidden layer between the two kernels' scratch rows); measure A
    on the plain scratch (every layer from its own input) and the matrix-core scratch (a3 three layers deep); hip_bf16x3 under A
    and B"""
    P = H.value_regimes()[regime]
    boards, cuts = all_boards()
    n = len(boards)
    st = torch.from_numpy(boards.reshape(n, 200)).cuda()
    ms = {b: vn_model(b, P) for b in ("hip", "hip_plain", "hip_bf16x3")}
    out = {b: vn_run(m, st) for b, m in ms.items()}
    orc = orc_vn(oracle, P, boards)
    assert out["hip_plain"].numpy().tobytes() == orc.tobytes(), regime
    assert out["hip"].numpy().tobytes() == orc.tobytes(), regime
    sp, sm, sx = (vn_scratch(ms[b], n) for b in ("hip_plain", "hip", "hip_bf16x3"))
    assert torch.equal(sm[2].view(torch.int32), sp[2].contiguous().view(torch.int32)), "a3: matrix cores vs plain"
    assert torch.equal(sm[3].view(torch.int32), sp[3].contiguous().view(torch.int32)), "hidden: matrix cores vs plain"
    refs = vn_refs(P, boards)
    vn_measures(P, boards, cuts, out["hip_plain"], sp, None, M_VN_FP32, "value %s hip_plain" % regime, refs)
    vn_measures(P, boards, cuts, out["hip"], sm, None, M_VN_FP32, "value %s hip" % regime, refs)
    vn_measures(P, boards, cuts, out["hip_bf16x3"], sx, X3_VN, M_VN_X3, "value %s hip_bf16x3" % regime, refs)


def test_value_net_request_path_under_r06(oracle):
    """a short ValueSim and ValueSimLP search under the r06 checkpoint: inference_requests (observations rendered inside the
    convolution kernel) = inference_device(render_eval()) bit for bit on the fp32 backend, the oracle's bits, and A and B on
    those states"""
    from tetris_mcts_amd import agents, store as tst
    from tetris_mcts_amd.pyTetris import Tetris
    P = H.value_regimes()["r06"]
    m = vn_model("hip", P)
    env_args = ((20, 10), 1, 0, 0)
    for name in ("ValueSim", "ValueSimLP"):
        game = Tetris(*env_args, seed=31, n_games=40)
        agent = getattr(agents, name)(sims=12, env=Tetris, env_args=env_args, n_games=40, max_nodes=4000, model=m, online=False)
        agent.update_root(game)
        for _ in range(3):
            act = agent.play()
            game.play(act)
            agent.update_root(game)
        s = agent.store
        s.move_begin(4)
        s.sim_step(tst.SIM_BACKUP | tst.SIM_FRONT)
        states = s.render_eval().clone()
        used = s.t["eval_obs"] != 0
        assert int(used.sum()) > 0
        s.t["eval_v"].fill_(float("nan"))
        s.t["eval_var"].fill_(float("nan"))
        m.inference_requests(s)
        rv, rr = s.t["eval_v"].clone(), s.t["eval_var"].clone()
        vd, rd = m.inference_device(states)
        assert torch.equal(rv[used], vd[used]) and torch.equal(rr[used], rd[used]), name
        assert torch.isnan(rv[~used]).all() and torch.isnan(rr[~used]).all(), name
        boards = states[used].cpu().numpy().reshape(-1, 20, 10)
        out = torch.stack([vd[used], rd[used]], 1).cpu()
        assert out.numpy().tobytes() == orc_vn(oracle, P, boards).tobytes(), name
        dense = vn_run(m, states[used].contiguous())
        assert torch.equal(dense, out)
        vn_measures(P, boards, {"searched": slice(0, len(boards))}, dense, vn_scratch(m, len(boards)), None, M_VN_FP32,
                    "value r06 requests %s" % name)


@pytest.mark.parametrize("entry", ["tm_valuenet_forward", "tm_valuenet_forward_plain", "tm_valuenet_forward-bf16x3"])
def test_value_net_n0_writes_nothing(entry):
    from tetris_mcts_amd import _lib
    from tetris_mcts_amd.store import _p, _stream
    P = H.value_regimes()["params"]
    m = vn_model("hip_bf16x3", P)
    prep = m._ensure_prepared()
    flat = m.flat_params()
    st = torch.zeros(4, 200, dtype=torch.int8, device="cuda")
    v, var = torch.full((4,), float("nan"), device="cuda"), torch.full((4,), float("nan"), device="cuda")
    scr = torch.full((4, H.VN_PLAIN_ROW), float("nan"), device="cuda")
    L = _lib.lib()
    if entry == "tm_valuenet_forward":
        r = L.tm_valuenet_forward(_p(flat), _p(prep), 0, 0, _p(st), 0, _p(v), _p(var), _p(scr), _stream())
    elif entry == "tm_valuenet_forward_plain":
        r = L.tm_valuenet_forward_plain(_p(flat), _p(st), 0, _p(v), _p(var), _p(scr), _stream())
    else:
        r = L.tm_valuenet_forward(_p(flat), _p(prep), 1, 0, _p(st), 0, _p(v), _p(var), _p(scr), _stream())
    torch.cuda.synchronize()
    assert r == 0
    assert torch.isnan(v).all() and torch.isnan(var).all() and torch.isnan(scr).all()


def test_value_net_subnormal_products(oracle):
    """Weights scaled (by exact powers of two) so that every product of conv2 is below fp32's normal range while every sum is
    normal, and conv2's output has bf16 `mid` / `lo` planes that are bf16 subnormals (heads_numerics.subnormal_value_regime).
    hip_plain's fmaf chains equal the oracle's, and so do the fp32 matrix cores' (outputs, a3 and the hidden layer, bit for bit:
    measured on the MI355X - a subnormal product inside the chain is kept, as fmaf keeps it).  hip_bf16x3 is NOT as accurate as
    fp32 arithmetic here: measured 1.9e-4 / 2.8e-3 from the fp64 forward on (v, var) where the fp32 paths are 4.8e-6 / 1.0e-4
    away - bf16 planes below bf16's normal range (2^-126) are lost, so an activation below about 2^-110 keeps its `hi` plane
    only.  What holds there is measure A with the allowances of heads_numerics.chain_bound(tiny=True): K 2^-126 for products, and
    the two lower planes of each operand of a split layer where they can be lost.  DESIGN.md section 4."""
    P = H.subnormal_value_regime()
    boards, cuts = all_boards()
    n = len(boards)
    st = torch.from_numpy(boards.reshape(n, 200)).cuda()
    ms = {b: vn_model(b, P) for b in ("hip", "hip_plain", "hip_bf16x3")}
    out = {b: vn_run(m, st) for b, m in ms.items()}
    orc = orc_vn(oracle, P, boards)
    o64 = H.vn_forward(P, boards, torch.float64)[1].numpy()
    for b in out:
        print("subnormal regime %-10s max |out - oracle| %s  max |out - fp64| %s  bits equal %s" % (
            b, np.abs(out[b].numpy() - orc).max(0), np.abs(out[b].numpy() - o64).max(0), out[b].numpy().tobytes() == orc.tobytes()))
    assert out["hip_plain"].numpy().tobytes() == orc.tobytes()
    sp, sm, sx = (vn_scratch(ms[b], n) for b in ("hip_plain", "hip", "hip_bf16x3"))
    print("subnormal regime a3 bits hip == plain: %s, hidden: %s" % (
        torch.equal(sm[2].view(torch.int32), sp[2].contiguous().view(torch.int32)),
        torch.equal(sm[3].view(torch.int32), sp[3].contiguous().view(torch.int32))))
    assert out["hip"].numpy().tobytes() == orc.tobytes()
    assert torch.equal(sm[2].view(torch.int32), sp[2].contiguous().view(torch.int32))
    assert torch.equal(sm[3].view(torch.int32), sp[3].contiguous().view(torch.int32))
    for b, sc, cs in (("hip_plain", sp, None), ("hip", sm, None), ("hip_bf16x3", sx, X3_VN)):
        rA = H.vn_check_A(P, boards, {**sc, 4: out[b]}, cs, True)
        print("subnormal regime A (+ the allowances for lost subnormals) %-10s %s" % (b, {k: round(v, 5) for k, v in rA.items()}))
        assert max(rA.values()) <= 1, (b, rA)


# ------------------------------------------------------------------------------------------------- distributional head
def dn_measures(W, boards, cuts, p, a2, cs, M, what, refs):
    rA = H.dn_check_A(W, boards, {1: a2, 3: p}, cs)
    print("A %s: %s" % (what, {k: round(v, 5) for k, v in rA.items()}))
    assert max(rA.values()) <= 1, (what, rA)
    p64, p32 = refs
    for fam, sl in cuts.items():
        m_lp, m_sum = H.dn_B(p.numpy()[sl], p32[sl], p64[sl])
        print("B %s %-8s needed M log p %.2f sum %.2f" % (what, fam, m_lp, m_sum))
        assert m_lp <= M and m_sum <= M, (what, fam, m_lp, m_sum)


@pytest.mark.parametrize("regime", DIST_REGIMES)
def test_dist_head_regimes(oracle, regime):
    """hip == oracle bit for bit; A (conv2's output two layers deep, log p two layers deep from it) and B for hip and hip_bf16x3;
    rows sum to one; the columns at and beyond `atoms` of a zeroed output stay exactly zero"""
    atoms, W = H.dist_regimes()[regime]
    boards, cuts = all_boards()
    n = len(boards)
    st = torch.from_numpy(boards.reshape(n, 200)).cuda()
    orc = orc_dn(oracle, W, boards, atoms)
    refs = H.dn_forward(W, boards, torch.float64)[1].numpy(), H.dn_forward(W, boards, torch.float32)[1].numpy()
    for backend, cs, M in (("hip", None, M_DN_FP32), ("hip_bf16x3", X3_DN, M_DN_X3)):
        m = dn_model(backend, atoms, W)
        full = m.inference_device(st).cpu()
        p, a2 = full[:, :atoms].contiguous(), m._scratch[:n, :2048].cpu()
        if backend == "hip":
            assert p.numpy().tobytes() == orc.tobytes(), regime
        assert float(full[:, atoms:].abs().sum()) == 0.0 and not bool(torch.isnan(full).any())
        assert float((p.double().sum(1) - 1).abs().max()) <= 1e-5
        dn_measures(W, boards, cuts, p, a2, cs, M, "dist %s %s" % (regime, backend), refs)


SIZES = (1, 3, 4, 5, 15, 16, 17, 31, 33, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097)


@pytest.mark.parametrize("backend", ["hip", "hip_bf16x3"])
def test_dist_head_batch_sizes(oracle, backend):
    """around the 4-state convolution workgroups, the 16-state FC tiles and the grid caps (512 workgroups of k_dn_conv, 256 of
    k_dn_conv_x3, beyond which the waves stride over the states): the scratch filled with random words and the output with NaN
    before every launch; hip against the oracle's bits, hip_bf16x3 against its own single-state results; nothing written at or
    beyond `atoms`"""
    atoms, W = 50, H.peaked(H.seeded_dist_net(50), 50)
    rng = np.random.default_rng(4097)
    boards = rng.integers(-1, 2, size=(4097, 200)).astype(np.int8)
    boards[::2, :100] = 0
    st = torch.from_numpy(boards).cuda()
    m = dn_model(backend, atoms, W)
    m.hip_buffers(4097)
    if backend == "hip":
        ref = torch.from_numpy(orc_dn(oracle, W, boards, atoms))
    else:
        ref = torch.cat([m.inference_device(st[i:i + 1])[:, :atoms].clone() for i in range(4097)]).cpu()
    for n in SIZES:
        m._scratch.view(torch.int32).random_(-2 ** 31, 2 ** 31 - 1)
        out = torch.full((n, 64), float("nan"), device="cuda")
        m.inference_device(st[:n].contiguous(), out)
        out = out.cpu()
        assert torch.equal(out[:, :atoms].view(torch.int32), ref[:n].contiguous().view(torch.int32)), n
        assert bool(torch.isnan(out[:, atoms:]).all()), n


def _dn_call(m, st, n, atoms, out, stride):
    from tetris_mcts_amd import _lib
    from tetris_mcts_amd.store import _p, _stream
    P, prep, scr = m.hip_buffers(max(n, 1))
    return _lib.lib().tm_distnet_forward(P, prep, 1 if m.backend == "hip_bf16x3" else 0, _p(st), n, atoms, _p(out), stride, scr,
                                         _stream())


@pytest.mark.parametrize("backend", ["hip", "hip_bf16x3"])
def test_dist_head_strides_and_refused_arguments(oracle, backend):
    """dist_stride 50 (= atoms) and 70 through the C ABI: the guard columns and the words behind the last row stay untouched;
    atoms 0 and 65 and dist_stride < atoms are refused on the host (hipErrorInvalidValue) and n = 0 returns 0, nothing written"""
    atoms, W = 50, H.seeded_dist_net(50)
    boards = H.ternary_boards(37, 9).reshape(37, 200)
    st = torch.from_numpy(boards).cuda()
    m = dn_model(backend, atoms, W)
    ref = m.inference_device(st)[:, :atoms].clone().cpu()
    if backend == "hip":
        assert ref.numpy().tobytes() == orc_dn(oracle, W, boards, atoms).tobytes()
    for stride in (50, 70):
        buf = torch.full((37 * stride + 64,), float("nan"), device="cuda")
        assert _dn_call(m, st, 37, atoms, buf, stride) == 0
        torch.cuda.synchronize()
        rows = buf[:37 * stride].reshape(37, stride).cpu()
        assert torch.equal(rows[:, :atoms].contiguous().view(torch.int32), ref.view(torch.int32)), stride
        assert bool(torch.isnan(rows[:, atoms:]).all()) and bool(torch.isnan(buf[37 * stride:]).all()), stride
    buf = torch.full((37 * 70 + 64,), float("nan"), device="cuda")
    for n, a, stride, want in ((37, 0, 64, INVALID), (37, 65, 70, INVALID), (37, 50, 49, INVALID), (0, 50, 64, 0)):
        assert _dn_call(m, st, n, a, buf, stride) == want, (n, a, stride)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all()), (n, a, stride)
