"""The prepared buffer of the leaf evaluators is ONE buffer whose parts are prefixes (include/tetris_mcts_hip.h): the fp32 operand
streams, then the convolutions' planes, then (value net) fc1's planes.  tm_*_prepare writes exactly the parts its mode names, so a
buffer prepared for the largest mode gives every smaller mode the output bytes of a buffer prepared for that mode alone."""
import numpy as np
import pytest
import torch

import heads_numerics as H

pytestmark = pytest.mark.gpu
VN_MODES = ((0, 0), (1, 0), (1, 1))        # (backend, fc1)
VN_PARTS = (477184, 27648, 688128)         # TM_VALUENET_PREPARED, _PREPARED_X3, _PREPARED_FC1_X3
DN_PARTS = (278528, 24576)                 # TM_DISTNET_PREPARED, _PREPARED_X3
GUARD = 0x7FC0BEEF                         # (a NaN's bits: whatever reads a word that was never prepared shows)


def _prepared(entry, P, mode, floats, total):
    """a buffer of `total` floats, all guard words, prepared for `mode`: exactly its first `floats` floats are written"""
    from tetris_mcts_amd import _lib
    from tetris_mcts_amd.store import _p, _stream
    buf = torch.full((total,), GUARD, dtype=torch.int32, device="cuda")
    assert getattr(_lib.lib(), entry)(_p(P), _p(buf), *mode, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((buf[floats:] == GUARD).all()), (entry, mode)
    return buf


def _vn_total(mode):
    return VN_PARTS[0] + (VN_PARTS[1] if mode[0] else 0) + (VN_PARTS[2] if mode[1] else 0)


def test_value_net_modes_read_a_prefix_of_the_largest_buffer():
    """n = 33 (one state over a 32-row tile), 4 097 (one over the split fc1's switch to 64-row tiles on 256 CUs) and 8 192 (the fp32
    fc1's switch); scratch filled with random words and the outputs with NaN before every launch"""
    from tetris_mcts_amd import _lib
    from tetris_mcts_amd.store import _p, _stream
    L = _lib.lib()
    P = torch.from_numpy(H.value_regimes()["r06"]).cuda()
    st = torch.from_numpy(H.ternary_boards(8192).reshape(8192, 200)).cuda()
    big = _prepared("tm_valuenet_prepare", P, (1, 1), sum(VN_PARTS), sum(VN_PARTS))
    own = {m: _prepared("tm_valuenet_prepare", P, m, _vn_total(m), sum(VN_PARTS)) for m in VN_MODES}
    for m in VN_MODES:      # the same bytes, part for part
        assert torch.equal(own[m][:_vn_total(m)], big[:_vn_total(m)]), m
    scr = torch.empty(8192, 2064, dtype=torch.int32, device="cuda")
    for n in (33, 4097, 8192):
        for m in VN_MODES:
            outs = []
            for prep in (big, own[m][:_vn_total(m)].clone()):
                scr.random_(-2 ** 31, 2 ** 31 - 1)
                v, var = torch.full((n,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
                assert L.tm_valuenet_forward(_p(P), _p(prep), *m, _p(st), n, _p(v), _p(var), _p(scr), _stream()) == 0
                torch.cuda.synchronize()
                assert not bool(torch.isnan(v).any() or torch.isnan(var).any()), (n, m)
                outs.append((v.cpu().numpy().tobytes(), var.cpu().numpy().tobytes()))
            assert outs[0] == outs[1], (n, m)


def test_dist_head_backends_read_a_prefix_of_the_larger_buffer():
    """the head's two backends at n = 33 and 4 097 (beyond both convolution kernels' grid caps)"""
    from tetris_mcts_amd import _lib
    from tetris_mcts_amd.store import _p, _stream
    L = _lib.lib()
    atoms = 50
    P = torch.from_numpy(np.ascontiguousarray(H.dn_flat(H.seeded_dist_net(atoms)))).float().cuda()
    st = torch.from_numpy(H.ternary_boards(4097).reshape(4097, 200)).cuda()
    big = _prepared("tm_distnet_prepare", P, (1,), sum(DN_PARTS), sum(DN_PARTS))
    own = {0: _prepared("tm_distnet_prepare", P, (0,), DN_PARTS[0], sum(DN_PARTS))[:DN_PARTS[0]].clone(),
           1: _prepared("tm_distnet_prepare", P, (1,), sum(DN_PARTS), sum(DN_PARTS))}
    assert torch.equal(own[0], big[:DN_PARTS[0]]) and torch.equal(own[1], big)
    scr = torch.empty(4097, 2048, dtype=torch.int32, device="cuda")
    for n in (33, 4097):
        for backend in (0, 1):
            outs = []
            for prep in (big, own[backend]):
                scr.random_(-2 ** 31, 2 ** 31 - 1)
                out = torch.full((n, 64), float("nan"), device="cuda")
                assert L.tm_distnet_forward(_p(P), _p(prep), backend, _p(st), n, atoms, _p(out), 64, _p(scr), _stream()) == 0
                torch.cuda.synchronize()
                out = out.cpu()
                assert not bool(torch.isnan(out[:, :atoms]).any()) and bool(torch.isnan(out[:, atoms:]).all()), (n, backend)
                outs.append(out[:, :atoms].numpy().tobytes())
            assert outs[0] == outs[1], (n, backend)
