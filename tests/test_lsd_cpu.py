"""Localized-statistics decoding on the host (ops.lsd_host -> gnnd_lsd_host, ops.lsd_gated_host,
ops.bplsd_host) against the independent statement of tests/lsd_cases.py, exact equality of every
output; the two consequences of the definition (status is osd0's; the estimate is osd0's for the
column order "cluster variables first"); hand cases on the toric codes; the gated and one-call
mirrors against compositions of the pieces; the refusals through the raw ABI.  CPU only."""
import ctypes

import numpy as np
import pytest

from gnndecode import _lib, ops

import bposd_cases as bc
import lsd_cases as lc
import minsum_cases as mc
import osd_cases as oc

DTYPES = ('float32', 'float64')
BASES = ('zero', 'hard')


@pytest.mark.parametrize('bits', lc.BITS)
@pytest.mark.parametrize('base', BASES)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('code,B', lc.SHAPES)
def test_mirror_equals_statement_and_has_both_consequences(code, B, dtype, base, bits):
    H, x, p = oc.inputs(code, B, dtype)
    V, C = H.shape
    ref = lc.reference(code, B, dtype, base, bits)
    got = ops.lsd_host(H, x, p, base, bits)
    lc.assert_equal(got, lc.as_tuple(ref, dtype), (code, B, dtype, base, bits))
    # P1: the status of osd0; a solution wherever there is one
    e0, s0 = ops.osd0_host(H, x, p, base)
    assert np.array_equal(got[1], s0)
    ok = got[1] == 0
    assert oc.satisfied(H, x, got[0])[ok].all()
    assert np.array_equal(got[0].reshape(B, V)[~ok], e0.reshape(B, V)[~ok])      # the base vector
    assert (got[2] <= V + 1).all() and (got[4] <= V).all() and (got[3] <= C).all()
    # P2: osd0 with the final cluster variables first, then the rest, both in `order` order
    pb = p.reshape(B, V)
    hard = base == 'hard'
    key = -np.abs(pb - 0.5) if hard else pb.copy()
    key = np.where(np.isnan(key), -np.inf, key)
    p2 = np.empty_like(pb)
    for b in range(B):
        order = np.lexsort((np.arange(V), -key[b]))
        inV = ref['inV'][b]
        walk = np.concatenate([order[inV[order]], order[~inV[order]]])
        pos = np.empty(V, np.int64)
        pos[walk] = np.arange(V)
        if hard:
            z = np.nan_to_num(pb[b], nan=0.0) > 0.5
            p2[b] = 0.5 + np.where(z, 1, -1) * (pos + 1) / (4.0 * (V + 1))
        else:
            p2[b] = (V - pos) / (V + 1.0)
    e2, s2 = ops.osd0_host(H, x, p2.reshape(-1), base)
    assert np.array_equal(s2, s0)
    assert np.array_equal(e2.reshape(B, V)[ok], got[0].reshape(B, V)[ok])


@pytest.mark.parametrize('L', [5, 7])
def test_hand_cases_on_the_toric_codes(L):
    H = oc.code_matrix(f'toric_{L}')
    V, C = H.shape
    Hi = H.astype(np.int64)
    for v in (0, V // 2 + 3, V - 1):
        H, x, p = lc.hand_case(L, [v])
        ehat, status, rounds, nclus, ncols = ops.lsd_host(H, x, p, 'zero', 1)
        assert np.flatnonzero(ehat).tolist() == [v]
        assert (status[0], rounds[0], nclus[0], ncols[0]) == (0, 1, 1, 1)
    # two flips whose checks share no variable
    a = 0
    near = (Hi @ Hi[a] > 0) | (Hi @ ((Hi @ Hi[a] > 0) @ Hi > 0) > 0)
    b = int(np.flatnonzero(~near)[0])
    H, x, p = lc.hand_case(L, [a, b])
    ehat, status, rounds, nclus, ncols = ops.lsd_host(H, x, p, 'zero', 1)
    assert np.flatnonzero(ehat).tolist() == sorted([a, b])
    assert (status[0], rounds[0], nclus[0], ncols[0]) == (0, 1, 2, 2)
    lc.assert_equal((ehat, status, rounds, nclus, ncols),
                    lc.as_tuple(lc.ref_batch(H, x, p, False, 1), 'float64'))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('code,B', bc.SHAPES)
def test_gated_mirror_is_the_composition(code, B, dtype):
    H, x, p = oc.inputs(code, B, dtype)
    V = H.shape[0]
    llr = bc.llr_input(code, B, dtype)
    for name in bc.GATES:
        g = bc.gate(code, B, dtype, name)
        for base, bits, with_llr in (('zero', 1, True), ('hard', 0, False)):
            full = lc.reference(code, B, dtype, base, bits)
            l = llr if with_llr else None
            want = [full[k].copy() for k in lc.NAMES]
            off = g == 0
            want[0][off] = bc.hard_decision(p, l).reshape(B, V)[off]
            for a in want[1:]:
                a[off] = 0
            got = ops.lsd_gated_host(H, x, p, g, base, bits, llr=l)
            lc.assert_equal(got, (want[0].reshape(-1).astype(dtype),) + tuple(want[1:]),
                            (code, name, base, bits))


@pytest.mark.parametrize('dtype', DTYPES)
def test_bplsd_mirror_is_minsum_then_gated_lsd_and_bposd_on_the_solved_rows(dtype):
    H, x, args = lc.bp_inputs(dtype)
    V, C = H.shape
    B = lc.BP_B
    for base, bits in (('zero', 1), ('hard', 0), ('zero', 3)):
        out = ops.bplsd_host(H, x, *args, base, bits)
        ehat, status, rounds, nclus, ncols, its, bp, pred, llr = out
        po = ops.bposd_host(H, x, *args, base, 'osd0', 0)
        for a, b in zip((its, bp, pred, llr), po[3:]):
            assert np.array_equal(a, b, equal_nan=True)
        solved = bp == 0
        assert solved.any() and (~solved).any()
        assert np.array_equal(ehat.reshape(B, V)[solved], po[0].reshape(B, V)[solved])
        assert np.array_equal(status, po[1])                                       # P1
        assert not rounds[solved].any() and not nclus[solved].any() and not ncols[solved].any()
        lc.assert_equal(out[:5], ops.lsd_gated_host(H, x, pred, bp, base, bits, llr=llr))
        assert oc.satisfied(H, x, ehat).all() and not status.any()
        # the statement on min-sum's soft output, where min-sum stopped unsolved
        ref = lc.ref_batch(H, x, pred, base == 'hard', bits)
        assert np.array_equal(ehat.reshape(B, V)[~solved], ref['ehat'][~solved])
        assert np.array_equal(rounds[~solved], ref['rounds'][~solved])


def test_refusals_through_the_raw_abi():
    lib = _lib.get()
    H, x, p = oc.inputs('toric_5', 9, 'float64')
    V, C = H.shape
    from gnndecode.graph import edge_list
    var, chk = edge_list(H)
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    vp, cp = var.ctypes.data_as(P64), chk.ctypes.data_as(P64)
    ehat = np.full(9 * V, 7.0)
    ints = [np.full(9, 7, np.int32) for _ in range(4)]
    ip = [a.ctypes.data_as(P32) for a in ints]
    gate = np.ones(9, np.int32)
    gp = gate.ctypes.data_as(P32)

    def lsd(dtype=_lib.F64, xx=x.ctypes.data, pp=p.ctypes.data, base=0, bits=1,
            eh=ehat.ctypes.data, B=9):
        return lib.gnnd_lsd_host(vp, cp, var.size, V, C, dtype, xx, pp, base, bits, eh, *ip, B)

    assert lsd(bits=-1) == _lib.ERR_INVALID_ARG
    assert lsd(base=2) == _lib.ERR_INVALID_ARG
    assert lsd(xx=None) == _lib.ERR_INVALID_ARG
    assert lsd(pp=None) == _lib.ERR_INVALID_ARG
    assert lsd(eh=None) == _lib.ERR_INVALID_ARG
    assert lsd(dtype=7) == _lib.ERR_INVALID_ARG
    assert lsd(B=-1) == _lib.ERR_INVALID_ARG
    assert lsd(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert lsd(B=0, xx=None, pp=None, eh=None) == _lib.OK
    assert lib.gnnd_lsd_gated_host(vp, cp, var.size, V, C, _lib.F64, x.ctypes.data, p.ctypes.data,
                                   None, None, 0, 1, ehat.ctypes.data, *ip, 9) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_lsd_gated_host(vp, cp, var.size, V, C, _lib.F64, x.ctypes.data, p.ctypes.data,
                                   None, gp, 0, -2, ehat.ctypes.data, *ip, 9) == _lib.ERR_INVALID_ARG
    for kw in (dict(bits=-1), dict(base=5), dict(iters=0), dict(alpha=0.0), dict(pred=None),
               dict(llr=None), dict(bp=None)):
        a = dict(bits=1, base=0, iters=5, alpha=0.75, pred=ehat.ctypes.data, llr=ehat.ctypes.data,
                 bp=ip[0])
        a.update(kw)
        st = lib.gnnd_bplsd_host(vp, cp, var.size, V, C, _lib.F64, x.ctypes.data, a['alpha'], 0.0,
                                 a['iters'], 1, a['base'], a['bits'], a['pred'], a['llr'], None,
                                 a['bp'], ehat.ctypes.data, None, None, None, None, 9)
        assert st == _lib.ERR_INVALID_ARG, kw
    assert (ehat == 7).all() and all((a == 7).all() for a in ints)
    # the device entries refuse the same arguments before any device call: no graph is needed
    assert lib.gnnd_lsd(None, _lib.F64, None, None, 0, 1, None, None, None, None, None, 1,
                        None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_lsd_gated(None, _lib.F64, None, None, None, None, 0, 1, None, None, None, None,
                              None, None, 0, 1, None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_bplsd(None, _lib.F64, None, 0.75, 0.0, 5, 1, 0, 1, None, None, None, None, None,
                          None, None, None, None, None, 0, 1, None) == _lib.ERR_INVALID_ARG
    # optional outputs skipped: the same ehat
    full = ops.lsd_host(H, x, p, 'zero', 1)
    e2 = np.empty_like(ehat)
    assert lib.gnnd_lsd_host(vp, cp, var.size, V, C, _lib.F64, x.ctypes.data, p.ctypes.data, 0, 1,
                             e2.ctypes.data, None, None, None, None, 9) == _lib.OK
    assert np.array_equal(e2, full[0])
    for bad in (dict(bits_per_step=-1), dict(bits_per_step=1.5), dict(bits_per_step=True),
                dict(base='soft')):
        with pytest.raises(ValueError):
            ops.lsd_host(H, x, p, **bad)
