"""Soft relay and relay+OSD, host mirrors (gnnd_relay_soft_host, gnnd_relay_osd_host through
ops.relay_soft_host / ops.relay_osd_host) against the numpy statement (tests/relay_osd_cases.py):
soft, llr and the integers bit for bit in both dtypes and both soft modes, the OSD stage for the
soft probability the mirror returned, the relay outputs against relay_host, the one-leg zero-gamma
LAST case against bposd_host(early_stop=True), and the refusals, NULL outputs and empty batch of
the four C entry points (all decided before any device call).  CPU only."""
import ctypes

import numpy as np
import pytest

from gnndecode import _lib, ops

import minsum_cases as mc
import relay_cases as rc
import relay_osd_cases as roc

# every shape of the device tests at the parameter sets that keep the numpy statement quick
CASES = ([(code, B, p) for _, code, B in roc.SHAPES if code != 'ldpc_648_324' for p in rc.PARAMS]
         + [('ldpc_648_324', 3, rc.PARAMS[0]), ('ldpc_648_324', 3, rc.PARAMS[3])])


def _args(code, B, dtype, params):
    legs, iters0, iters_leg, S = params
    H, x = roc.inputs(code, B, dtype, params)
    return H, x, (rc.gammas(H.shape[0], params, dtype), iters0, iters_leg, S, rc.ALPHA, rc.BETA)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B,params', CASES)
def test_mirrors_equal_the_numpy_statement(code, B, params, dtype):
    ref = roc.reference(code, B, dtype, params)
    H, x, args = _args(code, B, dtype, params)
    V = H.shape[0]
    plain = ops.relay_host(H, x, *args)
    for mode in roc.MODES:
        pred, soft, *relay = ops.relay_soft_host(H, x, *args, soft=mode)
        rc.assert_equal(tuple(relay), ref, (code, B, dtype, params, mode))
        rc.assert_equal(tuple(relay), plain, 'relay_soft_host against relay_host')
        assert soft.dtype == x.dtype and np.array_equal(soft, ref['soft_' + mode])
        assert np.array_equal(np.signbit(soft), np.signbit(ref['soft_' + mode]))
        np.testing.assert_allclose(pred, ref['pred_' + mode], **mc.pred_tolerance(dtype))
        got = ops.relay_osd_host(H, x, *args, soft=mode, base=roc.base_of(code))
        ehat, status, choice, o_pred, o_llr, o_its, o_rst, o_leg, o_nsol = got
        assert np.array_equal(o_pred, pred)
        rc.assert_equal(((o_llr < 0).astype(x.dtype), o_llr, o_its, o_rst, o_leg, o_nsol), ref)
        # the OSD stage orders its columns by pred, whose exponential is the mirror's own: the
        # statement takes pred as given (as tests/bposd_cases.py does)
        r_e, r_s, r_c = roc.osd_stage(code, x, pred, ref['status'], ref['llr'])
        assert np.array_equal(ehat.reshape(-1, V), r_e.astype(x.dtype))
        assert np.array_equal(status, r_s) and np.array_equal(choice, r_c)
        solved = o_rst == 0
        assert (choice[solved] == -1).all() and (status[solved] == 0).all()
        assert np.array_equal(ehat.reshape(-1, V)[solved], relay[0].reshape(-1, V)[solved])
        assert rc.satisfied(H, x, -ehat)[status == 0].all()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B', [('toric_5', 67), ('bch_63_45', 33)])
def test_one_leg_zero_gamma_last_is_bposd(code, B, dtype):
    H, x = mc.inputs(code, B, dtype)
    base = roc.base_of(code)
    got = ops.relay_osd_host(H, x, np.zeros((1, H.shape[0])), 12, soft='last', base=base)
    ehat, status, choice, pred, llr, its, rst, leg, nsol = got
    b = ops.bposd_host(H, x, 12, early_stop=True, base=base)
    for a, w in zip((ehat, status, choice, its, rst, pred, llr), b):
        assert a.dtype == w.dtype and np.array_equal(a, w)
    assert np.array_equal(np.signbit(llr), np.signbit(b[6]))
    assert set(rst.tolist()) == {0, 1}


def test_refusals_null_outputs_and_empty_batch():
    lib = _lib.get()
    H, x = roc.inputs('toric_5', 9, 'float64', rc.PARAMS[1])
    V, C = H.shape
    B = 9
    from gnndecode.graph import edge_list
    var, chk = edge_list(H)
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    vp, cp = var.ctypes.data_as(P64), chk.ctypes.data_as(P64)
    gm = rc.gammas(V, rc.PARAMS[1], 'float64')
    real = [np.empty(B * V) for _ in range(4)]
    ints = [np.empty(B, np.int32) for _ in range(6)]
    ip = [a.ctypes.data_as(P32) for a in ints]
    nul = ctypes.POINTER(ctypes.c_int32)()

    def soft(soft=0, dtype=_lib.F64, legs=6, iters0=12, alpha=0.75, pred=real[0].ctypes.data,
             ehat=real[2].ctypes.data, batch=B, xp=x.ctypes.data):
        return lib.gnnd_relay_soft_host(vp, cp, var.size, V, C, dtype, xp, gm.ctypes.data, legs,
                                        iters0, 12, 1, alpha, 0.0, soft, pred,
                                        real[1].ctypes.data, ehat, real[3].ctypes.data, *ip[:4],
                                        batch)

    def both(soft=0, base=0, method=1, order=10, dtype=_lib.F64, iters0=12, pred=real[0].ctypes.data,
             llr=real[1].ctypes.data, rst=ip[1], ehat=real[2].ctypes.data, status=ip[4],
             choice=ip[5], batch=B):
        return lib.gnnd_relay_osd_host(vp, cp, var.size, V, C, dtype, x.ctypes.data,
                                       gm.ctypes.data, 6, iters0, 12, 1, 0.75, 0.0, soft, base,
                                       method, order, pred, llr, ip[0], rst, ip[2], ip[3], ehat,
                                       status, choice, batch)

    assert soft() == _lib.OK and both() == _lib.OK
    for kw in ({'soft': 2}, {'soft': -1}, {'legs': 0}, {'iters0': 0}, {'alpha': 0.0}, {'pred': None},
               {'ehat': None}, {'xp': None}, {'batch': -1}, {'dtype': 7}):
        assert soft(**kw) == _lib.ERR_INVALID_ARG, kw
    assert soft(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    for kw in ({'soft': 2}, {'base': 2}, {'method': 3}, {'order': -1}, {'order': 65}, {'iters0': 0},
               {'pred': None}, {'llr': None}, {'rst': nul}, {'ehat': None}, {'status': nul},
               {'batch': -1}, {'dtype': 7}):
        assert both(**kw) == _lib.ERR_INVALID_ARG, kw
    assert both(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    # batch 0 returns OK whatever the pointers; a bad soft mode is still refused
    assert soft(batch=0, pred=None, ehat=None) == _lib.OK and soft(batch=0, soft=2) != _lib.OK
    assert both(batch=0, pred=None, ehat=None) == _lib.OK and both(batch=0, soft=2) != _lib.OK
    # optional outputs NULL: the required ones are the bits of the full call
    full = ops.relay_osd_host(H, x, gm, 12, 12, 1, soft='mean')
    e2, p2, l2 = (np.empty(B * V) for _ in range(3))
    st = lib.gnnd_relay_osd_host(vp, cp, var.size, V, C, _lib.F64, x.ctypes.data, gm.ctypes.data, 6,
                                 12, 12, 1, 0.75, 0.0, 1, 0, 1, 10, p2.ctypes.data, l2.ctypes.data,
                                 nul, ip[1], nul, nul, e2.ctypes.data, ip[4], nul, B)
    assert st == _lib.OK
    assert np.array_equal(e2, full[0]) and np.array_equal(p2, full[3])
    assert np.array_equal(l2, full[4]) and np.array_equal(ints[1], full[6])
    assert np.array_equal(ints[4], full[1])
    # the device entry points refuse the same arguments before touching a device: no graph needed
    assert lib.gnnd_relay_soft(None, _lib.F64, None, None, 6, 12, 12, 1, 0.75, 0.0, 0, None, None,
                               None, None, None, None, None, None, B, None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_relay_osd(None, _lib.F64, None, None, 6, 12, 12, 1, 0.75, 0.0, 0, 0, 1, 10,
                              None, None, None, None, None, None, None, None, None, None, 0, B,
                              None) == _lib.ERR_INVALID_ARG
    # the Python forms
    for kw in ({'soft': 'median'}, {'iters0': 0}, {'alpha': 0.0}, {'stop_after': 0}):
        args = dict(iters0=12)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.relay_soft_host(H, x, gm, **args)
        with pytest.raises(ValueError):
            ops.relay_osd_host(H, x, gm, **args)
    with pytest.raises(ValueError):
        ops.relay_osd_host(H, x, gm, 12, method='cs', order=65)
    with pytest.raises(ValueError):
        ops.relay_osd_host(H, x, gm[:, :-1], 12)
    with pytest.raises(TypeError):
        ops.relay_soft_host(H, x.astype(np.float16), gm, 12)
    out = ops.relay_osd_host(H, x[:0], gm, 12)
    assert len(out) == 9 and all(a.size == 0 for a in out)
    out = ops.relay_soft_host(H, x[:0], gm, 12)
    assert len(out) == 8 and all(a.size == 0 for a in out)
