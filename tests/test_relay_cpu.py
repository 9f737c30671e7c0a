"""Relay min-sum BP, host mirror (gnnd_relay_host through ops.relay_host) against the numpy
statement of the definition (tests/relay_cases.py): every output bit for bit on toric-5 and
BCH(63,45) in both dtypes, the one-leg zero-gamma case against the min-sum mirror, the gamma
tables, the argument checks of both entry points (before any device call), and status 0 implying
a satisfied syndrome.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch

from gnndecode import _lib, ops

import minsum_cases as mc
import relay_cases as rc

# (family, code, B, params)
CASES = ([('plain', 'toric_5', B, p) for B in (5, 67) for p in (rc.PARAMS[0], rc.PARAMS[1],
                                                                 rc.PARAMS[3])]
         + [('hard', 'toric_5', 67, rc.PARAMS[2]), ('plain', 'bch_63_45', 33, rc.PARAMS[0]),
            ('plain', 'bch_63_45', 33, rc.PARAMS[1])])


def host(family, code, B, dtype, params):
    legs, iters0, iters_leg, S = params
    H, x = rc.inputs(family, code, B, dtype)
    return ops.relay_host(H, x, rc.gammas(H.shape[0], params, dtype), iters0, iters_leg, S,
                          rc.ALPHA, rc.BETA)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('family,code,B,params', CASES)
def test_host_mirror_equals_reference(family, code, B, params, dtype):
    ref = rc.reference(family, code, B, dtype, params)
    got = host(family, code, B, dtype, params)
    rc.assert_equal(got, ref, (family, code, B, dtype, params))
    # status 0 implies H^T ehat == t, and ehat is the hard decision of llr
    H, x = rc.inputs(family, code, B, dtype)
    ehat, llr, its, status, leg, nsol = got
    assert set(np.unique(ehat).tolist()) <= {0.0, 1.0}
    assert np.array_equal(ehat, (llr < 0).astype(ehat.dtype))
    assert np.array_equal(status == 0, rc.satisfied(H, x, llr))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B', [('toric_5', 67), ('bch_63_45', 33)])
def test_one_leg_zero_gamma_is_minsum(code, B, dtype):
    """legs = 1, gamma = 0: llr, iters and status are minsum_host(early_stop=True)'s bits, on the
    BCH inputs with their -0.0 priors too."""
    H, x = mc.inputs(code, B, dtype)
    V = H.shape[0]
    assert code != 'bch_63_45' or (np.signbit(x) & (x == 0)).any()
    ehat, llr, its, status, leg, nsol = ops.relay_host(H, x, np.zeros((1, V)), 12)
    _, m_llr, m_its, m_st = ops.minsum_host(H, x, 12, early_stop=True)
    assert np.array_equal(llr, m_llr) and np.array_equal(np.signbit(llr), np.signbit(m_llr))
    assert np.array_equal(its, m_its) and np.array_equal(status, m_st)
    assert np.array_equal(leg, np.where(m_st == 0, 0, -1)) and np.array_equal(nsol, 1 - m_st)
    assert set(m_st.tolist()) == {0, 1}


def test_relay_gammas_is_deterministic_with_a_constant_first_row():
    a = ops.relay_gammas(100, 6, seed=3)
    b = ops.relay_gammas(100, 6, seed=3)
    assert a.shape == (6, 100) and a.dtype == torch.float64 and torch.equal(a, b)
    assert (a[0] == 0.125).all()
    want = np.random.default_rng(3).uniform(0.21 - 0.45, 0.21 + 0.45, (5, 100))
    assert np.array_equal(a[1:].numpy(), want)
    assert not torch.equal(a, ops.relay_gammas(100, 6, seed=4))
    f = ops.relay_gammas(100, 3, gamma0=0.25, center=0.0, width=0.5, seed=1, dtype=torch.float32)
    assert f.dtype == torch.float32 and (f[0] == 0.25).all()
    assert float(f[1:].min()) >= -0.25 and float(f[1:].max()) <= 0.25
    assert np.array_equal(f[1:].numpy(),
                          np.random.default_rng(1).uniform(-0.25, 0.25, (2, 100)).astype(np.float32))
    assert ops.relay_gammas(7, 1).shape == (1, 7)
    with pytest.raises(ValueError):
        ops.relay_gammas(7, 0)


def test_argument_checks_before_any_device_call():
    lib = _lib.get()
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    v = np.array([0, 1], np.int64)
    c = np.array([0, 0], np.int64)
    x = np.zeros(3)
    gm = np.zeros(4)
    o = np.zeros(2)
    L = np.zeros(2)
    ints = [np.zeros(1, np.int32) for _ in range(4)]
    vp, cp = v.ctypes.data_as(P64), c.ctypes.data_as(P64)
    ip = [a.ctypes.data_as(P32) for a in ints]

    def host(dtype=_lib.F64, alpha=0.75, beta=0.0, legs=2, iters0=3, iters_leg=2, S=1, batch=1,
             xp=x.ctypes.data, gp=gm.ctypes.data, op=o.ctypes.data, lp=L.ctypes.data, ips=ip,
             var=vp, chk=cp, E=2, V=2, C=1):
        return lib.gnnd_relay_host(var, chk, E, V, C, dtype, xp, gp, legs, iters0, iters_leg, S,
                                   alpha, beta, op, lp, *ips, batch)

    assert host() == _lib.OK
    assert host(dtype=_lib.F32) == _lib.OK
    assert host(lp=None, ips=[None] * 4) == _lib.OK                 # the optional outputs
    assert host(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert host(dtype=7) == _lib.ERR_INVALID_ARG
    bad_params = ({'legs': 0}, {'legs': -1}, {'iters0': 0}, {'iters_leg': 0}, {'iters_leg': -2},
                  {'S': 0}, {'legs': 3, 'iters_leg': 2 ** 30}, {'alpha': 0.0}, {'alpha': 1.5},
                  {'alpha': float('nan')}, {'beta': -0.1}, {'beta': float('inf')},
                  {'beta': float('nan')}, {'batch': -1})
    for kw in bad_params:
        assert host(**kw) == _lib.ERR_INVALID_ARG, kw
    assert host(batch=0, xp=None, gp=None, op=None, lp=None, ips=[None] * 4) == _lib.OK
    for kw in ({'xp': None}, {'gp': None}, {'op': None}, {'var': None}, {'chk': None}):
        assert host(**kw) == _lib.ERR_INVALID_ARG, kw
    bad = np.array([0, 2], np.int64)                       # variable id outside [0, V)
    assert host(var=bad.ctypes.data_as(P64)) == _lib.ERR_GRAPH
    unsorted = np.array([1, 0], np.int64)                  # not sorted by (v, c)
    assert host(var=unsorted.ctypes.data_as(P64)) == _lib.ERR_GRAPH
    dv = np.array([0, 1, 2, 2], np.int64)                  # check 1 has the single edge (2, 1)
    dc = np.array([0, 0, 0, 1], np.int64)
    x5, g6, o3 = np.zeros(5), np.zeros(6), np.zeros(3)
    assert host(var=dv.ctypes.data_as(P64), chk=dc.ctypes.data_as(P64), E=4, V=3, C=2,
                xp=x5.ctypes.data, gp=g6.ctypes.data, op=o3.ctypes.data,
                lp=None) == _lib.ERR_UNSUPPORTED

    # the device entry point rejects these before it touches a device (a fake non-null handle
    # stands in for the graph: it is never dereferenced on these paths)
    g = ctypes.c_void_p(8)
    d = ctypes.c_void_p(8)

    def dev(graph=g, dtype=_lib.F64, alpha=0.75, beta=0.0, legs=2, iters0=3, iters_leg=2, S=1,
            batch=1, xp=d, gp=d, op=d):
        return lib.gnnd_relay(graph, dtype, xp, gp, legs, iters0, iters_leg, S, alpha, beta, op, d,
                              d, d, d, d, batch, None)

    assert dev(graph=None) == _lib.ERR_INVALID_ARG
    for kw in bad_params:
        assert dev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert dev(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert dev(dtype=7) == _lib.ERR_INVALID_ARG
    for kw in ({'xp': None}, {'gp': None}, {'op': None}):
        assert dev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert dev(batch=0, xp=None, gp=None, op=None) == _lib.OK       # nothing launched


def test_wrapper_rejects_bad_inputs():
    H = mc.code_matrix('bch_63_45')
    x = np.zeros(81)
    g = np.zeros((2, 63))
    for kw in ({'iters0': 0}, {'iters0': 2.0}, {'iters_leg': 0}, {'stop_after': 0},
               {'alpha': 0.0}, {'alpha': 1.5}, {'alpha': float('nan')}, {'beta': -1.0},
               {'beta': float('inf')}):
        args = dict(iters0=5)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.relay_host(H, x, g, **args)
    with pytest.raises(ValueError):
        ops.relay_host(H, np.zeros(80), g, 5)
    with pytest.raises(ValueError):
        ops.relay_host(H, x, np.zeros((2, 62)), 5)
    with pytest.raises(ValueError):
        ops.relay_host(H, x, np.zeros((0, 63)), 5)
    with pytest.raises(TypeError):
        ops.relay_host(H, np.zeros(81, np.float16), g, 5)
    # iters_leg defaults to iters0
    H5, x5 = rc.inputs('plain', 'toric_5', 5, 'float64')
    g5 = rc.gammas(100, rc.PARAMS[1], 'float64')
    for a, b in zip(ops.relay_host(H5, x5, g5, 12), ops.relay_host(H5, x5, g5, 12, 12)):
        assert np.array_equal(a, b)
