"""Min-sum BP, host mirror (gnnd_minsum_host through ops.minsum_host) against the numpy statement
of the definition (tests/minsum_cases.py): bit-for-bit llr, iteration counts and statuses on every
shipped code in both dtypes, every parameter set on toric-5; the soft output within the project's
soft-output tolerance; status against the syndrome recomputed from llr; the argument checks of
both entry points (before any device call).  CPU only."""
import ctypes

import numpy as np
import pytest

from gnndecode import _lib, ops

import minsum_cases as mc

# every parameter set on toric-5, the first one elsewhere (LDPC at B = 3: the numpy loop is slow)
CASES = ([('toric_5', 5, p) for p in mc.PARAMS]
         + [('toric_7', 9, mc.PARAMS[0]), ('bch_63_45', 33, mc.PARAMS[2]),
            ('ldpc_648_324', 3, mc.PARAMS[0])])


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B,params', CASES)
def test_host_mirror_equals_reference(code, B, params, dtype):
    alpha, beta, iters, early_stop = params
    H, x = mc.inputs(code, B, dtype)
    ref_llr, ref_it, ref_st = mc.reference(code, B, dtype, params)
    pred, llr, its, status = ops.minsum_host(H, x, iters, alpha, beta, bool(early_stop))
    assert llr.dtype == x.dtype and pred.dtype == x.dtype
    assert its.dtype == np.int32 and status.dtype == np.int32
    assert np.array_equal(its, ref_it)
    assert np.array_equal(status, ref_st)
    assert np.array_equal(llr, ref_llr)
    assert np.array_equal(np.signbit(llr), np.signbit(ref_llr))      # -0.0 and 0.0 told apart
    np.testing.assert_allclose(pred, mc.soft_output(ref_llr), **mc.pred_tolerance(dtype))
    # status 0 iff the hard decision of the returned llr satisfies the syndrome
    assert np.array_equal(status == 0, mc.satisfied(H, x, llr))
    assert ((its >= 1) & (its <= iters)).all()
    if not early_stop:
        assert (its == iters).all()


def test_issue_inputs_reach_several_depths():
    """The inputs hold early exits at several depths and codewords that never converge."""
    _, its, st = mc.reference('toric_5', 40, 'float64', mc.PARAMS[0])
    pairs = set(zip(its.tolist(), st.tolist()))
    assert (12, 1) in pairs and len({i for i, s in pairs if s == 0}) >= 3, pairs
    _, its, st = mc.reference('bch_63_45', 20, 'float64', mc.PARAMS[2])
    pairs = set(zip(its.tolist(), st.tolist()))
    assert (10, 1) in pairs and len({i for i, s in pairs if s == 0}) >= 2, pairs


def test_ties_for_the_minimum_see_the_minimum():
    """One check over three variables, two of them tying for the smallest |q|: each of the two
    receives the other's magnitude (the minimum), the third receives it as well; signs by parity."""
    H = np.ones((3, 1), np.uint8)
    x = np.array([1.0, -1.0, 4.0, 1.0])                    # t = 0
    pred, llr, its, st = ops.minsum_host(H, x, 1, 1.0, 0.0, False)
    # r = (-1, +1, -1): L = l + r, no negative L and t = 0
    assert llr.tolist() == [0.0, 0.0, 3.0] and its.tolist() == [1] and st.tolist() == [0]
    x = np.array([1.0, -1.0, 4.0, -1.0])                   # t = 1 flips every sign
    pred, llr, its, st = ops.minsum_host(H, x, 1, 1.0, 0.0, False)
    assert llr.tolist() == [2.0, -2.0, 5.0] and st.tolist() == [0]
    # offset larger than the scaled minimum clamps the magnitude to +0: L = l, -0.0 is not negative
    x = np.array([1.0, -0.0, 4.0, 1.0])
    pred, llr, its, st = ops.minsum_host(H, x, 2, 0.5, 3.0, True)
    assert llr.tolist() == [1.0, 0.0, 4.0] and its.tolist() == [1] and st.tolist() == [0]
    assert pred.tolist() == pytest.approx([1 / (1 + np.e), 0.5, 1 / (1 + np.exp(4.0))])


def _degree_one_graph():
    """V = 3, C = 2: check 1 has the single edge (2, 1)."""
    return np.array([0, 1, 2, 2], np.int64), np.array([0, 0, 0, 1], np.int64)


def test_argument_checks_before_any_device_call():
    lib = _lib.get()
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    v = np.array([0, 1], np.int64)
    c = np.array([0, 0], np.int64)
    x = np.zeros(3)
    o = np.zeros(2)
    L = np.zeros(2)
    it = np.zeros(1, np.int32)
    s = np.zeros(1, np.int32)
    vp, cp = v.ctypes.data_as(P64), c.ctypes.data_as(P64)
    itp, sp = it.ctypes.data_as(P32), s.ctypes.data_as(P32)

    def host(dtype=_lib.F64, alpha=0.75, beta=0.0, iters=5, early=1, batch=1, xp=x.ctypes.data,
             op=o.ctypes.data, lp=L.ctypes.data, ip=itp, stp=sp, var=vp, chk=cp, E=2, V=2, C=1):
        return lib.gnnd_minsum_host(var, chk, E, V, C, dtype, xp, alpha, beta, iters, early, op, lp,
                                    ip, stp, batch)

    assert host() == _lib.OK
    assert host(dtype=_lib.F32) == _lib.OK
    assert host(lp=None, ip=None, stp=None) == _lib.OK              # the optional outputs
    assert host(alpha=1.0) == _lib.OK and host(beta=2.5) == _lib.OK
    assert host(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert host(dtype=7) == _lib.ERR_INVALID_ARG
    bad_params = ({'iters': 0}, {'iters': -3}, {'alpha': 0.0}, {'alpha': 1.5}, {'alpha': -0.5},
                  {'alpha': float('nan')}, {'alpha': float('inf')}, {'beta': -0.1},
                  {'beta': float('nan')}, {'beta': float('inf')}, {'early': 2}, {'batch': -1})
    for kw in bad_params:
        assert host(**kw) == _lib.ERR_INVALID_ARG, kw
    assert host(batch=0, xp=None, op=None, lp=None, ip=None, stp=None) == _lib.OK
    for kw in ({'xp': None}, {'op': None}, {'var': None}, {'chk': None}):
        assert host(**kw) == _lib.ERR_INVALID_ARG, kw
    bad = np.array([0, 2], np.int64)                       # variable id outside [0, V)
    assert host(var=bad.ctypes.data_as(P64)) == _lib.ERR_GRAPH
    unsorted = np.array([1, 0], np.int64)                  # not sorted by (v, c)
    assert host(var=unsorted.ctypes.data_as(P64)) == _lib.ERR_GRAPH
    dv, dc = _degree_one_graph()                           # a check of degree 1
    x5 = np.zeros(5)
    o3 = np.zeros(3)
    assert host(var=dv.ctypes.data_as(P64), chk=dc.ctypes.data_as(P64), E=4, V=3, C=2,
                xp=x5.ctypes.data, op=o3.ctypes.data, lp=None) == _lib.ERR_UNSUPPORTED

    # the device entry point rejects these before it touches a device (no graph exists here, so
    # a fake non-null handle stands in: it is never dereferenced on these paths)
    g = ctypes.c_void_p(8)
    d = ctypes.c_void_p(8)

    def dev(graph=g, dtype=_lib.F64, alpha=0.75, beta=0.0, iters=5, early=1, batch=1, xp=d, op=d):
        return lib.gnnd_minsum(graph, dtype, xp, alpha, beta, iters, early, op, d, d, d, batch, None)

    assert dev(graph=None) == _lib.ERR_INVALID_ARG
    for kw in bad_params:
        assert dev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert dev(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert dev(dtype=7) == _lib.ERR_INVALID_ARG
    assert dev(op=None) == _lib.ERR_INVALID_ARG            # d_out is required
    assert dev(xp=None) == _lib.ERR_INVALID_ARG
    assert dev(batch=0, xp=None, op=None) == _lib.OK       # nothing launched


def test_wrapper_rejects_bad_inputs():
    H = mc.code_matrix('bch_63_45')
    x = np.zeros(81)
    for kw in ({'iters': 0}, {'iters': 2.0}, {'alpha': 0.0}, {'alpha': 1.5}, {'alpha': float('nan')},
               {'beta': -1.0}, {'beta': float('inf')}):
        args = dict(iters=5, alpha=0.75, beta=0.0)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.minsum_host(H, x, args['iters'], args['alpha'], args['beta'], True)
    with pytest.raises(ValueError):
        ops.minsum_host(H, np.zeros(80), 5)
    with pytest.raises(TypeError):
        ops.minsum_host(H, np.zeros(81, np.float16), 5)
    dv, dc = _degree_one_graph()
    Hd = np.zeros((3, 2), np.uint8)
    Hd[dv, dc] = 1
    with pytest.raises(_lib.GnndError) as e:
        ops.minsum_host(Hd, np.zeros(5), 5)
    assert e.value.status == _lib.ERR_UNSUPPORTED
