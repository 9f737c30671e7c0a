"""Layered-schedule min-sum BP, host side (gnnd_minsum_layered_host / gnnd_bposd_layered_host /
gnnd_graph_layers_host through gnndecode.ops) against the numpy statement of the definition
(tests/minsum_layered_cases.py): bit-for-bit llr, iteration counts and statuses on every shipped
code in both dtypes, every parameter set on toric-5; the layer rule and the layer sizes; the
disjointness property the kernel relies on (any order, or all-read-then-all-write, inside a layer
gives the serial statement's bits) and its guard (a sweep that ignores the layers does not);
schedule='flooding' unchanged; the argument checks of every new entry point before any device
call.  CPU only."""
import ctypes

import numpy as np
import pytest

from gnndecode import _lib, ops

import minsum_cases as mc
import minsum_layered_cases as lc

CASES = ([('toric_5', 67, p) for p in lc.PARAMS]
         + [(code, B, p) for code, B in lc.SHAPES[1:] for p in lc.COMMON_PARAMS])


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B,params', CASES)
def test_host_mirror_equals_reference(code, B, params, dtype):
    alpha, beta, iters, early_stop = params
    H, x = lc.inputs(code, B, dtype)
    ref_llr, ref_it, ref_st = lc.reference(code, B, dtype, params)
    pred, llr, its, status = ops.minsum_host(H, x, iters, alpha, beta, bool(early_stop),
                                             schedule='layered')
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


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B', lc.SHAPES)
def test_inputs_reach_several_depths(code, B, dtype):
    """Both statuses and at least three early-stop depths in every batch of the comparisons."""
    for params in lc.COMMON_PARAMS:
        _, its, st = lc.reference(code, B, dtype, params)
        assert set(st.tolist()) == {0, 1}
        assert len(set(its.tolist())) >= 3, (params, sorted(set(its.tolist())))


@pytest.mark.parametrize('code', lc.CODES)
def test_layers_equal_the_numpy_rule(code):
    H = lc.code_matrix(code)
    want = lc.layer_of_check(code)
    got = ops.layers_host(H)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.bincount(got).tolist() == lc.LAYER_SIZES[code]
    # two checks of one layer share no variable
    Hb = H.astype(np.int64)
    for k in range(int(got.max()) + 1):
        assert (Hb[:, got == k].sum(axis=1) <= 1).all()
    # the layered order is the ascending order exactly where the issue's table says so
    same = np.array_equal(lc.layered_order(code), np.arange(H.shape[1]))
    assert same == (not code.startswith('toric'))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B', [('toric_5', 67), ('toric_7', 9), ('ldpc_648_324', 5)])
def test_any_order_inside_a_layer_gives_the_same_bits(code, B, dtype):
    """The disjointness property: the checks of a layer touch disjoint L_v and r_e, so reversing
    or shuffling them, or letting them all read before any writes (the kernel's lanes), gives the
    bits of the serial statement."""
    params = lc.PARAMS[0]
    ref = lc.reference(code, B, dtype, params)
    for how in ('reversed', 'shuffled', 'parallel'):
        got = lc.variant(code, B, dtype, params, how)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), how
        assert np.array_equal(np.signbit(got[0]), np.signbit(ref[0])), how


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_layered_order_differs_from_an_ascending_sweep_on_toric_5(dtype):
    """A mirror that ignored the layers and swept the checks in ascending c would not pass: on
    toric-5 that sweep gives other bits."""
    params = lc.PARAMS[0]
    ref = lc.reference('toric_5', 67, dtype, params)
    asc = lc.variant('toric_5', 67, dtype, params, 'ascending')
    assert not np.array_equal(asc[0], ref[0])
    H, x = lc.inputs('toric_5', 67, dtype)
    host = ops.minsum_host(H, x, params[2], params[0], params[1], True, schedule='layered')
    assert np.array_equal(host[1], ref[0]) and not np.array_equal(host[1], asc[0])


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_flooding_schedule_is_unchanged(dtype):
    alpha, beta, iters, early = lc.PARAMS[0]
    H, x = lc.inputs('toric_5', 67, dtype)
    old = ops.minsum_host(H, x, iters, alpha, beta, bool(early))
    new = ops.minsum_host(H, x, iters, alpha, beta, bool(early), schedule='flooding')
    ref_llr, ref_it, ref_st = mc.reference('toric_5', 67, dtype, lc.PARAMS[0])
    for a, b in zip(old, new):
        assert np.array_equal(a, b)
    assert np.array_equal(new[1], ref_llr) and np.array_equal(new[2], ref_it)
    lay = ops.minsum_host(H, x, iters, alpha, beta, bool(early), schedule='layered')
    assert not np.array_equal(lay[1], new[1])               # the schedules are different decoders
    old = ops.bposd_host(H, x, iters, alpha, beta, bool(early))
    new = ops.bposd_host(H, x, iters, alpha, beta, bool(early), schedule='flooding')
    for a, b in zip(old, new):
        assert np.array_equal(a, b)
    for fn in (ops.minsum_host, ops.bposd_host):
        with pytest.raises(ValueError):
            fn(H, x, iters, schedule='serial')


@pytest.mark.parametrize('code,B,dtype', [('toric_5', 67, 'float64'), ('toric_5', 67, 'float32'),
                                          ('bch_63_45', 9, 'float32'),
                                          ('ldpc_648_324', 5, 'float64')])
def test_bposd_layered_host_is_its_two_stages(code, B, dtype):
    alpha, beta, iters, early = lc.PARAMS[2] if code.startswith('bch') else lc.PARAMS[0]
    base = 'zero' if code.startswith('toric') else 'hard'
    H, x = lc.inputs(code, B, dtype)
    ehat, status, choice, its, bp, pred, llr = ops.bposd_host(
        H, x, iters, alpha, beta, bool(early), base, 'cs', 10, schedule='layered')
    m_pred, m_llr, m_its, m_st = ops.minsum_host(H, x, iters, alpha, beta, bool(early),
                                                 schedule='layered')
    ref_llr, ref_it, ref_st = lc.reference(code, B, dtype, (alpha, beta, iters, early))
    assert np.array_equal(llr, m_llr) and np.array_equal(llr, ref_llr)
    assert np.array_equal(its, m_its) and np.array_equal(bp, m_st) and np.array_equal(bp, ref_st)
    np.testing.assert_allclose(pred, m_pred, **mc.pred_tolerance(dtype))
    g_ehat, g_status, g_choice = ops.osd_gated_host(H, x, pred, bp, base, 'cs', 10, llr=llr)
    assert np.array_equal(ehat, g_ehat) and np.array_equal(status, g_status)
    assert np.array_equal(choice, g_choice)
    assert set(bp.tolist()) == {0, 1} and (choice[bp == 0] == -1).all()
    from osd_cases import satisfied
    assert satisfied(H, x, ehat)[status == 0].all()


def _degree_one_graph():
    """V = 3, C = 2: check 1 has the single edge (2, 1)."""
    return np.array([0, 1, 2, 2], np.int64), np.array([0, 0, 0, 1], np.int64)


def test_argument_checks_before_any_device_call():
    lib = _lib.get()
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    v = np.array([0, 1], np.int64)
    c = np.array([0, 0], np.int64)
    x = np.zeros(3)
    o, L, e = np.zeros(2), np.zeros(2), np.zeros(2)
    it, s, s2, ch = (np.zeros(1, np.int32) for _ in range(4))
    vp, cp = v.ctypes.data_as(P64), c.ctypes.data_as(P64)
    i32 = lambda a: a.ctypes.data_as(P32)

    def host(dtype=_lib.F64, alpha=0.75, beta=0.0, iters=5, early=1, batch=1, xp=x.ctypes.data,
             op=o.ctypes.data, lp=L.ctypes.data, ip=i32(it), stp=i32(s), var=vp, chk=cp, E=2, V=2,
             C=1):
        return lib.gnnd_minsum_layered_host(var, chk, E, V, C, dtype, xp, alpha, beta, iters, early,
                                            op, lp, ip, stp, batch)

    def bhost(dtype=_lib.F64, alpha=0.75, beta=0.0, iters=5, early=1, batch=1, xp=x.ctypes.data,
              op=o.ctypes.data, lp=L.ctypes.data, ip=i32(it), stp=i32(s), var=vp, chk=cp,
              base=0, method=1, order=10, ep=e.ctypes.data, sp=i32(s2), chp=i32(ch)):
        return lib.gnnd_bposd_layered_host(var, chk, 2, 2, 1, dtype, xp, alpha, beta, iters, early,
                                           base, method, order, op, lp, ip, stp, ep, sp, chp, batch)

    assert host() == _lib.OK and host(dtype=_lib.F32) == _lib.OK
    assert host(lp=None, ip=None, stp=None) == _lib.OK              # the optional outputs
    assert bhost() == _lib.OK and bhost(ip=None, chp=None) == _lib.OK
    bad_params = ({'iters': 0}, {'iters': -3}, {'alpha': 0.0}, {'alpha': 1.5}, {'alpha': -0.5},
                  {'alpha': float('nan')}, {'alpha': float('inf')}, {'beta': -0.1},
                  {'beta': float('nan')}, {'beta': float('inf')}, {'early': 2}, {'batch': -1})
    bad_osd = ({'base': 2}, {'method': 3}, {'order': -1}, {'method': 1, 'order': 65},
               {'method': 2, 'order': 13})
    for fn in (host, bhost):
        assert fn(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
        assert fn(dtype=7) == _lib.ERR_INVALID_ARG
        for kw in bad_params:
            assert fn(**kw) == _lib.ERR_INVALID_ARG, kw
        for kw in ({'xp': None}, {'op': None}, {'var': None}, {'chk': None}):
            assert fn(**kw) == _lib.ERR_INVALID_ARG, kw
    assert host(batch=0, xp=None, op=None, lp=None, ip=None, stp=None) == _lib.OK
    assert bhost(batch=0, xp=None, op=None, lp=None, stp=None, ep=None, sp=None) == _lib.OK
    for kw in bad_osd + ({'lp': None}, {'stp': None}, {'ep': None}, {'sp': None}):
        assert bhost(**kw) == _lib.ERR_INVALID_ARG, kw
    bad = np.array([0, 2], np.int64)                       # variable id outside [0, V)
    assert host(var=bad.ctypes.data_as(P64)) == _lib.ERR_GRAPH
    unsorted = np.array([1, 0], np.int64)                  # not sorted by (v, c)
    assert host(var=unsorted.ctypes.data_as(P64)) == _lib.ERR_GRAPH
    dv, dc = _degree_one_graph()                           # a check of degree 1
    x5, o3 = np.zeros(5), np.zeros(3)
    assert host(var=dv.ctypes.data_as(P64), chk=dc.ctypes.data_as(P64), E=4, V=3, C=2,
                xp=x5.ctypes.data, op=o3.ctypes.data, lp=None) == _lib.ERR_UNSUPPORTED

    # gnnd_graph_layers_host
    n = ctypes.c_int32()
    lay = np.zeros(2, np.int32)
    assert lib.gnnd_graph_layers_host(vp, cp, 2, 2, 1, ctypes.byref(n), i32(lay)) == _lib.OK
    assert n.value == 1 and lay[0] == 0
    assert lib.gnnd_graph_layers_host(vp, cp, 2, 2, 1, ctypes.byref(n), None) == _lib.OK
    assert lib.gnnd_graph_layers_host(None, cp, 2, 2, 1, ctypes.byref(n), None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_graph_layers_host(vp, cp, 2, 2, 1, None, None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_graph_layers_host(bad.ctypes.data_as(P64), cp, 2, 2, 1, ctypes.byref(n),
                                      None) == _lib.ERR_GRAPH
    assert lib.gnnd_graph_layers_host(dv.ctypes.data_as(P64), dc.ctypes.data_as(P64), 4, 3, 2,
                                      ctypes.byref(n), i32(lay)) == _lib.OK
    assert n.value == 2 and lay.tolist() == [0, 1]         # the two checks share variable 2

    # the device entry points reject these before they touch a device (no graph exists here, so
    # a fake non-null handle stands in: it is never dereferenced on these paths)
    g = ctypes.c_void_p(8)
    d = ctypes.c_void_p(8)

    def dev(graph=g, dtype=_lib.F64, alpha=0.75, beta=0.0, iters=5, early=1, batch=1, xp=d, op=d):
        return lib.gnnd_minsum_layered(graph, dtype, xp, alpha, beta, iters, early, op, d, d, d,
                                       batch, None)

    def bdev(graph=g, dtype=_lib.F64, alpha=0.75, beta=0.0, iters=5, early=1, batch=1, xp=d, op=d,
             base=0, method=1, order=10, lp=d, stp=d, ep=d, sp=d, wp=d, wbytes=8):
        return lib.gnnd_bposd_layered(graph, dtype, xp, alpha, beta, iters, early, base, method,
                                      order, op, lp, d, stp, ep, sp, d, wp, wbytes, batch, None)

    for fn in (dev, bdev):
        assert fn(graph=None) == _lib.ERR_INVALID_ARG
        for kw in bad_params:
            assert fn(**kw) == _lib.ERR_INVALID_ARG, kw
        assert fn(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
        assert fn(dtype=7) == _lib.ERR_INVALID_ARG
        assert fn(op=None) == _lib.ERR_INVALID_ARG
        assert fn(xp=None) == _lib.ERR_INVALID_ARG
        assert fn(batch=0, xp=None, op=None) == _lib.OK    # nothing launched
    for kw in bad_osd + ({'lp': None}, {'stp': None}, {'ep': None}, {'sp': None}, {'wp': None},
                         {'wbytes': 7}, {'batch': 3, 'wbytes': 15}):
        assert bdev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert bdev(batch=2 ** 31 - 1, wbytes=2 ** 40) == _lib.ERR_UNSUPPORTED
    p4 = (ctypes.c_int32 * 4)()
    assert lib.gnnd_graph_layers(None, ctypes.byref(n), None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_graph_layers(g, None, None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_minsum_layered_plan(None, _lib.F64, p4) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_minsum_layered_plan(g, _lib.F64, None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_minsum_layered_plan(g, _lib.BF16, p4) == _lib.ERR_UNSUPPORTED
    assert lib.gnnd_minsum_layered_plan(g, 7, p4) == _lib.ERR_INVALID_ARG
