"""Gated OSD and BP+OSD, host mirrors (gnnd_osd_gated_host / gnnd_bposd_host through
ops.osd_gated_host / ops.bposd_host) against the numpy statement (tests/bposd_cases.py), exact
equality: every shipped code in both dtypes and bases, three methods, four gates, the pass-through
decision from llr and from pred; the tiny-LLR case that llr exists for; the rank-deficient graph;
the argument checks of the four entry points (before any device call).  CPU only."""
import ctypes

import numpy as np
import pytest

from gnndecode import _lib, ops

import bposd_cases as bc
import minsum_cases as mc
import osd_cases as oc

P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)


def _same(got, ref, B, V):
    ehat, status, choice = got
    assert status.dtype == np.int32 and choice.dtype == np.int32
    assert np.array_equal(ehat.reshape(B, V), ref[0].astype(ehat.dtype))
    assert np.array_equal(status, ref[1]) and np.array_equal(choice, ref[2])


@pytest.mark.parametrize('method,order', bc.METHODS)
@pytest.mark.parametrize('base', ['zero', 'hard'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B', bc.SHAPES)
def test_gated_host_mirror_equals_reference(code, B, dtype, base, method, order):
    H, x, p = oc.inputs(code, B, dtype)
    V = H.shape[0]
    L = bc.llr_input(code, B, dtype)
    full = ops.osd_host(H, x, p, base, method, order)
    for name in bc.GATES:
        g = bc.gate(code, B, dtype, name)
        for llr in (L, None):
            got = ops.osd_gated_host(H, x, p, g, base, method, order, llr=llr)
            assert got[0].dtype == p.dtype
            _same(got, bc.gated_reference(code, B, dtype, base, method, order, name,
                                          llr is not None), B, V)
            if name == 'ones':                      # bit for bit the ungated mirror
                for a, b in zip(got, full):
                    assert np.array_equal(a, b)
            if name == 'zeros':
                assert (got[2] == -1).all() and (got[1] == 0).all()
                assert np.array_equal(got[0], bc.hard_decision(p, llr).astype(p.dtype))
    # the two hard decisions differ on these inputs, so the comparisons above tell them apart
    assert not np.array_equal(bc.hard_decision(p, L), bc.hard_decision(p, None))


@pytest.mark.parametrize('method,order', bc.METHODS)
@pytest.mark.parametrize('base', ['zero', 'hard'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B', bc.SHAPES)
def test_bposd_host_mirror_equals_reference(code, B, dtype, base, method, order):
    alpha, beta, iters, early = bc.bp_params(code)
    H, x = mc.inputs(code, B, dtype)
    V = H.shape[0]
    ehat, status, choice, its, bp, pred, llr = ops.bposd_host(H, x, iters, alpha, beta, bool(early),
                                                              base, method, order)
    r_e, r_s, r_c, r_it, r_bp, r_llr = bc.bposd_reference(code, B, dtype, pred, base, method, order)
    assert np.array_equal(llr, r_llr) and np.array_equal(np.signbit(llr), np.signbit(r_llr))
    assert np.array_equal(its, r_it) and np.array_equal(bp, r_bp)
    np.testing.assert_allclose(pred, mc.soft_output(r_llr), **mc.pred_tolerance(dtype))
    _same((ehat, status, choice), (r_e, r_s, r_c), B, V)
    # the two stages, called one after the other: min-sum's bit-exact outputs are the same bits;
    # pred is not among them (in fp64 bposd_host computes it with the kernel's exponential scheme,
    # minsum_host with the host library's), so the OSD stage is compared on bposd_host's pred
    m = ops.minsum_host(H, x, iters, alpha, beta, bool(early))
    assert all(np.array_equal(a, b) for a, b in zip(m[1:], (llr, its, bp)))
    np.testing.assert_allclose(m[0], pred, **mc.pred_tolerance(dtype))
    if dtype == 'float32':
        assert np.array_equal(m[0], pred)
    o = ops.osd_gated_host(H, x, pred, m[3], base, method, order, llr=m[1])
    assert all(np.array_equal(a, b) for a, b in zip(o, (ehat, status, choice)))
    # the guarantee: BP's own solutions are kept and satisfy the syndrome
    ok = bp == 0
    assert np.array_equal(ehat.reshape(B, V)[ok], (llr.reshape(B, V)[ok] < 0).astype(ehat.dtype))
    assert oc.satisfied(H, x, ehat)[ok].all() and (choice[ok] == -1).all()
    assert oc.satisfied(H, x, ehat)[status == 0].all()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_tiny_llr_needs_the_llr_argument(dtype):
    """Priors scaled by 2^-100: the same decoding, every pred exactly 0.5.  With llr the
    pass-through rows are min-sum's decision and satisfy the syndrome; from pred alone they are
    all zero."""
    alpha, beta, iters, early = bc.TINY_BP
    H, x, xs = bc.tiny_llr_inputs(dtype)
    V, C = H.shape
    B = x.size // (V + C)
    big = ops.minsum_host(H, x, iters, alpha, beta, True)
    ehat, status, choice, its, bp, pred, llr = ops.bposd_host(H, xs, iters, alpha, beta, True,
                                                              'zero', 'cs', 10)
    assert np.array_equal(its, big[2]) and np.array_equal(bp, big[3])
    assert np.array_equal(llr < 0, big[1] < 0)
    assert np.array_equal(llr, big[1] * np.dtype(dtype).type(2.0 ** -100))
    assert (pred == 0.5).all()
    ok = bp == 0
    assert ok.any() and (~ok).any()
    e = ehat.reshape(B, V)
    assert np.array_equal(e[ok], (llr.reshape(B, V)[ok] < 0).astype(e.dtype))
    assert e[ok].any()
    assert oc.satisfied(H, xs, ehat)[ok].all()
    assert oc.satisfied(H, xs, ehat)[status == 0].all()
    blind = ops.osd_gated_host(H, xs, pred, bp, 'zero', 'cs', 10, llr=None)
    assert not blind[0].reshape(B, V)[ok].any()
    assert not oc.satisfied(H, xs, blind[0])[ok].all()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('base', ['zero', 'hard'])
def test_rank_deficient_graph(base, dtype):
    """BCH(63,45) with check 0 repeated: the even codewords carry t_0 != t_18 and fail.  Gated,
    they report status 1 and ehat = z; ungated, they pass through whatever the syndrome."""
    B = 4
    H, x, p = oc.inputs('bch_dup', B, dtype)
    V = H.shape[0]
    pb = p.reshape(B, V)
    z = ((pb > 0.5) if base == 'hard' else np.zeros_like(pb, bool)).astype(p.dtype)
    g = np.array([1, 0, 1, 0], np.int32)                    # gates on the failing codewords
    for method, order in (('osd0', 0), ('cs', 10), ('e', 8)):
        ehat, status, choice = ops.osd_gated_host(H, x, p, g, base, method, order)
        assert status.tolist() == [1, 0, 1, 0] and choice.tolist() == [0, -1, 0, -1]
        assert np.array_equal(ehat.reshape(B, V)[0::2], z[0::2])
        assert np.array_equal(ehat.reshape(B, V)[1::2], (pb[1::2] > 0.5).astype(p.dtype))
        full = ops.osd_host(H, x, p, base, method, order)
        ehat, status, choice = ops.osd_gated_host(H, x, p, 1 - g, base, method, order)
        assert status.tolist() == [0, 0, 0, 0]
        assert np.array_equal(ehat.reshape(B, V)[1::2], full[0].reshape(B, V)[1::2])
        assert np.array_equal(choice[1::2], full[2][1::2])


def test_argument_checks_before_any_device_call():
    lib = _lib.get()
    n = ctypes.c_int64()
    assert lib.gnnd_osd_gated_workspace(0, ctypes.byref(n)) == _lib.OK and n.value == 4
    assert lib.gnnd_osd_gated_workspace(67, ctypes.byref(n)) == _lib.OK and n.value == 4 * 68
    assert lib.gnnd_osd_gated_workspace(-1, ctypes.byref(n)) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_osd_gated_workspace(5, None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_osd_gated_workspace(2 ** 31, ctypes.byref(n)) == _lib.ERR_UNSUPPORTED

    v = np.array([0, 1], np.int64)
    c = np.array([0, 0], np.int64)
    x = np.zeros(3)
    p = np.full(2, 0.25)
    L = np.zeros(2)
    e = np.zeros(2)
    gt = np.ones(1, np.int32)
    s, ch, it, bp = (np.zeros(1, np.int32) for _ in range(4))
    vp, cp = v.ctypes.data_as(P64), c.ctypes.data_as(P64)
    i32 = lambda a: a.ctypes.data_as(P32)

    def ghost(dtype=_lib.F64, base=0, method=1, order=10, batch=1, xp=x.ctypes.data,
              pp=p.ctypes.data, lp=L.ctypes.data, gp=i32(gt), ep=e.ctypes.data, sp=i32(s),
              cp_=i32(ch), var=vp, chk=cp):
        return lib.gnnd_osd_gated_host(var, chk, 2, 2, 1, dtype, xp, pp, lp, gp, base, method, order,
                                       ep, sp, cp_, batch)

    bad_osd = ({'base': 2}, {'base': -1}, {'method': 3}, {'method': -1}, {'order': -1},
               {'method': 1, 'order': 65}, {'method': 2, 'order': 13}, {'batch': -1}, {'dtype': 7})
    assert ghost() == _lib.OK
    assert ghost(dtype=_lib.F32) == _lib.OK
    assert ghost(lp=None, cp_=None) == _lib.OK                  # the optional arrays
    for kw in bad_osd:
        assert ghost(**kw) == _lib.ERR_INVALID_ARG, kw
    assert ghost(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert ghost(batch=0, xp=None, pp=None, gp=None, ep=None, sp=None) == _lib.OK
    for kw in ({'xp': None}, {'pp': None}, {'gp': None}, {'ep': None}, {'sp': None}, {'var': None},
               {'chk': None}):
        assert ghost(**kw) == _lib.ERR_INVALID_ARG, kw
    far = np.array([0, 2], np.int64)
    assert ghost(var=far.ctypes.data_as(P64)) == _lib.ERR_GRAPH

    def bhost(dtype=_lib.F64, alpha=0.75, beta=0.0, iters=5, early=1, base=0, method=1, order=10,
              batch=1, xp=x.ctypes.data, pp=p.ctypes.data, lp=L.ctypes.data, ip=i32(it), bpp=i32(bp),
              ep=e.ctypes.data, sp=i32(s), cp_=i32(ch), var=vp, chk=cp):
        return lib.gnnd_bposd_host(var, chk, 2, 2, 1, dtype, xp, alpha, beta, iters, early, base,
                                   method, order, pp, lp, ip, bpp, ep, sp, cp_, batch)

    bad_bp = ({'iters': 0}, {'alpha': 0.0}, {'alpha': 1.5}, {'alpha': float('nan')}, {'beta': -0.1},
              {'beta': float('inf')}, {'early': 2})
    assert bhost() == _lib.OK
    assert bhost(dtype=_lib.F32) == _lib.OK
    assert bhost(ip=None, cp_=None) == _lib.OK
    for kw in bad_osd + bad_bp:
        assert bhost(**kw) == _lib.ERR_INVALID_ARG, kw
    assert bhost(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert bhost(batch=0, xp=None, pp=None, lp=None, bpp=None, ep=None, sp=None) == _lib.OK
    for kw in ({'xp': None}, {'pp': None}, {'lp': None}, {'bpp': None}, {'ep': None}, {'sp': None},
               {'var': None}, {'chk': None}):
        assert bhost(**kw) == _lib.ERR_INVALID_ARG, kw
    assert bhost(var=far.ctypes.data_as(P64)) == _lib.ERR_GRAPH
    dv = np.array([0, 1, 2, 2], np.int64)                   # check 1 has degree 1: min-sum refuses
    dc = np.array([0, 0, 0, 1], np.int64)
    x5, p3, L3, e3 = np.zeros(5), np.zeros(3), np.zeros(3), np.zeros(3)
    assert lib.gnnd_bposd_host(dv.ctypes.data_as(P64), dc.ctypes.data_as(P64), 4, 3, 2, _lib.F64,
                               x5.ctypes.data, 0.75, 0.0, 5, 1, 0, 1, 10, p3.ctypes.data,
                               L3.ctypes.data, i32(it), i32(bp), e3.ctypes.data, i32(s),
                               i32(ch), 1) == _lib.ERR_UNSUPPORTED

    # the device entry points reject these before they touch a device (no graph exists here, so a
    # fake non-null handle stands in: it is never dereferenced on these paths)
    d = ctypes.c_void_p(8)

    def gdev(graph=d, dtype=_lib.F64, base=0, method=1, order=10, batch=1, xp=d, pp=d, gp=d, ep=d,
             sp=d, wp=d, wb=8):
        return lib.gnnd_osd_gated(graph, dtype, xp, pp, None, gp, base, method, order, ep, sp, None,
                                  wp, wb, batch, None)

    assert gdev(graph=None) == _lib.ERR_INVALID_ARG
    for kw in bad_osd:
        assert gdev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert gdev(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    for kw in ({'xp': None}, {'pp': None}, {'gp': None}, {'ep': None}, {'sp': None}, {'wp': None},
               {'wb': 7}, {'wb': 0}):
        assert gdev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert gdev(batch=0, xp=None, pp=None, gp=None, ep=None, sp=None, wp=None, wb=0) == _lib.OK

    def bdev(graph=d, dtype=_lib.F64, alpha=0.75, beta=0.0, iters=5, early=1, base=0, method=1,
             order=10, batch=1, xp=d, pp=d, lp=d, bpp=d, ep=d, sp=d, wp=d, wb=8):
        return lib.gnnd_bposd(graph, dtype, xp, alpha, beta, iters, early, base, method, order, pp,
                              lp, None, bpp, ep, sp, None, wp, wb, batch, None)

    assert bdev(graph=None) == _lib.ERR_INVALID_ARG
    for kw in bad_osd + bad_bp:
        assert bdev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert bdev(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    for kw in ({'xp': None}, {'pp': None}, {'lp': None}, {'bpp': None}, {'ep': None}, {'sp': None},
               {'wp': None}, {'wb': 7}):
        assert bdev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert bdev(batch=0, xp=None, pp=None, lp=None, bpp=None, ep=None, sp=None, wp=None,
                wb=0) == _lib.OK


def test_wrappers_reject_bad_inputs():
    H = mc.code_matrix('bch_63_45')
    x, p, g = np.zeros(81), np.zeros(63), np.zeros(1, np.int32)
    for kw in ({'base': 'soft'}, {'method': 'osd1'}, {'order': -1}, {'method': 'e', 'order': 13}):
        with pytest.raises(ValueError):
            ops.osd_gated_host(H, x, p, g, **kw)
        with pytest.raises(ValueError):
            ops.bposd_host(H, x, 5, **kw)
    for kw in ({'iters': 0}, {'alpha': 0.0}, {'beta': -1.0}):
        args = dict(iters=5)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.bposd_host(H, x, **args)
    with pytest.raises(ValueError):
        ops.osd_gated_host(H, x, p, np.zeros(2, np.int32))
    with pytest.raises(ValueError):
        ops.osd_gated_host(H, x, p, g, llr=np.zeros(62))
    with pytest.raises(ValueError):
        ops.bposd_host(H, np.zeros(80), 5)
    with pytest.raises(TypeError):
        ops.osd_gated_host(H, x, p.astype(np.float16), g)
    with pytest.raises(TypeError):
        ops.bposd_host(H, x.astype(np.float16), 5)
