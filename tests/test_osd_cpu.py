"""OSD-0 post-processing, host mirror (gnnd_osd0_host through ops.osd0_host) against the numpy
statement of the definition (tests/osd_cases.py): bit-for-bit estimates and statuses on every
shipped code, both bases and dtypes, with ties, saturated entries and a NaN; the rank-deficient
graph; the argument checks of both entry points (before any device call).  CPU only."""
import ctypes

import numpy as np
import pytest

from gnndecode import _lib, ops

import osd_cases as oc

B = 8


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('base', ['zero', 'hard'])
@pytest.mark.parametrize('code', oc.CODES)
def test_host_mirror_equals_reference(code, base, dtype):
    H, x, p = oc.inputs(code, B, dtype)
    ref_e, ref_s = oc.reference(code, B, dtype, base)
    ehat, status = ops.osd0_host(H, x, p, base)
    assert ehat.dtype == p.dtype and status.dtype == np.int32
    assert np.isin(ehat, (0.0, 1.0)).all()
    assert np.array_equal(status, ref_s)
    assert np.array_equal(ehat.reshape(B, -1), ref_e)
    # the shipped codes have full row rank: every syndrome is solvable, and solved
    assert not status.any()
    assert oc.satisfied(H, x, ehat).all()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('base', ['zero', 'hard'])
def test_rank_deficient_graph(base, dtype):
    """BCH(63,45) with check 0 repeated as check 18: t_0 != t_18 (even codewords) is outside
    the column space -> status 1 and ehat = z; t_0 == t_18 (odd codewords) -> status 0."""
    H, x, p = oc.inputs('bch_dup', B, dtype)
    V = H.shape[0]
    ehat, status = ops.osd0_host(H, x, p, base)
    ref_e, ref_s = oc.reference('bch_dup', B, dtype, base)
    assert np.array_equal(status, ref_s) and np.array_equal(ehat.reshape(B, V), ref_e)
    assert status.tolist() == [1, 0] * (B // 2)
    pb = p.reshape(B, V)
    z = (pb > 0.5) if base == 'hard' else np.zeros_like(pb, bool)
    assert np.array_equal(ehat.reshape(B, V)[0::2], z[0::2].astype(p.dtype))
    assert oc.satisfied(H, x, ehat)[1::2].all()


def test_tie_rule_is_ascending_variable():
    """Repetition-like check: one check over three variables with equal keys -> the pivot (the
    only flipped bit) is the smallest variable index; a larger key moves it."""
    H = np.ones((3, 1), np.uint8)
    x = np.array([0, 0, 0, -1.0])
    e, s = ops.osd0_host(H, x, np.array([0.4, 0.4, 0.4]), 'zero')
    assert s.tolist() == [0] and e.tolist() == [1, 0, 0]
    e, s = ops.osd0_host(H, x, np.array([0.4, 0.4, 0.5]), 'zero')
    assert e.tolist() == [0, 0, 1]
    e, s = ops.osd0_host(H, x, np.array([np.nan, 0.0, 0.0]), 'zero')     # NaN sorts last
    assert e.tolist() == [0, 1, 0]
    # hard base: z = (1, 0, 1) has even parity, the least reliable bit (nearest 0.5) is flipped
    e, s = ops.osd0_host(H, x, np.array([0.9, 0.2, 0.6]), 'hard')
    assert e.tolist() == [1, 0, 0]


def test_argument_checks_before_any_device_call():
    lib = _lib.get()
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    v = np.array([0, 1], np.int64)
    c = np.array([0, 0], np.int64)
    x = np.zeros(3)
    p = np.zeros(2)
    e = np.zeros(2)
    s = np.zeros(1, np.int32)
    vp, cp, sp = v.ctypes.data_as(P64), c.ctypes.data_as(P64), s.ctypes.data_as(P32)

    def host(dtype=_lib.F64, base=0, batch=1, xp=x.ctypes.data, pp=p.ctypes.data, ep=e.ctypes.data,
             stp=sp, var=vp):
        return lib.gnnd_osd0_host(var, cp, 2, 2, 1, dtype, xp, pp, base, ep, stp, batch)

    assert host() == _lib.OK
    assert host(dtype=_lib.F32) == _lib.OK
    assert host(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert host(dtype=7) == _lib.ERR_INVALID_ARG
    assert host(base=2) == _lib.ERR_INVALID_ARG and host(base=-1) == _lib.ERR_INVALID_ARG
    assert host(batch=-1) == _lib.ERR_INVALID_ARG
    assert host(batch=0, xp=None, pp=None, ep=None, stp=None) == _lib.OK
    for kw in ({'xp': None}, {'pp': None}, {'ep': None}, {'stp': None}, {'var': None}):
        assert host(**kw) == _lib.ERR_INVALID_ARG, kw
    bad = np.array([0, 2], np.int64)                  # variable id outside [0, V)
    assert host(var=bad.ctypes.data_as(P64)) == _lib.ERR_GRAPH

    # the device entry point rejects these before it touches a device (no graph exists here, so
    # a fake non-null handle stands in: it is never dereferenced on these paths)
    g = ctypes.c_void_p(8)
    d = ctypes.c_void_p(8)
    dev = lib.gnnd_osd0
    assert dev(None, _lib.F64, d, d, 0, d, d, 1, None) == _lib.ERR_INVALID_ARG
    assert dev(g, _lib.F64, d, d, 2, d, d, 1, None) == _lib.ERR_INVALID_ARG
    assert dev(g, _lib.F64, d, d, 0, d, d, -1, None) == _lib.ERR_INVALID_ARG
    assert dev(g, _lib.BF16, d, d, 0, d, d, 1, None) == _lib.ERR_UNSUPPORTED
    assert dev(g, 7, d, d, 0, d, d, 1, None) == _lib.ERR_INVALID_ARG
    assert dev(g, _lib.F32, None, None, 1, None, None, 0, None) == _lib.OK      # nothing launched
    for i in (2, 3, 5, 6):
        args = [g, _lib.F64, d, d, 0, d, d, 1, None]
        args[i] = None
        assert dev(*args) == _lib.ERR_INVALID_ARG, i


def test_wrapper_rejects_bad_inputs():
    H = oc.code_matrix('bch_63_45')
    with pytest.raises(ValueError):
        ops.osd0_host(H, np.zeros(81), np.zeros(63), 'soft')
    with pytest.raises(ValueError):
        ops.osd0_host(H, np.zeros(80), np.zeros(63), 'zero')
    with pytest.raises(TypeError):
        ops.osd0_host(H, np.zeros(81), np.zeros(63, np.float16), 'zero')
