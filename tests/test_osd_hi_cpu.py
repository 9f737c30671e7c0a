"""Higher-order OSD post-processing, host mirror (gnnd_osd_host through ops.osd_host) against the
numpy statement of the definition (tests/osd_hi_cases.py): exact equality of estimates, statuses
and chosen candidate indices on every shipped code, toric-7 and the rank-deficient graph, both
bases and dtypes, with OSD-0's inputs (ties, saturated entries, a NaN); that the reference's
choices cover the empty set, singles and pairs; global optimality against brute force on a small
random graph; the argument checks of both entry points.  CPU only."""
import ctypes
import functools

import numpy as np
import pytest

from gnndecode import _lib, ops

import osd_hi_cases as hc

SHAPES = [('toric_5', 67), ('toric_7', 9), ('bch_63_45', 33), ('ldpc_648_324', 3), ('bch_dup', 4)]


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('base', ['zero', 'hard'])
@pytest.mark.parametrize('code,B', SHAPES)
def test_host_mirror_equals_reference(code, B, base, dtype):
    H, x, p = hc.inputs(code, B, dtype)
    V = H.shape[0]
    e0, s0 = ops.osd0_host(H, x, p, base)
    cost0 = hc.cost(e0.reshape(B, V), p.reshape(B, V), base)
    for method, order in hc.METHODS:
        ref_e, ref_s, ref_c = hc.reference(code, B, dtype, base, method, order)
        ehat, status, choice = ops.osd_host(H, x, p, base, method, order)
        tag = (method, order)
        assert ehat.dtype == p.dtype and status.dtype == np.int32 and choice.dtype == np.int32
        assert np.isin(ehat, (0.0, 1.0)).all(), tag
        assert np.array_equal(status, ref_s), tag
        assert np.array_equal(choice, ref_c), tag
        assert np.array_equal(ehat.reshape(B, V), ref_e), tag
        assert np.array_equal(status, s0), tag
        assert not choice[status != 0].any(), tag
        assert hc.satisfied(H, x, ehat)[status == 0].all(), tag
        assert (hc.cost(ehat.reshape(B, V), p.reshape(B, V), base) <= cost0).all(), tag
        if method == 'osd0' or (method, order) == ('e', 0):
            assert np.array_equal(ehat, e0) and not choice.any(), tag
    if code == 'bch_dup':
        assert s0.tolist() == [1, 0] * (B // 2)
    else:
        assert not s0.any()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('base', ['zero', 'hard'])
@pytest.mark.parametrize('code,B,F', [('toric_5', 67, 52), ('bch_63_45', 33, 45)])
def test_order_above_free_count_is_clamped(code, B, F, base, dtype):
    """(cs, 64) with F < 64 free columns is (cs, F): the pairs stop at the free list's end."""
    assert set(hc.free_count(code, B, dtype, base)) == {F}
    H, x, p = hc.inputs(code, B, dtype)
    a = ops.osd_host(H, x, p, base, 'cs', 64)
    b = ops.osd_host(H, x, p, base, 'cs', F)
    ref = hc.reference(code, B, dtype, base, 'cs', F)
    for u, v, r in zip(a, b, ref):
        assert np.array_equal(u, v) and np.array_equal(u.reshape(r.shape), r)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('base', ['zero', 'hard'])
def test_reference_choices_cover_empty_single_and_pair(base, dtype):
    """The coverage the comparisons above rest on, asserted on the numpy reference itself:
    toric-5 B = 67 (cs, 10) picks the OSD-0 solution, a single and a pair, each at least once."""
    _, _, choice = hc.reference('toric_5', 67, dtype, base, 'cs', 10)
    F = 52
    n0 = int((choice == 0).sum())
    n1 = int(((choice >= 1) & (choice <= F)).sum())
    n2 = int((choice > F).sum())
    print(f'{base} {dtype}: empty {n0}, singles {n1}, pairs {n2}')
    assert n0 > 0 and n1 > 0 and n2 > 0
    assert int(choice.max()) <= F + 45


@functools.lru_cache(maxsize=None)
def _small_graph():
    """A seeded random H with V = 20, C = 12 and 8 <= F <= 12 free columns (F = V - rank), with
    all 2^V vectors and their syndromes."""
    for seed in range(100):
        rng = np.random.default_rng(seed)
        H = (rng.random((20, 12)) < 0.25).astype(np.uint8)
        if not H.any(axis=0).all() or not H.any(axis=1).all():
            continue
        F = 20 - hc.eliminate(H, np.zeros(12, np.uint8), rng.random(20), False)[3].size
        if 8 <= F <= 12:
            allv = ((np.arange(1 << 20)[:, None] >> np.arange(20)) & 1).astype(np.uint8)
            syn = ((allv.astype(np.int32) @ H.astype(np.int32)) % 2).astype(np.uint8)
            return H, F, allv, syn
    raise AssertionError('no seed gives 8 <= F <= 12')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('base', ['zero', 'hard'])
def test_exhaustive_is_globally_optimal_on_a_small_graph(base, dtype):
    """(e, 12) with lambda = F enumerates every solution: its cost is the minimum over all 2^F
    solutions of H^T e = t, picked out of all 2^20 vectors by their syndrome."""
    H, F, allv, syn = _small_graph()
    V, C = H.shape
    rng = np.random.default_rng([7, base == 'hard', dtype == 'float64'])
    B = 6
    p = rng.random((B, V)).astype(dtype)
    err = (rng.random((B, V)) < 0.3).astype(np.int64)
    t = (err @ H.astype(np.int64)) % 2                      # targets in the column space
    x = np.zeros((B, V + C), dtype)
    x[:, V:] = 1 - 2 * t
    ehat, status, choice = ops.osd_host(H, x.reshape(-1), p.reshape(-1), base, 'e', 12)
    assert not status.any()
    assert hc.satisfied(H, x.reshape(-1), ehat).all()
    ref_e, ref_s, ref_c = hc.ref_batch(H, x.reshape(-1), p.reshape(-1), base == 'hard', 'e', 12)
    assert np.array_equal(ehat.reshape(B, V), ref_e) and np.array_equal(choice, ref_c)
    z = (p > 0.5) if base == 'hard' else np.zeros_like(p, bool)
    got = hc.cost(ehat.reshape(B, V), p, base)
    for b in range(B):
        sol = allv[(syn == t[b]).all(axis=1)]
        assert sol.shape[0] == 1 << F
        assert got[b] == (sol ^ z[b].astype(np.uint8)).sum(1).min()


def test_bad_arguments():
    lib = _lib.get()
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    v = np.array([0, 1], np.int64)
    c = np.array([0, 0], np.int64)
    x = np.zeros(3)
    p = np.zeros(2)
    e = np.zeros(2)
    s = np.zeros(1, np.int32)
    ch = np.zeros(1, np.int32)
    vp, cp = v.ctypes.data_as(P64), c.ctypes.data_as(P64)
    sp, chp = s.ctypes.data_as(P32), ch.ctypes.data_as(P32)

    def host(dtype=_lib.F64, base=0, method=1, order=10, batch=1, chp=chp, ep=e.ctypes.data):
        return lib.gnnd_osd_host(vp, cp, 2, 2, 1, dtype, x.ctypes.data, p.ctypes.data, base,
                                 method, order, ep, sp, chp, batch)

    g = ctypes.c_void_p(8)      # never dereferenced on these paths (as in test_osd_cpu.py)
    d = ctypes.c_void_p(8)

    def dev(dtype=_lib.F64, base=0, method=1, order=10, batch=1, g=g, chp=d, ep=d):
        return lib.gnnd_osd(g, dtype, d, d, base, method, order, ep, d, chp, batch, None)

    assert host() == _lib.OK and host(chp=None) == _lib.OK
    assert host(method=0, order=1000) == _lib.OK            # order ignored as a value for OSD-0
    assert host(method=1, order=64) == _lib.OK and host(method=2, order=12) == _lib.OK
    for f in (host, dev):
        for method in (0, 1, 2):
            assert f(method=method, order=-1) == _lib.ERR_INVALID_ARG, method
        assert f(method=1, order=65) == _lib.ERR_INVALID_ARG
        assert f(method=2, order=13) == _lib.ERR_INVALID_ARG
        assert f(method=3) == _lib.ERR_INVALID_ARG and f(method=-1) == _lib.ERR_INVALID_ARG
        assert f(base=2) == _lib.ERR_INVALID_ARG and f(base=-1) == _lib.ERR_INVALID_ARG
        assert f(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
        assert f(dtype=7) == _lib.ERR_INVALID_ARG
        assert f(batch=-1) == _lib.ERR_INVALID_ARG
        assert f(batch=0, ep=None, chp=None) == _lib.OK     # nothing to do, nothing launched
        assert f(ep=None) == _lib.ERR_INVALID_ARG
    assert dev(g=None) == _lib.ERR_INVALID_ARG


def test_wrapper_rejects_bad_inputs():
    H = hc.code_matrix('bch_63_45')
    x, p = np.zeros(81), np.zeros(63)
    for kw in ({'base': 'soft'}, {'method': 'osd1'}, {'order': -1}, {'method': 'cs', 'order': 65},
               {'method': 'e', 'order': 13}, {'order': 2.0}):
        with pytest.raises(ValueError):
            ops.osd_host(H, x, p, **kw)
    with pytest.raises(ValueError):
        ops.osd_host(H, np.zeros(80), p)
    with pytest.raises(TypeError):
        ops.osd_host(H, x, np.zeros(63, np.float16))
    assert _lib.OSD_METHOD == {'osd0': 0, 'cs': 1, 'e': 2}
