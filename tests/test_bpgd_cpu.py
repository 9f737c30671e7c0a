"""Min-sum BP with guided decimation, host mirror (gnnd_bpgd_host through ops.bpgd_host) against
the numpy statement of the definition (tests/bpgd_cases.py): every contract output bit for bit on
toric-5, toric-7, BCH(63,45) and three synthetic graphs in both dtypes under every parameter set,
the rounds == 0 case against the min-sum mirror, the fp64 soft output against the fixed
exponential, the argument checks of both entry points (before any device call), batch 0, NULL
optional outputs, and status 0 implying a satisfied syndrome.  CPU only."""
import ctypes

import numpy as np
import pytest

from gnndecode import _lib, ops

import bpgd_cases as bc
import minsum_cases as mc

# (code, B)
SHAPES = (('toric_5', 9), ('toric_7', 9), ('bch_63_45', 5), ('syn_hub', 9), ('syn_wide', 9),
          ('syn_sq64', 9))


def host(code, B, dtype, pset):
    H, x = bc.inputs(code, B, dtype)
    iters0, iters_round, rounds, per_round, pick = bc.params(H.shape[0])[pset]
    return ops.bpgd_host(H, x, iters0, iters_round, rounds, per_round, pick, bc.CLAMP, bc.ALPHA,
                         bc.BETA)


def test_recorded_coverage_holds_every_required_fact():
    bc.assert_required_coverage()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('pset', [0, 1, 2, 3])
@pytest.mark.parametrize('code,B', SHAPES)
def test_host_mirror_equals_reference(code, B, pset, dtype):
    ref = bc.reference(code, B, dtype, pset)
    got = host(code, B, dtype, pset)
    bc.assert_equal(got, ref, (code, B, dtype, pset))
    H, x = bc.inputs(code, B, dtype)
    ehat, llr, pred, its, status, ndec = got
    # ehat is the hard decision of llr, and status 0 is exactly a satisfied syndrome
    assert set(np.unique(ehat).tolist()) <= {0.0, 1.0}
    assert np.array_equal(ehat, (llr < 0).astype(ehat.dtype))
    assert np.array_equal(status == 0, bc.satisfied(H, x, llr))
    assert np.allclose(pred, ref['pred'], **mc.pred_tolerance(dtype))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B', [('toric_5', 67), ('bch_63_45', 33)])
def test_no_rounds_is_minsum(code, B, dtype):
    """rounds = 0: llr, iters and status are minsum_host(early_stop=True)'s bits, on the BCH inputs
    with their -0.0 priors too, whatever per_round, pick and clamp say."""
    H, x = mc.inputs(code, B, dtype)
    assert code != 'bch_63_45' or (np.signbit(x) & (x == 0)).any()
    ehat, llr, pred, its, status, ndec = ops.bpgd_host(H, x, 12, 7, 0, 3, 'most', 2.0)
    _, m_llr, m_its, m_st = ops.minsum_host(H, x, 12, early_stop=True)
    assert np.array_equal(llr, m_llr) and np.array_equal(np.signbit(llr), np.signbit(m_llr))
    assert np.array_equal(its, m_its) and np.array_equal(status, m_st)
    assert not ndec.any() and set(m_st.tolist()) == {0, 1}


def test_fp64_pred_is_the_fixed_exponential():
    """h_pred in fp64 is 1 / (1 + exp(L)) through gnnd_bposd's fixed exponential: the bits of
    bposd_host's pred on the same posteriors (rounds = 0 makes them min-sum's)."""
    H, x = mc.inputs('toric_5', 9, 'float64')
    pred = ops.bpgd_host(H, x, 12, 1, 0)[2]
    assert np.array_equal(pred, ops.bposd_host(H, x, 12)[5])


def test_argument_checks_before_any_device_call():
    lib = _lib.get()
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    v = np.array([0, 1], np.int64)
    c = np.array([0, 0], np.int64)
    x = np.zeros(3)
    real = [np.zeros(2) for _ in range(3)]
    ints = [np.zeros(1, np.int32) for _ in range(3)]
    vp, cp = v.ctypes.data_as(P64), c.ctypes.data_as(P64)
    rp = [a.ctypes.data for a in real]
    ip = [a.ctypes.data_as(P32) for a in ints]

    def host(dtype=_lib.F64, alpha=0.75, beta=0.0, iters0=3, iters_round=2, rounds=2, per_round=1,
             pick=0, clamp=25.0, batch=1, xp=x.ctypes.data, op=rp[0], rest=rp[1:], ips=ip, var=vp,
             chk=cp, E=2, V=2, C=1):
        return lib.gnnd_bpgd_host(var, chk, E, V, C, dtype, xp, alpha, beta, iters0, iters_round,
                                  rounds, per_round, pick, clamp, op, *rest, *ips, batch)

    assert host() == _lib.OK
    assert host(dtype=_lib.F32) == _lib.OK
    assert host(pick=1, per_round=5, rounds=9) == _lib.OK          # more picks asked than variables
    assert host(rest=[None, None], ips=[None] * 3) == _lib.OK      # the optional outputs
    assert host(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert host(dtype=7) == _lib.ERR_INVALID_ARG
    bad_params = ({'iters0': 0}, {'iters0': -1}, {'iters_round': 0}, {'rounds': -1},
                  {'per_round': 0}, {'per_round': -3}, {'rounds': 2 ** 30, 'iters_round': 2},
                  {'iters0': 2 ** 31 - 1, 'rounds': 1, 'iters_round': 1}, {'pick': 2}, {'pick': -1},
                  {'clamp': 0.0}, {'clamp': -1.0}, {'clamp': float('inf')}, {'clamp': float('nan')},
                  {'alpha': 0.0}, {'alpha': 1.5}, {'alpha': float('nan')}, {'beta': -0.1},
                  {'beta': float('inf')}, {'beta': float('nan')}, {'batch': -1})
    for kw in bad_params:
        assert host(**kw) == _lib.ERR_INVALID_ARG, kw
    # the largest total that fits, and a clamp that is finite only as a double
    assert host(iters0=2 ** 31 - 2, rounds=1, iters_round=1) == _lib.OK    # all-zero x: 1 iteration
    assert host(clamp=1e300) == _lib.OK
    assert host(clamp=1e300, dtype=_lib.F32) == _lib.ERR_INVALID_ARG
    assert host(batch=0, xp=None, op=None, rest=[None, None], ips=[None] * 3) == _lib.OK
    for kw in ({'xp': None}, {'op': None}, {'var': None}, {'chk': None}):
        assert host(**kw) == _lib.ERR_INVALID_ARG, kw
    bad = np.array([0, 2], np.int64)                       # variable id outside [0, V)
    assert host(var=bad.ctypes.data_as(P64)) == _lib.ERR_GRAPH
    unsorted = np.array([1, 0], np.int64)                  # not sorted by (v, c)
    assert host(var=unsorted.ctypes.data_as(P64)) == _lib.ERR_GRAPH
    dv = np.array([0, 1, 2, 2], np.int64)                  # check 1 has the single edge (2, 1)
    dc = np.array([0, 0, 0, 1], np.int64)
    x5, o3 = np.zeros(5), np.zeros(3)
    assert host(var=dv.ctypes.data_as(P64), chk=dc.ctypes.data_as(P64), E=4, V=3, C=2,
                xp=x5.ctypes.data, op=o3.ctypes.data, rest=[None, None]) == _lib.ERR_UNSUPPORTED

    # the device entry point rejects these before it touches a device (a fake non-null handle
    # stands in for the graph: it is never dereferenced on these paths)
    g = ctypes.c_void_p(8)
    d = ctypes.c_void_p(8)

    def dev(graph=g, dtype=_lib.F64, alpha=0.75, beta=0.0, iters0=3, iters_round=2, rounds=2,
            per_round=1, pick=0, clamp=25.0, batch=1, xp=d, op=d):
        return lib.gnnd_bpgd(graph, dtype, xp, alpha, beta, iters0, iters_round, rounds, per_round,
                             pick, clamp, op, d, d, d, d, d, batch, None)

    assert dev(graph=None) == _lib.ERR_INVALID_ARG
    for kw in bad_params:
        assert dev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert dev(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert dev(dtype=7) == _lib.ERR_INVALID_ARG
    assert dev(clamp=1e300, dtype=_lib.F32) == _lib.ERR_INVALID_ARG
    for kw in ({'xp': None}, {'op': None}):
        assert dev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert dev(batch=0, xp=None, op=None) == _lib.OK                # nothing launched


def test_every_variable_decimated_when_more_picks_are_asked_than_variables():
    """rounds * per_round >= V on the smallest graph there is: an unsatisfiable syndrome runs to
    ndec == V and stops there, before `rounds` is used up."""
    H = np.ones((2, 1), np.uint8)                           # one check over two variables
    x = np.array([1.0, 1.0, -1.0, 2.0, 1.0, 1.0])           # codeword 0: t = 1, equal priors; 1: t = 0
    for dtype in (np.float32, np.float64):
        for pick in ('least', 'most'):
            ehat, llr, pred, its, status, ndec = ops.bpgd_host(H, x.astype(dtype), 1, 1, 9, 5, pick)
            # codeword 0, by hand: r = -0.75 on both edges, L = (0.25, 0.25), syndrome 0 != 1; both
            # variables are frozen at +25 in round 0 (min(5, 2) picks, the tie to v = 0 first);
            # then L = 25 - 0.75 on both, still unsatisfied, and ndec == V ends it at r = 1 of 9
            assert (status[0], ndec[0], its[0]) == (1, 2, 2)
            assert llr[:2].tolist() == [24.25, 24.25] and ehat[:2].tolist() == [0.0, 0.0]
            assert (status[1], ndec[1], its[1]) == (0, 0, 1)


def test_wrapper_rejects_bad_inputs():
    H = mc.code_matrix('bch_63_45')
    x = np.zeros(81)
    for kw in ({'iters0': 0}, {'iters0': 2.0}, {'iters_round': 0}, {'rounds': -1}, {'rounds': True},
               {'per_round': 0}, {'pick': 'median'}, {'clamp': 0.0}, {'clamp': float('inf')},
               {'clamp': float('nan')}, {'alpha': 0.0}, {'alpha': 1.5}, {'beta': -1.0},
               {'rounds': 2 ** 30, 'iters_round': 4}):
        args = dict(iters0=5, iters_round=2, rounds=3)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.bpgd_host(H, x, **args)
    with pytest.raises(ValueError):
        ops.bpgd_host(H, np.zeros(80), 5, 2, 3)
    with pytest.raises(TypeError):
        ops.bpgd_host(H, np.zeros(81, np.float16), 5, 2, 3)
