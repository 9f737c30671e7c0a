"""Weighted union-find and belief-find, host mirrors (gnnd_ufw_host, gnnd_belief_find_host through
ops.ufw_host / ops.belief_find_host) against the independent unit-step statement of
tests/ufw_cases.py: every output bit for bit on the graphs of tests/uf_cases.py, in both dtypes,
with llr and with the priors; the scale = 0 anchor against uf_host and against uf_cases' statement;
H^T ehat == t wherever status is 0; unsatisfiable syndromes; the gate in both pass-through modes;
belief_find_host against minsum_host and ufw_host composed by hand; the refusals; the ABI symbols.
CPU only."""
import ctypes

import numpy as np
import pytest

import gnndecode as gd
from gnndecode import _lib, ops

import minsum_cases as mc
import uf_cases as uc
import ufw_cases as wc


def test_recorded_coverage_holds_every_required_fact():
    wc.assert_required_coverage()


@pytest.mark.parametrize('with_llr', [True, False], ids=['llr', 'priors'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', wc.SHAPES)
def test_host_mirror_equals_the_statement_and_satisfies_the_syndrome(shape, dtype, with_llr):
    B = wc.B_ALL
    H, x, llr = wc.inputs(shape, B, dtype)
    ref = wc.reference(shape, B, dtype, with_llr)
    got = ops.ufw_host(H, x, llr if with_llr else None, wc.SCALE, wc.WMAX)
    wc.assert_equal(got, ref, (shape, dtype, with_llr))
    ehat, rounds, status, nfull, events = got
    V, C = H.shape
    assert ehat.dtype == np.dtype(dtype) and set(np.unique(ehat).tolist()) <= {0.0, 1.0}
    t = x.reshape(B, V + C)[:, V:] < 0
    assert not status.any()
    assert np.array_equal(uc.syndrome(H, ehat.reshape(B, V)), t)
    zero = ~t.any(axis=1)
    assert zero.any() and not rounds[zero].any() and not events[zero].any()
    assert not nfull[zero].any() and not ehat.reshape(B, V)[zero].any()
    # sub-batches are the first codewords of the batch: codewords are independent
    for sub in (1, 3):
        Hs, xs, ls = wc.inputs(shape, sub, dtype)
        wc.assert_equal(ops.ufw_host(Hs, xs, ls if with_llr else None, wc.SCALE, wc.WMAX),
                        wc.reference(shape, sub, dtype, with_llr), (shape, dtype, sub))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', wc.SHAPES)
def test_scale_zero_and_wmax_one_are_uf(shape, dtype):
    """The anchor: every weight 1, so ehat / rounds / status / nfull are uf_host's bits, and those
    of uf_cases' statement; the unit-step statement of ufw_cases says the same, which ties its
    forest and peel to uf_cases'."""
    B = wc.B_ALL
    H, x, llr = wc.inputs(shape, B, dtype)
    host = ops.uf_host(H, x)
    r = uc.uf_ref(H, x)
    uc.assert_equal(host, (r['ehat01'].reshape(-1).astype(dtype), r['rounds'], r['status'],
                           r['nfull']))
    for kw in (dict(scale=0.0, wmax=32), dict(scale=3.0, wmax=1)):
        for l in (llr, None):
            got = ops.ufw_host(H, x, l, **kw)
            uc.assert_equal(got[:4], host, (shape, dtype, kw))
            assert (got[4] <= got[1]).all() and ((got[4] == 0) == (got[1] == 0)).all()
    st = wc.ufw_ref(H, x, llr, scale=0.0, wmax=32)
    uc.assert_equal(wc.as_tuple(st, dtype)[:4], host, (shape, dtype, 'statement'))
    assert np.array_equal(st['events'], ops.ufw_host(H, x, llr, 0.0, 32)[4])


@pytest.mark.parametrize('shape', ['ring_63', 'two_comp'])
def test_an_unsatisfiable_syndrome_stops_with_status_1(shape):
    H = uc.code_matrix(shape)
    V, C = H.shape
    x = np.ones((3, V + C))
    x[0, V + 2] = -1                                        # one defect on the ring
    x[1, V + 1] = x[1, V + 3] = -1                          # two: satisfiable
    x[2, V + 0] = x[2, V + 1] = x[2, V + 4] = -1            # three
    llr = np.random.default_rng(3).normal(1.5, 2.5, (3, V))
    for l in (llr.reshape(-1), None):
        got = ops.ufw_host(H, x.reshape(-1), l, wc.SCALE, wc.WMAX)
        wc.assert_equal(got, wc.as_tuple(wc.ufw_ref(H, x.reshape(-1), l), 'float64'))
        ehat, rounds, status, nfull, events = got
        assert status.tolist() == [1, 0, 1]
        ring_edges = 63 if shape == 'ring_63' else 5
        assert nfull[0] == nfull[2] == ring_edges and 0 < nfull[1] < ring_edges
        bad = uc.syndrome(H, ehat.reshape(3, V)) != (x[:, V:] < 0)
        assert bad.sum(axis=1).tolist() == [1, 0, 1]


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_non_finite_and_signed_zero_inputs_only_change_weights(dtype):
    """NaN, +-0 and +-inf in llr, in the priors and in the syndrome rows: the mirror is the
    statement's bits, and ehat satisfies the syndrome its signs give."""
    shape, B = 'toric_5', 9
    H, x, llr = wc.inputs(shape, B, dtype)
    xb, lb = wc.dirty_inputs(H, x, llr, B)
    V, C = H.shape
    with np.errstate(invalid='ignore'):
        t = xb[:, V:] < 0
    for l in (lb.reshape(-1), None):
        got = ops.ufw_host(H, xb.reshape(-1), l, wc.SCALE, wc.WMAX)
        wc.assert_equal(got, wc.as_tuple(wc.ufw_ref(H, xb.reshape(-1), l), dtype))
        assert np.array_equal(uc.syndrome(H, got[0].reshape(B, V)), t) and not got[2].any()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_gate_skips_or_passes_through(dtype):
    """Through the raw ABI over sentinel-filled outputs.  passthrough 0: the rows whose gate is 0
    keep the sentinel.  passthrough 1: they get (llr < 0) and zero counters.  The others hold the
    ungated bits in both modes."""
    shape, B = 'toric_5', 13
    H, x, llr = wc.inputs(shape, B, dtype)
    V, C = H.shape
    llr = llr.copy()
    llr[:8] = [np.nan, -0.0, 0.0, -np.inf, np.inf, -1.0, 1.0, -1e-30]
    full = ops.ufw_host(H, x, llr, wc.SCALE, wc.WMAX)
    gate = (np.arange(B) % 3 != 1).astype(np.int32) * np.array([1, 5, -2] * 5, np.int32)[:B]
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    var, chk = gd.graph.edge_list(H)
    on = gate != 0
    assert on.any() and (~on).any() and not on[1]
    for passthrough in (0, 1):
        ehat = np.full(B * V, 7, dtype)
        ints = [np.full(B, 7, np.int32) for _ in range(4)]
        st = _lib.get().gnnd_ufw_host(
            var.ctypes.data_as(P64), chk.ctypes.data_as(P64), var.size, V, C,
            _lib.F32 if dtype == 'float32' else _lib.F64, x.ctypes.data, llr.ctypes.data, wc.SCALE,
            wc.WMAX, gate.ctypes.data_as(P32), passthrough, ehat.ctypes.data,
            *(a.ctypes.data_as(P32) for a in ints), B)
        assert st == _lib.OK
        assert np.array_equal(ehat.reshape(B, V)[on], full[0].reshape(B, V)[on])
        for a, f in zip(ints, full[1:]):
            assert np.array_equal(a[on], f[on])
        if passthrough:
            with np.errstate(invalid='ignore'):
                hard = (llr.reshape(B, V) < 0).astype(dtype)
            assert np.array_equal(ehat.reshape(B, V)[~on], hard[~on])
            assert all(not a[~on].any() for a in ints)
        else:
            assert (ehat.reshape(B, V)[~on] == 7).all() and all((a[~on] == 7).all() for a in ints)
    # llr row 0 of codeword 0 is not gated off; codeword 1 is: its first eight pass-through bits
    w = ops.ufw_host(H, x, np.roll(llr, V), wc.SCALE, wc.WMAX, gate=gate, passthrough=True)
    assert w[0].reshape(B, V)[1, :8].tolist() == [0, 0, 0, 1, 0, 1, 0, 1]
    # the wrapper returns the rows a gate skips as zeros
    w = ops.ufw_host(H, x, llr, wc.SCALE, wc.WMAX, gate=gate)
    assert not w[0].reshape(B, V)[~on].any() and not w[1][~on].any() and not w[4][~on].any()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_belief_find_host_is_minsum_then_ufw(dtype):
    H, x = wc.bf_inputs(dtype)
    B = wc.B_ALL
    V, C = H.shape
    pred, llr, its, bp_status = ops.minsum_host(H, x, wc.BF_ITERS, wc.BF_ALPHA, wc.BF_BETA, True)
    assert set(bp_status.tolist()) == {0, 1}, 'the inputs must leave min-sum both statuses'
    by_hand = ops.ufw_host(H, x, llr, wc.SCALE, wc.WMAX, gate=bp_status, passthrough=True)
    out = ops.belief_find_host(H, x, wc.BF_ITERS, wc.BF_ALPHA, wc.BF_BETA, True, wc.SCALE, wc.WMAX)
    ehat, status, iters_used, bst, bpred, bllr, rounds, nfull, events = out
    assert np.array_equal(bllr, llr) and np.array_equal(iters_used, its)
    assert np.array_equal(bst, bp_status)
    np.testing.assert_allclose(bpred, pred, rtol=1e-5 if dtype == 'float32' else 1e-12)
    wc.assert_equal((ehat, rounds, status, nfull, events), by_hand)
    t = x.reshape(B, V + C)[:, V:] < 0
    assert np.array_equal(uc.syndrome(H, ehat.reshape(B, V)), t) and not status.any()
    solved = bp_status == 0
    assert np.array_equal(ehat.reshape(B, V)[solved], (llr.reshape(B, V) < 0)[solved])
    assert not rounds[solved].any() and not events[solved].any() and not nfull[solved].any()
    assert (rounds[~solved] >= 1).all() and (events[~solved] >= 1).all()
    # and the unsolved rows are the statement's on min-sum's posteriors
    st = wc.ufw_ref(H, x, llr)
    assert np.array_equal(ehat.reshape(B, V)[~solved], st['ehat01'][~solved])
    assert np.array_equal(rounds[~solved], st['rounds'][~solved])


def test_wrapper_rejects_bad_inputs():
    H = uc.code_matrix('toric_3')
    V, C = H.shape
    x = np.zeros(2 * (V + C))
    llr = np.zeros(2 * V)
    gate = np.ones(2, np.int32)
    for kw in (dict(wmax=0), dict(wmax=1025), dict(wmax=8.0), dict(scale=-1.0),
               dict(scale=float('nan')), dict(scale=float('inf')), dict(passthrough=True),
               dict(passthrough=True, gate=gate), dict(passthrough=True, llr=llr),
               dict(llr=llr[:-1]), dict(gate=gate[:1])):
        with pytest.raises(ValueError):
            ops.ufw_host(H, x, **{'llr': None, **kw})
    with pytest.raises(ValueError):
        ops.ufw_host(H, x[:-1])
    with pytest.raises(TypeError):
        ops.ufw_host(H, x.astype(np.float16))
    for kw in (dict(wmax=0), dict(wmax=1025), dict(scale=-1.0), dict(scale=float('nan')),
               dict(iters=0), dict(alpha=0.0), dict(beta=-1.0)):
        with pytest.raises(ValueError):
            ops.belief_find_host(H, x, **{'iters': 5, **kw})


@pytest.mark.parametrize('code', ['bch_63_45', 'syn_hub'])
def test_a_graph_that_is_not_matchable_is_refused(code):
    H = mc.code_matrix(code)
    V, C = H.shape
    with pytest.raises(_lib.GnndError) as e:
        ops.ufw_host(H, np.zeros(V + C))
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.GnndError) as e:
        ops.belief_find_host(H, np.ones(V + C), 5)
    assert e.value.status == _lib.ERR_UNSUPPORTED


def test_argument_checks_before_any_device_call():
    lib = _lib.get()
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    v = np.array([0, 0, 1, 1], np.int64)                    # two variables on checks 0 and 1
    c = np.array([0, 1, 0, 1], np.int64)
    x = np.ones(4)
    llr = np.ones(2)
    ehat = np.zeros(2)
    gate = np.ones(1, np.int32)
    ints = [np.zeros(1, np.int32) for _ in range(4)]
    vp, cp = v.ctypes.data_as(P64), c.ctypes.data_as(P64)
    ip = [a.ctypes.data_as(P32) for a in ints]
    gp = gate.ctypes.data_as(P32)
    nan, inf = float('nan'), float('inf')

    def host(dtype=_lib.F64, batch=1, xp=x.ctypes.data, lp=llr.ctypes.data, scale=2.0, wmax=8,
             gate=gp, passthrough=0, op=ehat.ctypes.data, ips=ip, var=vp):
        return lib.gnnd_ufw_host(var, cp, 4, 2, 2, dtype, xp, lp, scale, wmax, gate, passthrough, op,
                                 *ips, batch)

    assert host() == _lib.OK
    assert host(dtype=_lib.F32, passthrough=1) == _lib.OK
    assert host(ips=[None] * 4, lp=None, gate=None) == _lib.OK
    assert host(wmax=1) == host(wmax=1024) == host(scale=0.0) == _lib.OK
    assert host(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert host(batch=0, xp=None, op=None) == _lib.OK
    for kw in ({'wmax': 0}, {'wmax': 1025}, {'wmax': -1}, {'scale': -0.5}, {'scale': nan},
               {'scale': inf}, {'passthrough': 2}, {'passthrough': -1},
               {'passthrough': 1, 'gate': None}, {'passthrough': 1, 'lp': None}, {'xp': None},
               {'op': None}, {'var': None}, {'batch': -1}, {'dtype': 7}):
        assert host(**kw) == _lib.ERR_INVALID_ARG, kw

    pred = np.zeros(2)
    bst = np.zeros(1, np.int32)

    def bf(dtype=_lib.F64, batch=1, xp=x.ctypes.data, alpha=0.75, beta=0.0, iters=3, early=1,
           scale=2.0, wmax=8, pp=pred.ctypes.data, lp=llr.ctypes.data, bp=bst.ctypes.data_as(P32),
           op=ehat.ctypes.data, ips=ip):
        return lib.gnnd_belief_find_host(vp, cp, 4, 2, 2, dtype, xp, alpha, beta, iters, early, scale,
                                         wmax, pp, lp, ips[0], bp, op, ips[1], ips[2], ips[3],
                                         ips[0], batch)

    assert bf() == _lib.OK
    assert bf(ips=[None] * 4) == _lib.OK
    assert bf(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    for kw in ({'wmax': 0}, {'wmax': 1025}, {'scale': -1.0}, {'scale': nan}, {'iters': 0},
               {'alpha': 0.0}, {'alpha': 1.5}, {'beta': -1.0}, {'early': 2}, {'xp': None},
               {'pp': None}, {'lp': None}, {'bp': None}, {'op': None}, {'batch': -1}):
        assert bf(**kw) == _lib.ERR_INVALID_ARG, kw

    # the device entry points reject these before they touch a device (a fake non-null handle
    # stands in for the graph: it is never dereferenced on these paths)
    g = ctypes.c_void_p(8)
    d = ctypes.c_void_p(8)

    def dev(graph=g, dtype=_lib.F64, batch=1, xp=d, lp=d, scale=2.0, wmax=8, gate=d, passthrough=0,
            op=d):
        return lib.gnnd_ufw(graph, dtype, xp, lp, scale, wmax, gate, passthrough, op, d, d, d, d,
                            batch, None)

    for kw in ({'graph': None}, {'batch': -1}, {'dtype': 7}, {'wmax': 0}, {'wmax': 1025},
               {'scale': -1.0}, {'scale': nan}, {'scale': inf}, {'passthrough': 2},
               {'passthrough': 1, 'gate': None}, {'passthrough': 1, 'lp': None}, {'xp': None},
               {'op': None}):
        assert dev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert dev(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert dev(batch=0, xp=None, op=None) == _lib.OK                # nothing launched

    def dbf(graph=g, dtype=_lib.F64, batch=1, xp=d, alpha=0.75, iters=3, scale=2.0, wmax=8, pp=d,
            lp=d, bp=d, op=d):
        return lib.gnnd_belief_find(graph, dtype, xp, alpha, 0.0, iters, 1, scale, wmax, pp, lp, d,
                                    bp, op, d, d, d, d, batch, None)

    for kw in ({'graph': None}, {'batch': -1}, {'dtype': 7}, {'wmax': 0}, {'wmax': 1025},
               {'scale': -1.0}, {'scale': nan}, {'iters': 0}, {'alpha': 0.0}, {'xp': None},
               {'pp': None}, {'lp': None}, {'bp': None}, {'op': None}):
        assert dbf(**kw) == _lib.ERR_INVALID_ARG, kw
    assert dbf(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert dbf(batch=0, xp=None, op=None) == _lib.OK


def test_abi_symbols_exist():
    lib = _lib.get()
    for name in ('gnnd_ufw', 'gnnd_ufw_host', 'gnnd_belief_find', 'gnnd_belief_find_host',
                 'gnnd_debug_take_ufw'):
        assert hasattr(lib, name), name
