"""The union-find decoder, host mirror (gnnd_uf_host through ops.uf_host) against the independent
statement of the definition (tests/uf_cases.py): every output bit for bit on toric-3, toric-5,
rings, a chain, parallel edges and a graph of two components, in both dtypes; H^T ehat == t
everywhere; the decoding graph (gnnd_graph_matching_host) against the statement's and, for
toric-5, against the checks of each variable; the refusals of both entry points (before any device
call); the gate; NaN and signed zeros in the syndrome rows; a syndrome no error pattern satisfies.
CPU only."""
import ctypes

import numpy as np
import pytest

import gnndecode as gd
from gnndecode import _lib, ops

import minsum_cases as mc
import uf_cases as uc


def test_recorded_coverage_holds_every_required_fact():
    uc.assert_required_coverage()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', uc.SHAPES)
def test_host_mirror_equals_reference_and_satisfies_the_syndrome(shape, dtype):
    B = uc.B_ALL
    H, x = uc.inputs(shape, B, dtype)
    ref = uc.reference(shape, B, dtype)
    got = ops.uf_host(H, x)
    uc.assert_equal(got, ref, (shape, dtype))
    ehat, rounds, status, nfull = got
    V, C = H.shape
    assert ehat.dtype == np.dtype(dtype) and set(np.unique(ehat).tolist()) <= {0.0, 1.0}
    t = x.reshape(B, V + C)[:, V:] < 0
    assert np.array_equal(uc.syndrome(H, ehat.reshape(B, V)), t)
    assert not status.any()
    zero = ~t.any(axis=1)
    assert zero.any() and not rounds[zero].any() and not nfull[zero].any()
    assert not ehat.reshape(B, V)[zero].any()


@pytest.mark.parametrize('shape', uc.SHAPES)
def test_matching_host_is_the_statements_decoding_graph(shape):
    H = uc.code_matrix(shape)
    N, ends = ops.matching_host(H)
    rN, rends, _ = uc.matching_ref(H)
    assert N == rN and ends.dtype == np.int32 and np.array_equal(ends, rends)
    assert (ends[:, 0] < ends[:, 1]).all() and ends.min() >= 0 and ends.max() < N


def test_matching_of_toric_5_and_the_small_graphs():
    H = uc.code_matrix('toric_5')
    V, C = H.shape
    assert (V, C) == (100, 48)
    N, ends = ops.matching_host(H)
    assert N == 50
    for v in range(V):
        checks = np.nonzero(H[v])[0].tolist()
        assert ends[v, :len(checks)].tolist() == checks
        if len(checks) == 1:
            assert ends[v, 1] in (48, 49)
    # one plaquette of each half is left out: four degree-1 variables per half, and the half that
    # holds check 0 gets virtual vertex 48
    deg1 = np.nonzero(H.sum(axis=1) == 1)[0]
    assert deg1.size == 8
    assert sorted(ends[deg1, 1].tolist()) == [48] * 4 + [49] * 4
    assert ops.matching_host(uc.code_matrix('toric_3'))[0] == 18
    assert ops.matching_host(uc.code_matrix('ring_65'))[0] == 65
    assert ops.matching_host(uc.code_matrix('chain_65'))[0] == 66
    N, ends = ops.matching_host(uc.code_matrix('parallel'))
    assert N == 8 and ends[0].tolist() == ends[8].tolist() == [0, 1]
    N, ends = ops.matching_host(uc.code_matrix('two_comp'))
    assert N == 12 and ends[-2:].tolist() == [[10, 11], [5, 11]]


@pytest.mark.parametrize('code', ['bch_63_45', 'syn_hub'])
def test_a_graph_that_is_not_matchable_is_refused(code):
    H = mc.code_matrix(code)
    V, C = H.shape
    with pytest.raises(_lib.GnndError) as e:
        ops.uf_host(H, np.zeros(V + C))
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.GnndError) as e:
        ops.matching_host(H)
    assert e.value.status == _lib.ERR_UNSUPPORTED


def test_a_variable_of_degree_zero_is_refused():
    H = np.array(uc.code_matrix('ring_63'))
    H[5] = 0
    with pytest.raises(_lib.GnndError) as e:
        ops.uf_host(H, np.zeros(126))
    assert e.value.status == _lib.ERR_UNSUPPORTED


def test_argument_checks_before_any_device_call():
    lib = _lib.get()
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    v = np.array([0, 0, 1], np.int64)                       # variable 0 on checks 0, 1; 1 on check 1
    c = np.array([0, 1, 1], np.int64)
    x = np.zeros(4)
    ehat = np.zeros(2)
    ints = [np.zeros(1, np.int32) for _ in range(3)]
    vp, cp = v.ctypes.data_as(P64), c.ctypes.data_as(P64)
    ip = [a.ctypes.data_as(P32) for a in ints]

    def host(dtype=_lib.F64, batch=1, xp=x.ctypes.data, op=ehat.ctypes.data, ips=ip, var=vp, chk=cp,
             E=3, V=2, C=2, gate=None):
        return lib.gnnd_uf_host(var, chk, E, V, C, dtype, xp, gate, op, *ips, batch)

    assert host() == _lib.OK
    assert host(dtype=_lib.F32) == _lib.OK
    assert host(ips=[None] * 3) == _lib.OK                          # the optional outputs
    assert host(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert host(dtype=7) == _lib.ERR_INVALID_ARG
    assert host(batch=-1) == _lib.ERR_INVALID_ARG
    assert host(batch=0, xp=None, op=None, ips=[None] * 3) == _lib.OK
    for kw in ({'xp': None}, {'op': None}, {'var': None}, {'chk': None}):
        assert host(**kw) == _lib.ERR_INVALID_ARG, kw
    bad = np.array([0, 0, 2], np.int64)                     # variable id outside [0, V)
    assert host(var=bad.ctypes.data_as(P64)) == _lib.ERR_GRAPH
    unsorted = np.array([1, 0, 1], np.int64)                # not sorted by (v, c)
    assert host(chk=unsorted.ctypes.data_as(P64)) == _lib.ERR_GRAPH
    v3 = np.array([0, 0, 0], np.int64)                      # a variable of degree 3
    c3 = np.array([0, 1, 2], np.int64)
    x4 = np.zeros(4)
    assert host(var=v3.ctypes.data_as(P64), chk=c3.ctypes.data_as(P64), V=1, C=3,
                xp=x4.ctypes.data) == _lib.ERR_UNSUPPORTED
    n = ctypes.c_int32()
    assert lib.gnnd_graph_matching_host(vp, cp, 3, 2, 2, ctypes.byref(n), None) == _lib.OK
    assert n.value == 3
    assert lib.gnnd_graph_matching_host(vp, cp, 3, 2, 2, None, None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_graph_matching_host(None, cp, 3, 2, 2, ctypes.byref(n), None) == _lib.ERR_INVALID_ARG

    # the device entry points reject these before they touch a device (a fake non-null handle
    # stands in for the graph: it is never dereferenced on these paths)
    g = ctypes.c_void_p(8)
    d = ctypes.c_void_p(8)

    def dev(graph=g, dtype=_lib.F64, batch=1, xp=d, op=d):
        return lib.gnnd_uf(graph, dtype, xp, None, op, d, d, d, batch, None)

    assert dev(graph=None) == _lib.ERR_INVALID_ARG
    assert dev(batch=-1) == _lib.ERR_INVALID_ARG
    assert dev(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert dev(dtype=7) == _lib.ERR_INVALID_ARG
    for kw in ({'xp': None}, {'op': None}):
        assert dev(**kw) == _lib.ERR_INVALID_ARG, kw
    assert dev(batch=0, xp=None, op=None) == _lib.OK                # nothing launched
    assert lib.gnnd_graph_matching(None, ctypes.byref(n), None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_graph_matching(g, None, None) == _lib.ERR_INVALID_ARG


def test_wrapper_rejects_bad_inputs():
    H = uc.code_matrix('toric_3')
    with pytest.raises(ValueError):
        ops.uf_host(H, np.zeros(51))
    with pytest.raises(TypeError):
        ops.uf_host(H, np.zeros(52, np.float16))
    with pytest.raises(ValueError):
        ops.uf_host(H, np.zeros(52), gate=np.zeros(2, np.int32))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_gate_skips_codewords_and_writes_nothing_of_them(dtype):
    """Through the raw ABI over sentinel-filled outputs: the rows whose gate is 0 keep the
    sentinel, the others hold the ungated bits."""
    shape, B = 'toric_5', 13
    H, x = uc.inputs(shape, B, dtype)
    V, C = H.shape
    full = ops.uf_host(H, x)
    gate = (np.arange(B) % 3 != 1).astype(np.int32) * np.array([1, 5, -2] * 5, np.int32)[:B]
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    var, chk = gd.graph.edge_list(H)
    ehat = np.full(B * V, 7, dtype)
    ints = [np.full(B, 7, np.int32) for _ in range(3)]
    st = _lib.get().gnnd_uf_host(var.ctypes.data_as(P64), chk.ctypes.data_as(P64), var.size, V, C,
                                 _lib.F32 if dtype == 'float32' else _lib.F64, x.ctypes.data,
                                 gate.ctypes.data_as(P32), ehat.ctypes.data,
                                 *(a.ctypes.data_as(P32) for a in ints), B)
    assert st == _lib.OK
    on = gate != 0
    assert on.any() and (~on).any()
    assert np.array_equal(ehat.reshape(B, V)[on], full[0].reshape(B, V)[on])
    assert (ehat.reshape(B, V)[~on] == 7).all()
    for a, f in zip(ints, full[1:]):
        assert np.array_equal(a[on], f[on]) and (a[~on] == 7).all()
    # the wrapper returns the skipped rows as zeros
    w = ops.uf_host(H, x, gate=gate)
    assert np.array_equal(w[0].reshape(B, V)[on], full[0].reshape(B, V)[on])
    assert not w[0].reshape(B, V)[~on].any() and not w[1][~on].any()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_nan_and_signed_zeros_in_the_syndrome_rows(dtype):
    """t_c = (x < 0): a NaN, +0.0 and -0.0 are all syndrome bit 0, and junk priors (NaN and
    infinities among them) are not read."""
    shape, B = 'toric_5', 9
    H, x = uc.inputs(shape, B, dtype)
    V, C = H.shape
    xb = x.reshape(B, V + C).copy()
    t = xb[:, V:] < 0
    rng = np.random.default_rng(5)
    kind = rng.integers(0, 4, t.shape)
    for k, val in ((1, np.nan), (2, 0.0), (3, -0.0)):
        xb[:, V:][(kind == k) & ~t] = val                   # the zero bits only: t is unchanged
    xb[:, :V][::2] = np.nan
    xb[1, :V] = np.inf
    assert np.isnan(xb[:, V:]).any() and (np.signbit(xb[:, V:]) & (xb[:, V:] == 0)).any()
    clean = ops.uf_host(H, x)
    dirty = ops.uf_host(H, xb.reshape(-1))
    uc.assert_equal(dirty, clean)
    # and a NaN where the bit was 1 clears it: still a syndrome, still satisfied
    xb[:, V:][t & (kind == 1)] = np.nan
    with np.errstate(invalid='ignore'):
        t2 = xb[:, V:] < 0
    assert (t2 != t).any()
    ehat, rounds, status, nfull = ops.uf_host(H, xb.reshape(-1))
    assert np.array_equal(uc.syndrome(H, ehat.reshape(B, V)), t2) and not status.any()
    uc.assert_equal((ehat, rounds, status, nfull),
                    _as_tuple(uc.uf_ref(H, xb.reshape(-1)), dtype))


def _as_tuple(res, dtype):
    return (res['ehat01'].reshape(-1).astype(dtype), res['rounds'], res['status'], res['nfull'])


@pytest.mark.parametrize('shape', ['ring_63', 'two_comp'])
def test_an_unsatisfiable_syndrome_stops_with_status_1(shape):
    """A component without a virtual vertex and a syndrome of odd parity on it: no error pattern
    has that syndrome.  The odd cluster grows into the whole component, a round then changes
    nothing, and the decoder stops with status 1, every check but the cluster's root satisfied;
    the statement and the mirror agree on it, and the other codewords are untouched."""
    H = uc.code_matrix(shape)
    V, C = H.shape
    x = np.ones((3, V + C))
    x[0, V + 2] = -1                                        # one defect on the ring
    x[1, V + 1] = x[1, V + 3] = -1                          # two: satisfiable
    x[2, V + 0] = x[2, V + 1] = x[2, V + 4] = -1            # three
    got = ops.uf_host(H, x.reshape(-1))
    uc.assert_equal(got, _as_tuple(uc.uf_ref(H, x.reshape(-1)), 'float64'))
    ehat, rounds, status, nfull = got
    assert status.tolist() == [1, 0, 1]
    ring_edges = 63 if shape == 'ring_63' else 5
    assert nfull[0] == nfull[2] == ring_edges and 0 < nfull[1] < ring_edges
    bad = uc.syndrome(H, ehat.reshape(3, V)) != (x[:, V:] < 0)
    assert bad.sum(axis=1).tolist() == [1, 0, 1]
    root = (63 if shape == 'ring_63' else 5) - 1            # the highest vertex of the ring
    assert bad[0, root] and bad[2, root]
