"""Relay min-sum BP on the device (ops.relay -> gnnd_relay) against the numpy statement of the
definition (tests/relay_cases.py) and the host mirror, exact equality of every output: the shapes
where the one-wave-per-codeword plan can go wrong (V not a multiple of 64, a partial workgroup and
the grid-stride tail, several checks and variables per lane, C < 64 with check degree 24, fewer
waves per workgroup), solutions replaced by lighter ones and ties, the one-leg zero-gamma case
against ops.minsum, out= forms, refusals, non-finite inputs, stream capture, the registered ops,
the bounds-checked debug library, and sample_toric -> relay -> decision_errors end to end."""
import ctypes

import numpy as np
import pytest
import torch

import gnndecode as gd
from gnndecode import _lib, ops

import debug_child
import minsum_cases as mc
import relay_cases as rc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

# toric-5: V = 100 (not a multiple of 64), B = 1 / 5 / 67: one wave, a partial workgroup, 16 full
# workgroups + a 3-wave tail, every parameter set; toric-7: two checks per lane; BCH: C = 18 < 64,
# check degree 24; LDPC: many nodes per lane, three waves per workgroup in fp32 and one in fp64;
# hard toric-5: best-replacement and ties
CASES = ([('plain', 'toric_5', B, dt, p) for B in (1, 5, 67) for dt in ('float32', 'float64')
          for p in rc.PARAMS]
         + [('plain', 'toric_7', 9, 'float64', rc.PARAMS[1]),
            ('plain', 'bch_63_45', 33, 'float32', rc.PARAMS[1]),
            ('plain', 'ldpc_648_324', 3, 'float32', rc.PARAMS[3]),
            ('plain', 'ldpc_648_324', 3, 'float64', rc.PARAMS[3]),
            ('hard', 'toric_5', 67, 'float32', rc.PARAMS[2]),
            ('hard', 'toric_5', 67, 'float64', rc.PARAMS[2])])

_GRAPHS = {}


def graph_of(code):
    if code not in _GRAPHS:
        _GRAPHS[code] = gd.TannerGraph(mc.code_matrix(code), device=DEV)
    return _GRAPHS[code]


def _np(t):
    return t.cpu().numpy().reshape(-1)


def _dev_gammas(V, params, dtype):
    return torch.from_numpy(rc.gammas(V, params, dtype).copy()).to(DEV)


@pytest.mark.parametrize('family,code,B,dtype,params', CASES)
def test_relay_equals_reference_and_host_mirror(family, code, B, dtype, params):
    legs, iters0, iters_leg, S = params
    H, x = rc.inputs(family, code, B, dtype)
    ref = rc.reference(family, code, B, dtype, params)
    g = graph_of(code)
    xd = torch.from_numpy(x.copy()).to(DEV).unsqueeze(1)
    out = ops.relay(g, xd, _dev_gammas(g.V, params, dtype), iters0, iters_leg, S, rc.ALPHA, rc.BETA)
    ehat, llr, its, status, leg, nsol = out
    assert ehat.shape == (B * g.V, 1) and ehat.dtype == xd.dtype
    assert llr.shape == (B * g.V, 1) and llr.dtype == xd.dtype
    for t in (its, status, leg, nsol):
        assert t.shape == (B,) and t.dtype == torch.int32
    got = tuple(_np(t) for t in out)
    rc.assert_equal(got, ref, 'device against the numpy statement')
    assert np.array_equal(got[3] == 0, rc.satisfied(H, x, got[1]))
    mirror = ops.relay_host(H, x, rc.gammas(g.V, params, dtype), iters0, iters_leg, S, rc.ALPHA,
                            rc.BETA)
    rc.assert_equal(got, mirror, 'device against the host mirror')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B', [('toric_5', 67), ('bch_63_45', 33)])
def test_one_leg_zero_gamma_is_minsum(code, B, dtype):
    H, x = mc.inputs(code, B, dtype)
    g = graph_of(code)
    xd = torch.from_numpy(x.copy()).to(DEV)
    zero = torch.zeros(1, g.V, dtype=xd.dtype, device=DEV)
    ehat, llr, its, status, leg, nsol = ops.relay(g, xd, zero, 12)
    pred, m_llr, m_its, m_st = ops.minsum(g, xd, 12)
    assert torch.equal(llr, m_llr) and torch.equal(torch.signbit(llr), torch.signbit(m_llr))
    assert torch.equal(its, m_its) and torch.equal(status, m_st)
    assert torch.equal(ehat, (m_llr < 0).to(xd.dtype))
    assert torch.equal(nsol, 1 - m_st) and torch.equal(leg, -m_st)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_out_forms_null_outputs_and_raw_abi(dtype):
    params = rc.PARAMS[1]
    legs, iters0, iters_leg, S = params
    B = 67
    H, x = rc.inputs('plain', 'toric_5', B, dtype)
    g = graph_of('toric_5')
    xd = torch.from_numpy(x.copy()).to(DEV)
    gm = _dev_gammas(g.V, params, dtype)
    base = ops.relay(g, xd, gm, iters0, iters_leg, S)

    def fresh():
        return ((torch.full_like(base[0], 7), torch.full_like(base[1], 7))
                + tuple(torch.full((B,), 7, dtype=torch.int32, device=DEV) for _ in range(4)))

    out = fresh()
    r = ops.relay(g, xd, gm, iters0, iters_leg, S, out=out)
    assert all(a is b for a, b in zip(r, out))
    for a, b in zip(out, base):
        assert torch.equal(a, b)
    # every optional output skipped: the same ehat, nothing else written
    out = fresh()
    r = ops.relay(g, xd, gm, iters0, iters_leg, S, out=(out[0],) + (None,) * 5)
    assert r[0] is out[0] and all(t is None for t in r[1:])
    assert torch.equal(out[0], base[0])
    out = fresh()
    ops.relay(g, xd, gm, iters0, iters_leg, S, out=(out[0], None, out[2], None, out[4], None))
    assert torch.equal(out[0], base[0]) and torch.equal(out[2], base[2])
    assert torch.equal(out[4], base[4])
    assert all(bool((out[i] == 7).all()) for i in (1, 3, 5))
    # the raw C ABI call
    out = fresh()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    st = _lib.get().gnnd_relay(g.handle, _lib.F32 if dtype == 'float32' else _lib.F64, p(xd), p(gm),
                               legs, iters0, iters_leg, S, 0.75, 0.0, *(p(t) for t in out), B,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.OK
    torch.cuda.synchronize()
    for a, b in zip(out, base):
        assert torch.equal(a, b)


def test_unsupported_graph_bad_arguments_and_empty_batch():
    # a check of degree 1: refused with nothing launched
    Hd = np.zeros((3, 2), np.uint8)
    Hd[[0, 1, 2, 2], [0, 0, 0, 1]] = 1
    gdeg = gd.TannerGraph(Hd, device=DEV)
    x = torch.zeros(5, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.GnndError) as e:
        ops.relay(gdeg, x, torch.zeros(2, 3, dtype=torch.float64, device=DEV), 5)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    g = graph_of('toric_5')
    gm = ops.relay_gammas(g.V, 3, device=DEV)
    empty = torch.empty(0, 1, dtype=torch.float64, device=DEV)
    out = ops.relay(g, empty, gm, 5)
    assert len(out) == 6 and all(t.numel() == 0 for t in out)
    xd = torch.zeros(g.N, 1, dtype=torch.float64, device=DEV)
    for kw in ({'iters0': 0}, {'iters_leg': 0}, {'stop_after': 0}, {'iters0': 2.5}, {'alpha': 0.0},
               {'alpha': 1.5}, {'beta': -1.0}):
        args = dict(iters0=5)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.relay(g, xd, gm, **args)
    with pytest.raises(ValueError):
        ops.relay(g, xd[:-1], gm, 5)
    with pytest.raises(ValueError):
        ops.relay(g, xd, gm[:, :-1], 5)
    with pytest.raises(ValueError):
        ops.relay(g, xd, gm[:0], 5)
    with pytest.raises(TypeError):
        ops.relay(g, xd, gm.float(), 5)
    with pytest.raises(TypeError):
        ops.relay(g, xd.bfloat16(), gm.bfloat16(), 5)
    with pytest.raises(RuntimeError):
        ops.relay(g, xd.cpu(), gm, 5)
    with pytest.raises(RuntimeError):
        ops.relay(g, xd, gm.cpu(), 5)


def test_nonfinite_codeword_stays_in_its_codeword():
    """A NaN and an infinity in codeword 4 of 9: the call completes and the other eight codewords'
    outputs are the bits of the clean batch."""
    legs, iters0, iters_leg, S = params = rc.PARAMS[1]
    B = 9
    H, x = rc.inputs('plain', 'toric_5', B, 'float64')
    g = graph_of('toric_5')
    xd = torch.from_numpy(x.copy()).to(DEV)
    gm = _dev_gammas(g.V, params, 'float64')
    clean = ops.relay(g, xd, gm, iters0, iters_leg, 2)
    xb = xd.clone()
    xb[4 * g.N + 3] = float('nan')
    xb[4 * g.N + 17] = float('inf')
    dirty = ops.relay(g, xb, gm, iters0, iters_leg, 2)
    torch.cuda.synchronize()
    keep = torch.tensor([b for b in range(B) if b != 4], device=DEV)
    V = g.V
    for c, d in zip(clean[:2], dirty[:2]):
        assert torch.equal(c.view(B, V)[keep], d.view(B, V)[keep])
    for c, d in zip(clean[2:], dirty[2:]):
        assert torch.equal(c[keep], d[keep])
    assert 1 <= int(dirty[2][4]) <= iters0 + (legs - 1) * iters_leg
    assert int(dirty[3][4]) in (0, 1)


def test_capture_gives_the_eager_bits_on_two_replays():
    legs, iters0, iters_leg, S = params = rc.PARAMS[2]
    B = 67
    H, x = rc.inputs('hard', 'toric_5', B, 'float64')
    g = graph_of('toric_5')
    sx = torch.from_numpy(x.copy()).to(DEV)
    gm = _dev_gammas(g.V, params, 'float64')
    eager = ops.relay(g, sx, gm, iters0, iters_leg, S)
    out = ((torch.empty_like(eager[0]), torch.empty_like(eager[1]))
           + tuple(torch.empty(B, dtype=torch.int32, device=DEV) for _ in range(4)))
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.relay(g, sx, gm, iters0, iters_leg, S, out=out)
    for _ in range(2):
        for t in out:
            t.fill_(7)
        cg.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)


def test_relay_traces_as_registered_ops():
    """gnnd::relay and gnnd::relay_out have fake kernels: shapes and dtypes without a launch, under
    FakeTensorMode and on the meta device; the real ops give the reference's bits."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    g = graph_of('toric_5')
    for dt in (torch.float32, torch.float64):
        with FakeTensorMode():
            x = torch.empty(3 * g.N, 1, dtype=dt, device=DEV)
            gm = torch.empty(4, g.V, dtype=dt, device=DEV)
            out = torch.ops.gnnd.relay(g.gid, x, gm, 12, 10, 2, 0.75, 0.0)
            assert len(out) == 6
            for t in out[:2]:
                assert t.shape == (3 * g.V, 1) and t.dtype == dt
            for t in out[2:]:
                assert t.shape == (3,) and t.dtype == torch.int32
            assert torch.ops.gnnd.relay_out(g.gid, x, gm, 12, 10, 2, 0.75, 0.0, *out) is None
        xm = torch.empty(3 * g.N, 1, dtype=dt, device='meta')
        gmm = torch.empty(4, g.V, dtype=dt, device='meta')
        out = torch.ops.gnnd.relay(g.gid, xm, gmm, 12, 10, 2, 0.75, 0.0)
        assert out[0].shape == (3 * g.V, 1) and out[0].dtype == dt and out[0].device.type == 'meta'
        assert out[4].shape == (3,) and out[4].dtype == torch.int32
    legs, iters0, iters_leg, S = params = rc.PARAMS[1]
    H, xs = rc.inputs('plain', 'toric_5', 5, 'float64')
    ref = rc.reference('plain', 'toric_5', 5, 'float64', params)
    xd = torch.from_numpy(xs.copy()).to(DEV)
    gm = _dev_gammas(g.V, params, 'float64')
    out = torch.ops.gnnd.relay(g.gid, xd, gm, iters0, iters_leg, S, rc.ALPHA, rc.BETA)
    rc.assert_equal(tuple(_np(t) for t in out), ref)
    out2 = tuple(torch.empty_like(t) for t in out)
    torch.ops.gnnd.relay_out(g.gid, xd, gm, iters0, iters_leg, S, rc.ALPHA, rc.BETA, *out2)
    for a, b in zip(out2, out):
        assert torch.equal(a, b)


def test_debug_library_runs_relay_clean():
    """toric-5 B = 67 and LDPC B = 3 under the bounds-checked build (GNND_LIB, a fresh child
    process): no index check fires and the bits are the numpy reference's."""
    res = debug_child.run('decoder_debug_worker.py', 'relay')
    assert res['equal'] == {'toric_5': True, 'ldpc_648_324': True}


def test_sample_relay_decision_errors_end_to_end():
    """sample_toric (toric-5, p = 0.05, B = 256, seed 11) -> relay (6 legs x 12, S = 1) ->
    decision_errors: every status-0 codeword has zero residual syndrome, relay solves strictly more
    codewords than ops.minsum(g, x, 12) on the same x, and at most the status-1 codewords keep a
    residual syndrome."""
    g = graph_of('toric_5')
    H = mc.code_matrix('toric_5')
    B = 256
    lg = torch.from_numpy(gd.codes.toric_logicals(H).astype(np.int32)).to(DEV)
    x, y = ops.sample_toric(g, B, [0.05], seed=11)
    gm = ops.relay_gammas(g.V, 6, seed=0, dtype=x.dtype, device=DEV)
    ehat, llr, its, status, leg, nsol = ops.relay(g, x, gm, 12, 12, 1)
    m_status = ops.minsum(g, x, 12)[3]
    solved, m_solved = int(status.eq(0).sum()), int(m_status.eq(0).sum())
    print(f'relay status 0: {solved} of {B}; minsum status 0: {m_solved}')
    V, C = H.shape
    t = (_np(x).reshape(B, V + C)[:, V:] < 0).astype(np.int64)
    h = _np(ehat).reshape(B, V).astype(np.int64)
    residual = (((h @ H.astype(np.int64)) % 2) != t).any(axis=1)
    st = _np(status)
    assert not residual[st == 0].any()
    assert solved > m_solved
    counts = ops.decision_errors(g, lg, ehat, y).tolist()
    print(f'decision_errors: {counts}')
    assert counts[2] <= int((st == 1).sum())
    assert counts[2] == int(residual.sum())
