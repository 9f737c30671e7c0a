"""Min-sum BP on the device (ops.minsum -> gnnd_minsum) against the numpy statement of the
definition (tests/minsum_cases.py) and the host mirror, exact equality of llr, iteration counts and
statuses: the shapes where the one-wave-per-codeword plan can go wrong (V not a multiple of 64, a
partial workgroup and the grid-stride tail, several checks and variables per lane, C < 64 with
check degree 24, fewer waves per workgroup), the early exit returning exactly the state of its
iteration, minsum -> osd -> decision_errors end to end, stream capture, the registered ops and the
bounds-checked debug library."""
import ctypes

import numpy as np
import pytest
import torch

import gnndecode as gd
from gnndecode import _lib, ops

import debug_child
import minsum_cases as mc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

# toric-5: V = 100 (not a multiple of 64), B = 1 / 5 / 67: one wave, a partial workgroup, 16 full
# workgroups + a 3-wave tail, every parameter set; toric-7: C = 96, two checks per lane; BCH:
# C = 18 < 64, check degree 24; LDPC: six checks and eleven variables per lane, and in fp64 a
# 29 KB tile: two waves per workgroup instead of four
CASES = ([('toric_5', B, dt, p) for B in (1, 5, 67) for dt in ('float32', 'float64')
          for p in mc.PARAMS]
         + [('toric_7', 9, 'float64', mc.PARAMS[0]), ('bch_63_45', 33, 'float32', mc.PARAMS[2]),
            ('ldpc_648_324', 3, 'float32', mc.PARAMS[0]),
            ('ldpc_648_324', 3, 'float64', mc.PARAMS[0])])

_GRAPHS = {}


def graph_of(code):
    if code not in _GRAPHS:
        _GRAPHS[code] = gd.TannerGraph(mc.code_matrix(code), device=DEV)
    return _GRAPHS[code]


def _np(t):
    return t.cpu().numpy().reshape(-1)


@pytest.mark.parametrize('code,B,dtype,params', CASES)
def test_minsum_equals_reference(code, B, dtype, params):
    alpha, beta, iters, early_stop = params
    H, x = mc.inputs(code, B, dtype)
    ref_llr, ref_it, ref_st = mc.reference(code, B, dtype, params)
    g = graph_of(code)
    xd = torch.from_numpy(x.copy()).to(DEV).unsqueeze(1)
    pred, llr, its, status = ops.minsum(g, xd, iters, alpha, beta, bool(early_stop))
    assert pred.shape == (B * g.V, 1) and pred.dtype == xd.dtype
    assert llr.shape == (B * g.V, 1) and llr.dtype == xd.dtype
    assert its.shape == (B,) and its.dtype == torch.int32
    assert status.shape == (B,) and status.dtype == torch.int32
    got_llr = _np(llr)
    assert np.array_equal(_np(its), ref_it)
    assert np.array_equal(_np(status), ref_st)
    assert np.array_equal(got_llr, ref_llr)
    assert np.array_equal(np.signbit(got_llr), np.signbit(ref_llr))
    tol = mc.pred_tolerance(dtype)
    np.testing.assert_allclose(_np(pred), mc.soft_output(ref_llr), **tol)
    assert np.array_equal(_np(status) == 0, mc.satisfied(H, x, got_llr))
    # the same bits as the host mirror
    h_pred, h_llr, h_it, h_st = ops.minsum_host(H, x, iters, alpha, beta, bool(early_stop))
    assert np.array_equal(h_llr, got_llr) and np.array_equal(np.signbit(h_llr), np.signbit(got_llr))
    assert np.array_equal(h_it, _np(its)) and np.array_equal(h_st, _np(status))
    np.testing.assert_allclose(_np(pred), h_pred, **tol)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_out_forms_null_outputs_and_raw_abi(dtype):
    params = mc.PARAMS[2]
    alpha, beta, iters, early_stop = params
    B = 67
    H, x = mc.inputs('toric_5', B, dtype)
    g = graph_of('toric_5')
    xd = torch.from_numpy(x.copy()).to(DEV)
    pred, llr, its, status = ops.minsum(g, xd, iters, alpha, beta, True)

    def fresh():
        return (torch.full_like(pred, 7), torch.full_like(llr, 7),
                torch.full((B,), 7, dtype=torch.int32, device=DEV),
                torch.full((B,), 7, dtype=torch.int32, device=DEV))

    out = fresh()
    r = ops.minsum(g, xd, iters, alpha, beta, True, out=out)
    assert all(a is b for a, b in zip(r, out))
    for a, b in zip(out, (pred, llr, its, status)):
        assert torch.equal(a, b)
    # every optional output skipped: the same pred, nothing else written
    out = fresh()
    r = ops.minsum(g, xd, iters, alpha, beta, True, out=(out[0], None, None, None))
    assert r[0] is out[0] and r[1] is None and r[2] is None and r[3] is None
    assert torch.equal(out[0], pred)
    out = fresh()
    ops.minsum(g, xd, iters, alpha, beta, True, out=(out[0], None, out[2], None))
    assert torch.equal(out[0], pred) and torch.equal(out[2], its)
    # the raw C ABI call
    out = fresh()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    st = _lib.get().gnnd_minsum(g.handle, _lib.F32 if dtype == 'float32' else _lib.F64, p(xd),
                                alpha, beta, iters, 1, p(out[0]), p(out[1]), p(out[2]), p(out[3]),
                                B, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.OK
    torch.cuda.synchronize()
    for a, b in zip(out, (pred, llr, its, status)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_early_exit_returns_the_state_of_its_iteration(dtype):
    """Codewords that stop early after k iterations hold exactly what a run of k iterations
    without early stop holds."""
    alpha, beta, iters, _ = mc.PARAMS[0]
    B = 67
    H, x = mc.inputs('toric_5', B, dtype)
    g = graph_of('toric_5')
    xd = torch.from_numpy(x.copy()).to(DEV)
    pred, llr, its, status = ops.minsum(g, xd, iters, alpha, beta, True)
    its_h = its.cpu().numpy()
    depths = sorted(set(its_h.tolist()))
    assert len(depths) >= 3
    V = g.V
    for k in depths:
        pk, lk, ik, sk = ops.minsum(g, xd, k, alpha, beta, False)
        assert (ik == k).all()
        rows = torch.from_numpy(np.nonzero(its_h == k)[0]).to(DEV)
        assert torch.equal(lk.view(B, V)[rows], llr.view(B, V)[rows])
        assert torch.equal(pk.view(B, V)[rows], pred.view(B, V)[rows])
        assert torch.equal(sk[rows], status[rows])


def test_unsupported_graph_and_bad_arguments():
    # a check of degree 1: refused with nothing launched
    Hd = np.zeros((3, 2), np.uint8)
    Hd[[0, 1, 2, 2], [0, 0, 0, 1]] = 1
    gdeg = gd.TannerGraph(Hd, device=DEV)
    x = torch.zeros(5, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.GnndError) as e:
        ops.minsum(gdeg, x, 5)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    g = graph_of('toric_5')
    empty = torch.empty(0, 1, dtype=torch.float64, device=DEV)
    pred, llr, its, status = ops.minsum(g, empty, 5)
    assert pred.numel() == 0 and llr.numel() == 0 and its.numel() == 0 and status.numel() == 0
    xd = torch.zeros(g.N, 1, dtype=torch.float64, device=DEV)
    for kw in ({'iters': 0}, {'alpha': 0.0}, {'alpha': 1.5}, {'beta': -1.0}):
        args = dict(iters=5, alpha=0.75, beta=0.0)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.minsum(g, xd, **args)
    with pytest.raises(ValueError):
        ops.minsum(g, xd[:-1], 5)
    with pytest.raises(TypeError):
        ops.minsum(g, xd.bfloat16(), 5)
    with pytest.raises(RuntimeError):
        ops.minsum(g, xd.cpu(), 5)


def test_nonfinite_codeword_stays_in_its_codeword():
    """A NaN and an infinity in one codeword: the call completes and every other codeword's
    outputs are the bits of the clean batch."""
    alpha, beta, iters, _ = mc.PARAMS[0]
    B = 9
    H, x = mc.inputs('toric_5', B, 'float64')
    g = graph_of('toric_5')
    xd = torch.from_numpy(x.copy()).to(DEV)
    clean = ops.minsum(g, xd, iters, alpha, beta, True)
    xb = xd.clone()
    xb[4 * g.N + 3] = float('nan')
    xb[4 * g.N + 17] = float('inf')
    dirty = ops.minsum(g, xb, iters, alpha, beta, True)
    torch.cuda.synchronize()
    keep = torch.tensor([b for b in range(B) if b != 4], device=DEV)
    V = g.V
    for c, d in zip(clean[:2], dirty[:2]):
        assert torch.equal(c.view(B, V)[keep], d.view(B, V)[keep])
    for c, d in zip(clean[2:], dirty[2:]):
        assert torch.equal(c[keep], d[keep])
    assert 1 <= int(dirty[2][4]) <= iters and int(dirty[3][4]) in (0, 1)


def test_minsum_osd_decision_errors_end_to_end():
    """sample_toric (toric-5, p = 0.05, B = 256) -> minsum -> osd('cs', 10) -> decision_errors: no
    codeword keeps a residual syndrome, and where minsum reports status 0 the hard decision of its
    pred satisfies the syndrome."""
    g = graph_of('toric_5')
    H = mc.code_matrix('toric_5')
    B = 256
    lg = torch.from_numpy(gd.codes.toric_logicals(H).astype(np.int32)).to(DEV)
    x, y = ops.sample_toric(g, B, [0.05], seed=11)
    pred, llr, its, status = ops.minsum(g, x, 12)
    ehat, ost, choice = ops.osd(g, x, pred, 'zero', 'cs', 10)
    assert int(ost.abs().sum()) == 0
    counts = ops.decision_errors(g, lg, ehat, y).tolist()
    assert counts[2] == 0
    st = status.cpu().numpy()
    assert set(st.tolist()) == {0, 1}
    V, C = H.shape
    xs = x.cpu().numpy().reshape(B, V + C)
    t = (xs[:, V:] < 0).astype(np.int64)
    p = pred.cpu().numpy().reshape(B, V)
    L = llr.cpu().numpy().reshape(B, V)
    # a pred that rounded to exactly 0.5 (|llr| below half an ulp of 1) decides nothing: skipped
    skipped = 0
    for b in np.nonzero(st == 0)[0]:
        if (p[b] == 0.5).any():
            skipped += 1
            continue
        h = (p[b] > 0.5).astype(np.int64)
        assert np.array_equal(h, (L[b] < 0).astype(np.int64))
        assert np.array_equal((h @ H.astype(np.int64)) % 2, t[b])
    assert skipped == 0


def test_minsum_and_osd_in_one_capture():
    """gnnd_minsum only launches on the stream: captured in front of gnnd_osd, two replays give the
    eager bits."""
    g = graph_of('toric_5')
    B = 256
    x, y = ops.sample_toric(g, B, [0.05], seed=12)
    e_ms = ops.minsum(g, x, 12)
    e_osd = ops.osd(g, x, e_ms[0], 'zero', 'cs', 10)
    sx = x.clone()
    n = B * g.V
    ms = (torch.empty(n, 1, dtype=x.dtype, device=DEV), torch.empty(n, 1, dtype=x.dtype, device=DEV),
          torch.empty(B, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV))
    od = (torch.empty(n, 1, dtype=x.dtype, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV),
          torch.empty(B, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.minsum(g, sx, 12, out=ms)
        ops.osd(g, sx, ms[0], 'zero', 'cs', 10, out=od)
    for _ in range(2):
        for t in ms + od:
            t.fill_(7)
        cg.replay()
        torch.cuda.synchronize()
        for a, b in zip(ms + od, e_ms + e_osd):
            assert torch.equal(a, b)


def test_minsum_traces_as_registered_ops():
    """gnnd::minsum and gnnd::minsum_out have fake kernels: shapes and dtypes without a launch,
    under FakeTensorMode and on the meta device; the real ops give the reference's bits."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    g = graph_of('toric_5')
    for dt in (torch.float32, torch.float64):
        with FakeTensorMode():
            x = torch.empty(3 * g.N, 1, dtype=dt, device=DEV)
            pred, llr, its, status = torch.ops.gnnd.minsum(g.gid, x, 12, 0.75, 0.0, True)
            assert pred.shape == (3 * g.V, 1) and pred.dtype == dt
            assert llr.shape == (3 * g.V, 1) and llr.dtype == dt
            assert its.shape == (3,) and its.dtype == torch.int32
            assert status.shape == (3,) and status.dtype == torch.int32
            assert torch.ops.gnnd.minsum_out(g.gid, x, 12, 0.75, 0.0, True, pred, llr, its,
                                             status) is None
        xm = torch.empty(3 * g.N, 1, dtype=dt, device='meta')
        pred, llr, its, status = torch.ops.gnnd.minsum(g.gid, xm, 12, 0.75, 0.0, True)
        assert pred.shape == (3 * g.V, 1) and pred.dtype == dt and pred.device.type == 'meta'
        assert its.shape == (3,) and its.dtype == torch.int32 and status.shape == (3,)
    params = mc.PARAMS[0]
    H, xs = mc.inputs('toric_5', 5, 'float64')
    ref_llr, ref_it, ref_st = mc.reference('toric_5', 5, 'float64', params)
    xd = torch.from_numpy(xs.copy()).to(DEV)
    pred, llr, its, status = torch.ops.gnnd.minsum(g.gid, xd, params[2], params[0], params[1], True)
    assert np.array_equal(_np(llr), ref_llr) and np.array_equal(_np(its), ref_it)
    out = (torch.empty_like(pred), torch.empty_like(llr), torch.empty_like(its),
           torch.empty_like(status))
    torch.ops.gnnd.minsum_out(g.gid, xd, params[2], params[0], params[1], True, *out)
    for a, b in zip(out, (pred, llr, its, status)):
        assert torch.equal(a, b)


def test_debug_library_runs_minsum_clean():
    """toric-5 B = 67 and LDPC B = 3 under the bounds-checked build (GNND_LIB, a fresh child
    process): no index check fires and the bits are the numpy reference's."""
    res = debug_child.run('decoder_debug_worker.py', 'minsum')
    assert res['equal'] == {'toric_5': True, 'ldpc_648_324': True}
