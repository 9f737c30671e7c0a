"""Layered-schedule min-sum BP on the device (ops.minsum / ops.bposd with schedule='layered' ->
gnnd_minsum_layered / gnnd_bposd_layered) against the numpy statement of the definition
(tests/minsum_layered_cases.py) and the host mirror, exact equality of llr, iteration counts and
statuses: the shapes where the sub-wave-group plan can go wrong (16 lanes and four codewords per
wave with B = 1 / 5 / 67, so idle groups in the last wave; 64 lanes with layers of 36 and 12; 8
lanes with one busy; 32 lanes), groups of one wave stopping at different iterations, a non-finite
codeword next to its wave-mates, the early exit returning exactly the state of its iteration,
bposd on the layered schedule, minsum -> osd -> decision_errors, stream capture, the registered
ops and the bounds-checked debug library."""
import ctypes

import numpy as np
import pytest
import torch

import gnndecode as gd
from gnndecode import _lib, ops

import debug_child
import minsum_cases as mc
import minsum_layered_cases as lc
import osd_cases as oc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

CASES = ([('toric_5', B, dt, p) for B in (1, 5, 67) for dt in ('float32', 'float64')
          for p in lc.PARAMS]
         + [(code, B, dt, lc.PARAMS[0]) for code, B in lc.SHAPES[1:]
            for dt in ('float32', 'float64')])

_GRAPHS = {}


def graph_of(code):
    if code not in _GRAPHS:
        _GRAPHS[code] = gd.TannerGraph(lc.code_matrix(code), device=DEV)
    return _GRAPHS[code]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def _np(t):
    return t.cpu().numpy().reshape(-1)


def layered(g, x, iters, alpha=0.75, beta=0.0, early_stop=True, **kw):
    return ops.minsum(g, x, iters, alpha, beta, early_stop, schedule='layered', **kw)


@pytest.mark.parametrize('code,B,dtype,params', CASES)
def test_layered_equals_reference_and_host(code, B, dtype, params):
    alpha, beta, iters, early_stop = params
    H, x = lc.inputs(code, B, dtype)
    ref_llr, ref_it, ref_st = lc.reference(code, B, dtype, params)
    g = graph_of(code)
    xd = _dev(x).unsqueeze(1)
    pred, llr, its, status = layered(g, xd, iters, alpha, beta, bool(early_stop))
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
    h_pred, h_llr, h_it, h_st = ops.minsum_host(H, x, iters, alpha, beta, bool(early_stop),
                                                schedule='layered')
    assert np.array_equal(h_llr, got_llr) and np.array_equal(np.signbit(h_llr), np.signbit(got_llr))
    assert np.array_equal(h_it, _np(its)) and np.array_equal(h_st, _np(status))
    np.testing.assert_allclose(_np(pred), h_pred, **tol)


def test_flooding_default_is_unchanged_and_unknown_schedule_raises():
    alpha, beta, iters, early = lc.PARAMS[0]
    H, x = lc.inputs('toric_5', 67, 'float64')
    g = graph_of('toric_5')
    xd = _dev(x)
    old = ops.minsum(g, xd, iters, alpha, beta, True)
    new = ops.minsum(g, xd, iters, alpha, beta, True, schedule='flooding')
    assert all(torch.equal(a, b) for a, b in zip(old, new))
    assert np.array_equal(_np(new[1]), mc.reference('toric_5', 67, 'float64', lc.PARAMS[0])[0])
    old = ops.bposd(g, xd, iters, alpha, beta, True)
    new = ops.bposd(g, xd, iters, alpha, beta, True, schedule='flooding')
    assert all(torch.equal(a, b) for a, b in zip(old, new))
    for fn in (ops.minsum, ops.bposd):
        with pytest.raises(ValueError):
            fn(g, xd, iters, schedule='serial')


def test_graph_layers_and_plans():
    """gnnd_graph_layers on the device graph equals the numpy rule, and the plan query reports
    the sub-wave groups: three different lanes-per-codeword values across the codes."""
    lanes = {}
    for code in lc.CODES:
        g = graph_of(code)
        lay = g.layers()
        assert lay.dtype == np.int32 and np.array_equal(lay, lc.layer_of_check(code))
        assert np.array_equal(lay, ops.layers_host(lc.code_matrix(code)))
        sizes = lc.LAYER_SIZES[code]
        for dt in (torch.float32, torch.float64):
            p = ops.minsum_layered_plan(g, dt)
            assert p['layers'] == len(sizes) and p['largest_layer'] == max(sizes)
            G = p['lanes_per_codeword']
            assert G in (8, 16, 32, 64) and G >= min(max(sizes), 64)
            assert p['codewords_per_workgroup'] % (64 // G) == 0
            assert 1 <= p['codewords_per_workgroup'] // (64 // G) <= 4
            lanes[code, dt] = G
    for dt in (torch.float32, torch.float64):
        assert [lanes[c, dt] for c in lc.CODES] == [16, 64, 8, 32]
    assert len(set(lanes.values())) >= 3


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_out_forms_null_outputs_and_raw_abi(dtype):
    alpha, beta, iters, early_stop = lc.PARAMS[2]
    B = 67
    H, x = lc.inputs('toric_5', B, dtype)
    g = graph_of('toric_5')
    xd = _dev(x)
    pred, llr, its, status = layered(g, xd, iters, alpha, beta)

    def fresh():
        return (torch.full_like(pred, 7), torch.full_like(llr, 7),
                torch.full((B,), 7, dtype=torch.int32, device=DEV),
                torch.full((B,), 7, dtype=torch.int32, device=DEV))

    out = fresh()
    r = layered(g, xd, iters, alpha, beta, out=out)
    assert all(a is b for a, b in zip(r, out))
    for a, b in zip(out, (pred, llr, its, status)):
        assert torch.equal(a, b)
    # every optional output skipped: the same pred, nothing else written
    out = fresh()
    r = layered(g, xd, iters, alpha, beta, out=(out[0], None, None, None))
    assert r[0] is out[0] and r[1] is None and r[2] is None and r[3] is None
    assert torch.equal(out[0], pred)
    out = fresh()
    layered(g, xd, iters, alpha, beta, out=(out[0], None, out[2], None))
    assert torch.equal(out[0], pred) and torch.equal(out[2], its)
    # the raw C ABI call
    out = fresh()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    st = _lib.get().gnnd_minsum_layered(
        g.handle, _lib.F32 if dtype == 'float32' else _lib.F64, p(xd), alpha, beta, iters, 1,
        p(out[0]), p(out[1]), p(out[2]), p(out[3]), B,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.OK
    torch.cuda.synchronize()
    for a, b in zip(out, (pred, llr, its, status)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_early_exit_returns_the_state_of_its_iteration(dtype):
    """Codewords that stop early after k iterations hold exactly what a run of k iterations
    without early stop holds, although their wave-mates ran on."""
    alpha, beta, iters, _ = lc.PARAMS[0]
    B = 67
    H, x = lc.inputs('toric_5', B, dtype)
    g = graph_of('toric_5')
    xd = _dev(x)
    pred, llr, its, status = layered(g, xd, iters, alpha, beta)
    its_h = its.cpu().numpy()
    depths = sorted(set(its_h.tolist()))
    assert len(depths) >= 3
    # some wave (four consecutive codewords) holds groups that stop at different iterations
    assert any(len(set(its_h[w:w + 4].tolist())) > 1 for w in range(0, B, 4))
    V = g.V
    for k in depths:
        pk, lk, ik, sk = layered(g, xd, k, alpha, beta, False)
        assert (ik == k).all()
        rows = torch.from_numpy(np.nonzero(its_h == k)[0]).to(DEV)
        assert torch.equal(lk.view(B, V)[rows], llr.view(B, V)[rows])
        assert torch.equal(pk.view(B, V)[rows], pred.view(B, V)[rows])
        assert torch.equal(sk[rows], status[rows])


def test_unsupported_graph_and_bad_arguments():
    Hd = np.zeros((3, 2), np.uint8)                         # a check of degree 1
    Hd[[0, 1, 2, 2], [0, 0, 0, 1]] = 1
    gdeg = gd.TannerGraph(Hd, device=DEV)
    assert gdeg.layers().tolist() == [0, 1]
    x = torch.zeros(5, dtype=torch.float64, device=DEV)
    for call in (lambda: layered(gdeg, x, 5), lambda: ops.bposd(gdeg, x, 5, schedule='layered'),
                 lambda: ops.minsum_layered_plan(gdeg, torch.float64)):
        with pytest.raises(_lib.GnndError) as e:
            call()
        assert e.value.status == _lib.ERR_UNSUPPORTED
    g = graph_of('toric_5')
    empty = torch.empty(0, 1, dtype=torch.float64, device=DEV)
    assert all(t.numel() == 0 for t in layered(g, empty, 5))
    assert all(t.numel() == 0 for t in ops.bposd(g, empty, 5, schedule='layered'))
    xd = torch.zeros(g.N, 1, dtype=torch.float64, device=DEV)
    for kw in ({'iters': 0}, {'alpha': 0.0}, {'alpha': 1.5}, {'beta': -1.0}):
        args = dict(iters=5, alpha=0.75, beta=0.0)
        args.update(kw)
        with pytest.raises(ValueError):
            layered(g, xd, **args)
    with pytest.raises(ValueError):
        layered(g, xd[:-1], 5)
    with pytest.raises(TypeError):
        layered(g, xd.bfloat16(), 5)
    with pytest.raises(RuntimeError):
        layered(g, xd.cpu(), 5)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_nonfinite_codeword_leaves_its_wave_mates_alone(dtype):
    """A NaN and an infinity in codeword 5 of toric-5: codewords 4, 6 and 7 share its wave.  The
    call completes and every other codeword's outputs are the numpy reference's bits."""
    params = lc.PARAMS[0]
    alpha, beta, iters, _ = params
    B = 67
    H, x = lc.inputs('toric_5', B, dtype)
    ref_llr, ref_it, ref_st = lc.reference('toric_5', B, dtype, params)
    g = graph_of('toric_5')
    assert ops.minsum_layered_plan(g, getattr(torch, dtype))['lanes_per_codeword'] == 16
    V = g.V
    xb = _dev(x)
    xb[5 * g.N + 3] = float('nan')
    xb[5 * g.N + 17] = float('inf')
    pred, llr, its, status = layered(g, xb, iters, alpha, beta)
    torch.cuda.synchronize()
    keep = np.array([b for b in range(B) if b != 5])
    assert np.array_equal(_np(llr).reshape(B, V)[keep], ref_llr.reshape(B, V)[keep])
    assert np.array_equal(_np(its)[keep], ref_it[keep])
    assert np.array_equal(_np(status)[keep], ref_st[keep])
    assert 1 <= int(its[5]) <= iters and int(status[5]) in (0, 1)


BPOSD_CASES = [('toric_5', 67, 'float32'), ('toric_5', 67, 'float64'), ('toric_5', 5, 'float64'),
               ('toric_7', 9, 'float64'), ('bch_63_45', 9, 'float32'),
               ('ldpc_648_324', 5, 'float32')]


def _bposd_case(code, B, dtype):
    alpha, beta, iters, early = lc.PARAMS[2] if code.startswith('bch') else lc.PARAMS[0]
    H, x = lc.inputs(code, B, dtype)
    base = 'zero' if code.startswith('toric') else 'hard'
    return H, x, (iters, alpha, beta, bool(early), base, 'cs', 10)


@pytest.mark.parametrize('code,B,dtype', BPOSD_CASES)
def test_bposd_layered_equals_its_two_stages_and_host_mirror(code, B, dtype):
    """bposd(schedule='layered') is the layered minsum followed by osd_gated bit for bit.  Against
    gnnd_bposd_layered_host: every output in fp64 (pred goes through the fixed exponential on
    both sides); in fp32 every output but pred, as tests/test_gpu_bposd.py holds the flooding
    decoder (no column order depends on the last place of pred on these inputs), and ehat /
    status / choice equal osd_gated_host on the soft output the device returned."""
    H, x, args = _bposd_case(code, B, dtype)
    V = H.shape[0]
    g = graph_of(code)
    xd = _dev(x).unsqueeze(1)
    got = ops.bposd(g, xd, *args, schedule='layered')
    ehat, status, choice, its, bp, pred, llr = got
    assert ehat.shape == (B * V, 1) and ehat.dtype == xd.dtype
    m = layered(g, xd, *args[:4])
    o = ops.osd_gated(g, xd, m[0], m[3], *args[4:], llr=m[1])
    for a, b in zip((pred, llr, its, bp, ehat, status, choice), m + o):
        assert np.array_equal(_np(a), _np(b), equal_nan=True)
    params = (args[1], args[2], args[0], int(args[3]))
    r_llr, r_it, r_st = lc.reference(code, B, dtype, params)
    assert np.array_equal(_np(llr), r_llr) and np.array_equal(_np(its), r_it)
    assert np.array_equal(_np(bp), r_st)
    np.testing.assert_allclose(_np(pred), mc.soft_output(r_llr), **mc.pred_tolerance(dtype))
    h2 = ops.osd_gated_host(H, x, _np(pred), _np(bp), *args[4:], llr=_np(llr))
    for a, b in zip((ehat, status, choice), h2):
        assert np.array_equal(_np(a), b)
    host = ops.bposd_host(H, x, *args, schedule='layered')
    diff = {n: int((_np(a) != b).sum()) for n, a, b in zip(
        ('ehat', 'status', 'choice', 'iters_used', 'bp_status', 'llr'), got[:5] + got[6:],
        host[:5] + host[6:])}
    print(code, B, dtype, 'elements differing from the host mirror:', diff,
          'pred elements differing:', int((_np(pred) != host[5]).sum()))
    assert not any(diff.values()), diff
    if dtype == 'float64':
        assert np.array_equal(_np(pred), host[5])
    ok = _np(bp) == 0
    assert ok.any() and (~ok).any()
    assert oc.satisfied(H, x, _np(ehat))[ok].all()
    assert oc.satisfied(H, x, _np(ehat))[_np(status) == 0].all()
    assert bool((choice[bp == 0] == -1).all())


def test_minsum_osd_decision_errors_end_to_end():
    """sample_toric (toric-5, p = 0.05, B = 256) -> layered minsum -> osd('cs', 10) ->
    decision_errors: no codeword keeps a residual syndrome, and where the layered minsum reports
    status 0 its own hard decision satisfies the syndrome; the one-call bposd agrees."""
    g = graph_of('toric_5')
    H = lc.code_matrix('toric_5')
    B = 256
    lg = torch.from_numpy(gd.codes.toric_logicals(H).astype(np.int32)).to(DEV)
    x, y = ops.sample_toric(g, B, [0.05], seed=11)
    pred, llr, its, status = layered(g, x, 12)
    ehat, ost, choice = ops.osd(g, x, pred, 'zero', 'cs', 10)
    assert int(ost.abs().sum()) == 0
    counts = ops.decision_errors(g, lg, ehat, y).tolist()
    assert counts[2] == 0
    st = status.cpu().numpy()
    assert set(st.tolist()) == {0, 1}
    ok = mc.satisfied(H, _np(x), _np(llr))
    assert np.array_equal(ok, st == 0)
    one = ops.bposd(g, x, 12, schedule='layered')
    assert int(one[1].abs().sum()) == 0
    assert ops.decision_errors(g, lg, one[0], y).tolist()[2] == 0
    hard = (llr.view(B, g.V) < 0).to(pred.dtype)
    on = status == 0
    assert torch.equal(one[0].view(B, g.V)[on], hard[on])


def test_capture_and_two_replays():
    """gnnd_minsum_layered and gnnd_bposd_layered only launch on the stream: captured once, two
    replays on changing inputs give the eager bits."""
    g = graph_of('toric_5')
    B = 258                                                  # not a multiple of 4
    xa, _ = ops.sample_toric(g, B, [0.03], seed=21)
    xb, _ = ops.sample_toric(g, B, [0.09], seed=22)
    ea = layered(g, xa, 12) + ops.bposd(g, xa, 12, schedule='layered')
    eb = layered(g, xb, 12) + ops.bposd(g, xb, 12, schedule='layered')
    sx = xa.clone()
    n = B * g.V
    real = lambda: torch.empty(n, 1, dtype=sx.dtype, device=DEV)
    ints = lambda: torch.empty(B, dtype=torch.int32, device=DEV)
    ms = (real(), real(), ints(), ints())
    bo = (real(), ints(), ints(), ints(), ints(), real(), real())
    work = torch.empty(B + 1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        layered(g, sx, 12, out=ms)
        ops.bposd(g, sx, 12, out=bo, work=work, schedule='layered')
    for src, eager in ((xb, eb), (xa, ea)):
        sx.copy_(src)
        for t in ms + bo:
            t.fill_(7)
        cg.replay()
        torch.cuda.synchronize()
        for a, b in zip(ms + bo, eager):
            assert torch.equal(a, b)


def test_traces_as_registered_ops():
    """gnnd::minsum_layered[_out] and gnnd::bposd_layered[_out] have fake kernels: shapes and
    dtypes without a launch, under FakeTensorMode and on the meta device; the real ops give the
    eager bits."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    g = graph_of('toric_5')
    V, N = g.V, g.N

    def check_ms(r, dt, device_type=None):
        pred, llr, its, status = r
        assert pred.shape == (3 * V, 1) and pred.dtype == dt
        assert llr.shape == (3 * V, 1) and llr.dtype == dt
        assert its.shape == (3,) and its.dtype == torch.int32
        assert status.shape == (3,) and status.dtype == torch.int32
        if device_type:
            assert all(t.device.type == device_type for t in r)

    def check_bp(r, dt, device_type=None):
        ehat, status, choice, its, bp, pred, llr = r
        for t in (ehat, pred, llr):
            assert t.shape == (3 * V, 1) and t.dtype == dt
        for t in (status, choice, its, bp):
            assert t.shape == (3,) and t.dtype == torch.int32
        if device_type:
            assert all(t.device.type == device_type for t in r)

    for dt in (torch.float32, torch.float64):
        with FakeTensorMode():
            x = torch.empty(3 * N, 1, dtype=dt, device=DEV)
            r = torch.ops.gnnd.minsum_layered(g.gid, x, 12, 0.75, 0.0, True)
            check_ms(r, dt)
            assert torch.ops.gnnd.minsum_layered_out(g.gid, x, 12, 0.75, 0.0, True, *r) is None
            r = torch.ops.gnnd.bposd_layered(g.gid, x, 12, 0.75, 0.0, True, 'zero', 'cs', 10)
            check_bp(r, dt)
            assert torch.ops.gnnd.bposd_layered_out(g.gid, x, 12, 0.75, 0.0, True, 'zero', 'cs',
                                                    10, *r) is None
        xm = torch.empty(3 * N, 1, dtype=dt, device='meta')
        check_ms(torch.ops.gnnd.minsum_layered(g.gid, xm, 12, 0.75, 0.0, True), dt, 'meta')
        check_bp(torch.ops.gnnd.bposd_layered(g.gid, xm, 12, 0.75, 0.0, True, 'zero', 'cs', 10),
                 dt, 'meta')
    alpha, beta, iters, early = lc.PARAMS[0]
    H, xs = lc.inputs('toric_5', 5, 'float64')
    ref_llr, ref_it, ref_st = lc.reference('toric_5', 5, 'float64', lc.PARAMS[0])
    xd = _dev(xs)
    r = torch.ops.gnnd.minsum_layered(g.gid, xd, iters, alpha, beta, True)
    assert np.array_equal(_np(r[1]), ref_llr) and np.array_equal(_np(r[2]), ref_it)
    out = tuple(torch.empty_like(t) for t in r)
    torch.ops.gnnd.minsum_layered_out(g.gid, xd, iters, alpha, beta, True, *out)
    assert all(torch.equal(a, b) for a, b in zip(out, r))
    eager = ops.bposd(g, xd, iters, alpha, beta, True, 'zero', 'cs', 10, schedule='layered')
    r = torch.ops.gnnd.bposd_layered(g.gid, xd, iters, alpha, beta, True, 'zero', 'cs', 10)
    assert all(torch.equal(a, b) for a, b in zip(r, eager))
    out = tuple(torch.empty_like(t) for t in r)
    torch.ops.gnnd.bposd_layered_out(g.gid, xd, iters, alpha, beta, True, 'zero', 'cs', 10, *out)
    assert all(torch.equal(a, b) for a, b in zip(out, eager))


def test_debug_library_runs_layered_clean():
    """toric-5 B = 67 (fp64) and LDPC B = 5 (fp32) under the bounds-checked build (GNND_LIB, a
    fresh child process): no index check fires and the bits are the numpy reference's."""
    res = debug_child.run('decoder_debug_worker.py', 'minsum_layered')
    assert res['equal'] == {'toric_5': True, 'ldpc_648_324': True}
