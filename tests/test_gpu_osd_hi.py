"""Higher-order OSD post-processing on the device (ops.osd -> gnnd_osd) against the numpy statement
of the definition (tests/osd_hi_cases.py) and the host mirror, exact equality of estimate, status
and chosen candidate index: the shapes of tests/test_gpu_osd.py (V not a multiple of 32, partial
workgroups and the grid-stride tail, one row per lane with the ballot count and several with the
cross-lane sum, one wave per workgroup, a rank-deficient graph), decode -> osd -> decision_errors
end to end, stream capture, the registered op, and the bounds-checked debug library."""
import numpy as np
import pytest
import torch

import gnndecode as gd
from gnndecode import _lib, ops

import debug_child
import osd_hi_cases as hc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

# toric-5 in both bases and dtypes; elsewhere one dtype per base.  toric-7: two rows per lane (the
# cross-lane sum), F = 100 so (cs, 64) is unclamped: 2016 pairs; BCH: C <= 64, the ballot count;
# LDPC: six rows per lane, one wave per workgroup, 324 singles; bch_dup: failures between successes
CASES = ([('toric_5', B, base, dtype) for B in (1, 5, 67) for base in ('zero', 'hard')
          for dtype in ('float32', 'float64')]
         + [('toric_7', 9, 'zero', 'float64'), ('toric_7', 9, 'hard', 'float32'),
            ('bch_63_45', 33, 'zero', 'float32'), ('bch_63_45', 33, 'hard', 'float64'),
            ('ldpc_648_324', 3, 'zero', 'float32'), ('ldpc_648_324', 3, 'hard', 'float64'),
            ('bch_dup', 4, 'zero', 'float64'), ('bch_dup', 4, 'hard', 'float32')])

_GRAPHS = {}


def graph_of(code):
    if code not in _GRAPHS:
        _GRAPHS[code] = gd.TannerGraph(hc.code_matrix(code), device=DEV)
    return _GRAPHS[code]


def _device_inputs(code, B, dtype):
    H, x, p = hc.inputs(code, B, dtype)
    xd = torch.from_numpy(x.copy()).to(DEV).unsqueeze(1)
    pd = torch.from_numpy(p.copy()).to(DEV).unsqueeze(1)
    return H, x, p, xd, pd


@pytest.mark.parametrize('code,B,base,dtype', CASES)
def test_osd_equals_reference_and_host(code, B, base, dtype):
    H, x, p, xd, pd = _device_inputs(code, B, dtype)
    g = graph_of(code)
    e0, s0 = ops.osd0(g, xd, pd, base)
    for method, order in hc.METHODS:
        tag = (method, order)
        ref_e, ref_s, ref_c = hc.reference(code, B, dtype, base, method, order)
        ehat, status, choice = ops.osd(g, xd, pd, base, method, order)
        assert ehat.shape == pd.shape and ehat.dtype == pd.dtype, tag
        assert status.shape == (B,) and status.dtype == torch.int32, tag
        assert choice.shape == (B,) and choice.dtype == torch.int32, tag
        got_e, got_s, got_c = (ehat.cpu().numpy().reshape(B, -1), status.cpu().numpy(),
                               choice.cpu().numpy())
        assert np.isin(got_e, (0.0, 1.0)).all(), tag
        assert np.array_equal(got_s, ref_s), tag
        assert np.array_equal(got_c, ref_c), tag
        assert np.array_equal(got_e, ref_e), tag
        assert hc.satisfied(H, x, got_e)[got_s == 0].all(), tag
        assert not got_c[got_s != 0].any(), tag
        host_e, host_s, host_c = ops.osd_host(H, x, p, base, method, order)
        assert np.array_equal(host_e.reshape(B, -1), got_e), tag
        assert np.array_equal(host_s, got_s) and np.array_equal(host_c, got_c), tag
        if method == 'osd0':
            assert torch.equal(ehat, e0) and torch.equal(status, s0) and not got_c.any()
    if code == 'bch_dup':
        assert s0.tolist() == [1, 0] * (B // 2)
    else:
        assert not s0.any()


@pytest.mark.parametrize('method,order', [('cs', 10), ('e', 8)])
def test_out_forms_and_null_choice(method, order):
    """out = (ehat, status, choice) writes into the caller's tensors; out = (ehat, status) passes
    d_choice = NULL: the same ehat and status, no choice."""
    code, B, dtype, base = 'toric_5', 67, 'float64', 'zero'
    H, x, p, xd, pd = _device_inputs(code, B, dtype)
    g = graph_of(code)
    ehat, status, choice = ops.osd(g, xd, pd, base, method, order)
    out = (torch.full_like(pd, 7), torch.full((B,), 7, dtype=torch.int32, device=DEV),
           torch.full((B,), 7, dtype=torch.int32, device=DEV))
    r = ops.osd(g, xd, pd, base, method, order, out=out)
    assert all(a is b for a, b in zip(r, out))
    assert torch.equal(out[0], ehat) and torch.equal(out[1], status) and torch.equal(out[2], choice)
    out2 = (torch.full_like(pd, 7), torch.full((B,), 7, dtype=torch.int32, device=DEV))
    r = ops.osd(g, xd, pd, base, method, order, out=out2)
    assert r[0] is out2[0] and r[1] is out2[1] and r[2] is None
    assert torch.equal(out2[0], ehat) and torch.equal(out2[1], status)
    # and straight through the C ABI
    e3, s3 = torch.full_like(pd, 7), torch.full((B,), 7, dtype=torch.int32, device=DEV)
    st = _lib.get().gnnd_osd(g.handle, _lib.F64, xd.data_ptr(), pd.data_ptr(), 0,
                             _lib.OSD_METHOD[method], order, e3.data_ptr(), s3.data_ptr(), None, B,
                             ops.current_stream(pd.device))
    assert st == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(e3, ehat) and torch.equal(s3, status)


def test_empty_batch_and_bad_arguments():
    g = graph_of('toric_5')
    x = torch.empty(0, 1, dtype=torch.float64, device=DEV)
    ehat, status, choice = ops.osd(g, x, x.clone())
    assert ehat.numel() == 0 and status.numel() == 0 and choice.numel() == 0
    xd = torch.zeros(g.N, 1, dtype=torch.float64, device=DEV)
    pd = torch.zeros(g.V, 1, dtype=torch.float64, device=DEV)
    for kw in ({'base': 'soft'}, {'method': 'osd1'}, {'order': -1}, {'method': 'osd0', 'order': -1},
               {'method': 'cs', 'order': 65}, {'method': 'e', 'order': 13}):
        with pytest.raises(ValueError):
            ops.osd(g, xd, pd, **kw)
    with pytest.raises(ValueError):
        ops.osd(g, xd[:-1], pd)
    with pytest.raises(TypeError):
        ops.osd(g, xd, pd.float())
    with pytest.raises(TypeError):
        ops.osd(g, xd.bfloat16(), pd.bfloat16())
    with pytest.raises(RuntimeError):
        ops.osd(g, xd.cpu(), pd.cpu())
    # the C entry point itself, with a real graph
    lib = _lib.get()
    e, s = torch.empty_like(pd), torch.empty(1, dtype=torch.int32, device=DEV)

    def dev(dtype=_lib.F64, method=1, order=10):
        return lib.gnnd_osd(g.handle, dtype, xd.data_ptr(), pd.data_ptr(), 0, method, order,
                            e.data_ptr(), s.data_ptr(), None, 1, None)

    assert dev(order=-1) == _lib.ERR_INVALID_ARG and dev(method=0, order=-1) == _lib.ERR_INVALID_ARG
    assert dev(order=65) == _lib.ERR_INVALID_ARG and dev(method=2, order=13) == _lib.ERR_INVALID_ARG
    assert dev(method=3) == _lib.ERR_INVALID_ARG
    assert dev(dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED


def _decode_qbp(g, B=256, seed=11):
    x, y = ops.sample_toric(g, B, [0.05], seed=seed)
    return x, y, ops.decode(g, 'qbp', x, 10)


def test_decode_osd_decision_errors_end_to_end():
    """sample_toric (toric-5, p = 0.05, B = 256) -> decode qbp T = 10 -> osd(cs, 10): every status
    0, no codeword with a residual syndrome, the reference's bits on the device's pred, and a
    summed estimate weight no larger than OSD-0's on the same batch."""
    g = graph_of('toric_5')
    H = hc.code_matrix('toric_5')
    lg = torch.from_numpy(gd.codes.toric_logicals(H).astype(np.int32)).to(DEV)
    x, y, pred = _decode_qbp(g)
    ehat, status, choice = ops.osd(g, x, pred, 'zero', 'cs', 10)
    assert int(status.abs().sum()) == 0
    counts = ops.decision_errors(g, lg, ehat, y).tolist()
    assert counts[2] == 0
    e0, _ = ops.osd0(g, x, pred, 'zero')
    w, w0 = float(ehat.sum()), float(e0.sum())
    print(f'estimate weight: osd(cs, 10) {w}, osd0 {w0}; choices != 0: {int(choice.ne(0).sum())}')
    assert w <= w0
    assert bool((ehat.view(256, -1).sum(1) <= e0.view(256, -1).sum(1)).all())
    ref_e, ref_s, ref_c = hc.ref_batch(H, x.cpu().numpy().reshape(-1),
                                       pred.cpu().numpy().reshape(-1), False, 'cs', 10)
    assert not ref_s.any()
    assert np.array_equal(ehat.cpu().numpy().reshape(256, -1), ref_e)
    assert np.array_equal(choice.cpu().numpy(), ref_c)


def test_decode_and_osd_in_one_capture():
    """gnnd_osd only launches on the stream: captured behind a decode, one replay gives the eager
    bits."""
    g = graph_of('toric_5')
    x, y, pred = _decode_qbp(g, seed=12)
    eager = ops.osd(g, x, pred, 'zero', 'cs', 10)
    sx = x.clone()
    spred = torch.empty_like(pred)
    out = (torch.empty_like(pred), torch.empty(256, dtype=torch.int32, device=DEV),
           torch.empty(256, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.decode(g, 'qbp', sx, 10, out=spred)
        ops.osd(g, sx, spred, 'zero', 'cs', 10, out=out)
    for o in out:
        o.fill_(7)
    spred.fill_(7)
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(spred, pred)
    for a, b in zip(out, eager):
        assert torch.equal(a, b)


def test_osd_traces_as_registered_op():
    """gnnd::osd has a fake kernel: it propagates shapes without a launch, like gnnd::osd0; called
    for real it gives the reference's bits, and gnnd::osd_out writes its outputs."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    g = graph_of('toric_5')
    with FakeTensorMode():
        x = torch.empty(3 * g.N, 1, dtype=torch.float64, device=DEV)
        p = torch.empty(3 * g.V, 1, dtype=torch.float64, device=DEV)
        ehat, status, choice = torch.ops.gnnd.osd(g.gid, x, p, 'zero', 'cs', 10)
        assert ehat.shape == (3 * g.V, 1) and ehat.dtype == torch.float64
        assert status.shape == (3,) and status.dtype == torch.int32
        assert choice.shape == (3,) and choice.dtype == torch.int32
    H, xs, ps = hc.inputs('toric_5', 5, 'float64')
    xd, pd = torch.from_numpy(xs.copy()).to(DEV), torch.from_numpy(ps.copy()).to(DEV)
    ref = hc.reference('toric_5', 5, 'float64', 'hard', 'e', 8)
    got = torch.ops.gnnd.osd(g.gid, xd, pd, 'hard', 'e', 8)
    for a, r in zip(got, ref):
        assert np.array_equal(a.cpu().numpy().reshape(r.shape), r)
    out = (torch.empty_like(pd), torch.empty(5, dtype=torch.int32, device=DEV),
           torch.empty(5, dtype=torch.int32, device=DEV))
    torch.ops.gnnd.osd_out(g.gid, xd, pd, 'hard', 'e', 8, *out)
    for a, b in zip(out, got):
        assert torch.equal(a, b)


def test_debug_library_runs_osd_clean():
    """(cs, 10) and (e, 8) on toric-7 and the rank-deficient graph under the bounds-checked build
    (GNND_LIB, a fresh child process): no index check fires and the bits are the reference's."""
    res = debug_child.run('decoder_debug_worker.py', 'osd_hi')
    assert res['equal'] == {'toric_7_cs': True, 'toric_7_e': True, 'bch_dup_cs': True,
                            'bch_dup_e': True}
