"""OSD-0 post-processing on the device (ops.osd0 -> gnnd_osd0) against the numpy statement of the
definition (tests/osd_cases.py), exact equality: the shapes where the one-wave-per-codeword plan
can go wrong (V not a multiple of 32, grid-stride tail and partial workgroups, more than one row
per lane, one wave per workgroup, a rank-deficient graph), decode -> osd0 -> decision_errors end
to end, stream capture, and the bounds-checked debug library."""
import numpy as np
import pytest
import torch

import gnndecode as gd
from gnndecode import ops

import debug_child
import osd_cases as oc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

# toric-5: V = 100 (not a multiple of 32), B = 1 / 5 / 67: one wave, a partial workgroup, 16 full
# workgroups + a 3-wave tail; toric-7: C = 96, two rows per lane; BCH: V = 63 (one column word and
# a bit to spare); LDPC: 6 rows per lane, one wave per workgroup; bch_dup: C = 19, rank 18
SHAPES = [('toric_5', 1), ('toric_5', 5), ('toric_5', 67), ('toric_7', 9), ('bch_63_45', 33),
          ('ldpc_648_324', 3), ('bch_dup', 4)]

_GRAPHS = {}


def graph_of(code):
    if code not in _GRAPHS:
        _GRAPHS[code] = gd.TannerGraph(oc.code_matrix(code), device=DEV)
    return _GRAPHS[code]


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('base', ['zero', 'hard'])
@pytest.mark.parametrize('code,B', SHAPES)
def test_osd0_equals_reference(code, B, base, dtype):
    H, x, p = oc.inputs(code, B, dtype)
    ref_e, ref_s = oc.reference(code, B, dtype, base)
    g = graph_of(code)
    xd = torch.from_numpy(x.copy()).to(DEV).unsqueeze(1)
    pd = torch.from_numpy(p.copy()).to(DEV).unsqueeze(1)
    ehat, status = ops.osd0(g, xd, pd, base)
    assert ehat.shape == pd.shape and ehat.dtype == pd.dtype
    assert status.shape == (B,) and status.dtype == torch.int32
    got_e, got_s = ehat.cpu().numpy().reshape(B, -1), status.cpu().numpy()
    assert np.isin(got_e, (0.0, 1.0)).all()
    assert np.array_equal(got_s, ref_s)
    assert np.array_equal(got_e, ref_e)
    assert oc.satisfied(H, x, got_e)[got_s == 0].all()
    if code == 'bch_dup':
        assert got_s.tolist() == [1, 0] * (B // 2)
    else:
        assert not got_s.any()
    # the same bits as the host mirror, and into caller-owned outputs
    host_e, host_s = ops.osd0_host(H, x, p, base)
    assert np.array_equal(host_e.reshape(B, -1), got_e) and np.array_equal(host_s, got_s)
    out = (torch.full_like(pd, 7), torch.full((B,), 7, dtype=torch.int32, device=DEV))
    r = ops.osd0(g, xd, pd, base, out=out)
    assert r[0] is out[0] and r[1] is out[1]
    assert torch.equal(out[0], ehat) and torch.equal(out[1], status)


def test_empty_batch_and_bad_arguments():
    g = graph_of('toric_5')
    x = torch.empty(0, 1, dtype=torch.float64, device=DEV)
    ehat, status = ops.osd0(g, x, x.clone())
    assert ehat.numel() == 0 and status.numel() == 0
    xd = torch.zeros(g.N, 1, dtype=torch.float64, device=DEV)
    pd = torch.zeros(g.V, 1, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        ops.osd0(g, xd, pd, 'soft')
    with pytest.raises(ValueError):
        ops.osd0(g, xd[:-1], pd)
    with pytest.raises(TypeError):
        ops.osd0(g, xd, pd.float())
    with pytest.raises(TypeError):
        ops.osd0(g, xd.bfloat16(), pd.bfloat16())
    with pytest.raises(RuntimeError):
        ops.osd0(g, xd.cpu(), pd.cpu())


def _decode_qbp(g, B=256, seed=11):
    x, y = ops.sample_toric(g, B, [0.05], seed=seed)
    return x, y, ops.decode(g, 'qbp', x, 10)


@pytest.mark.parametrize('base', ['zero', 'hard'])
def test_decode_osd0_decision_errors_end_to_end(base):
    """sample_toric (toric-5, p = 0.05, B = 256) -> decode qbp T = 10 -> osd0: every status 0, no
    codeword with a residual syndrome, and the bits of the reference applied to the device's
    pred.  (Logical failures are not asserted: recorded by tools/osd_bench.py.)"""
    g = graph_of('toric_5')
    H = oc.code_matrix('toric_5')
    lg = torch.from_numpy(gd.codes.toric_logicals(H).astype(np.int32)).to(DEV)
    x, y, pred = _decode_qbp(g)
    ehat, status = ops.osd0(g, x, pred, base)
    assert int(status.abs().sum()) == 0
    counts = ops.decision_errors(g, lg, ehat, y).tolist()
    assert counts[2] == 0
    ref_e, ref_s = oc.ref_batch(H, x.cpu().numpy().reshape(-1), pred.cpu().numpy().reshape(-1),
                                base == 'hard')
    assert not ref_s.any()
    assert np.array_equal(ehat.cpu().numpy().reshape(256, -1), ref_e)


def test_decode_and_osd0_in_one_capture():
    """gnnd_osd0 only launches on the stream: captured behind a decode, one replay gives the eager
    bits."""
    g = graph_of('toric_5')
    x, y, pred = _decode_qbp(g, seed=12)
    eager = [ops.osd0(g, x, pred, b) for b in ('zero', 'hard')]
    sx = x.clone()
    spred = torch.empty_like(pred)
    outs = [(torch.empty_like(pred), torch.empty(256, dtype=torch.int32, device=DEV))
            for _ in range(2)]
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.decode(g, 'qbp', sx, 10, out=spred)
        ops.osd0(g, sx, spred, 'zero', out=outs[0])
        ops.osd0(g, sx, spred, 'hard', out=outs[1])
    for o in outs:
        o[0].fill_(7)
        o[1].fill_(7)
    spred.fill_(7)
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(spred, pred)
    for (e, s), (ee, es) in zip(outs, eager):
        assert torch.equal(e, ee) and torch.equal(s, es)


def test_osd0_traces_as_registered_op():
    """gnnd::osd0 has a fake kernel: it propagates shapes without a launch, like gnnd::decode."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    g = graph_of('toric_5')
    with FakeTensorMode():
        x = torch.empty(3 * g.N, 1, dtype=torch.float64, device=DEV)
        p = torch.empty(3 * g.V, 1, dtype=torch.float64, device=DEV)
        ehat, status = torch.ops.gnnd.osd0(g.gid, x, p, 'zero')
        assert ehat.shape == (3 * g.V, 1) and ehat.dtype == torch.float64
        assert status.shape == (3,) and status.dtype == torch.int32
    H, xs, ps = oc.inputs('toric_5', 5, 'float64')
    xd, pd = torch.from_numpy(xs.copy()).to(DEV), torch.from_numpy(ps.copy()).to(DEV)
    ehat, status = torch.ops.gnnd.osd0(g.gid, xd, pd, 'hard')
    ref_e, ref_s = oc.reference('toric_5', 5, 'float64', 'hard')
    assert np.array_equal(ehat.cpu().numpy().reshape(5, -1), ref_e)
    assert np.array_equal(status.cpu().numpy(), ref_s)


def test_debug_library_runs_osd0_clean():
    """One toric-5 case under the bounds-checked build (GNND_LIB, a fresh child process): no
    index check fires and the bits are the reference's."""
    res = debug_child.run('decoder_debug_worker.py', 'osd')
    assert res['equal'] == {'zero': True, 'hard': True}
