"""Gated OSD and BP+OSD on the device (ops.osd_gated -> gnnd_osd_gated, ops.bposd -> gnnd_bposd)
against the numpy statement (tests/bposd_cases.py) and the host mirrors, exact equality: the shapes
where the compaction and the list-driven plan can go wrong (count 0, count B, a partial workgroup
of list entries, two rows per lane, C < 64, one wave per workgroup, failures between successes, a
batch beyond the grid cap), every output element written for every gate, the tiny-LLR case,
sample_toric -> bposd -> decision_errors, stream capture with the gated count changing between
replays, the registered ops and the bounds-checked debug library."""
import ctypes

import numpy as np
import pytest
import torch

import gnndecode as gd
from gnndecode import _lib, ops

import bposd_cases as bc
import debug_child
import minsum_cases as mc
import osd_cases as oc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

# toric-5 B = 1 (count 0, then count 1), 5 (a partial workgroup) and 67 (16 workgroups and a tail
# at count B, fewer list entries than waves in flight under the mixed gates); toric-7: C = 96, two
# rows per lane; BCH: C = 18 < 64; LDPC: one wave per workgroup; bch_dup: rank-deficient
CASES = ([('toric_5', B, dt) for B in (1, 5, 67) for dt in ('float32', 'float64')]
         + [('toric_7', 9, 'float64'), ('bch_63_45', 33, 'float32'),
            ('ldpc_648_324', 3, 'float32'), ('ldpc_648_324', 3, 'float64')])

_GRAPHS = {}


def graph_of(code):
    if code not in _GRAPHS:
        _GRAPHS[code] = gd.TannerGraph(oc.code_matrix(code), device=DEV)
    return _GRAPHS[code]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def _np(t):
    return t.cpu().numpy().reshape(-1)


def _same(got, ref, B, V):
    assert np.array_equal(_np(got[0]).reshape(B, V), ref[0].astype(_np(got[0]).dtype))
    assert np.array_equal(_np(got[1]), ref[1]) and np.array_equal(_np(got[2]), ref[2])


def _gates(code, B, dtype):
    names = ('zeros', 'ones') if B == 1 else bc.GATES
    return [(n, bc.gate(code, B, dtype, n)) for n in names]


@pytest.mark.parametrize('code,B,dtype', CASES)
def test_osd_gated_equals_reference_and_host(code, B, dtype):
    H, x, p = oc.inputs(code, B, dtype)
    V = H.shape[0]
    g = graph_of(code)
    xd, pd, Ld = _dev(x).unsqueeze(1), _dev(p).unsqueeze(1), _dev(bc.llr_input(code, B, dtype))
    base = 'zero' if code.startswith('toric') else 'hard'
    for method, order in (('cs', 10), ('e', 8)) if B == 67 else (('cs', 10),):
        for name, gate in _gates(code, B, dtype):
            for with_llr in (True, False):
                ehat = torch.full_like(pd, 7)               # poisoned: every element is written
                status = torch.full((B,), 7, dtype=torch.int32, device=DEV)
                choice = torch.full((B,), 7, dtype=torch.int32, device=DEV)
                got = ops.osd_gated(g, xd, pd, _dev(gate), base, method, order,
                                    llr=Ld if with_llr else None, out=(ehat, status, choice))
                assert got[0] is ehat and got[1] is status and got[2] is choice
                _same(got, bc.gated_reference(code, B, dtype, base, method, order, name, with_llr),
                      B, V)
                host = ops.osd_gated_host(H, x, p, gate, base, method, order,
                                          llr=bc.llr_input(code, B, dtype) if with_llr else None)
                for a, b in zip(got, host):
                    assert np.array_equal(_np(a), b)
        full = ops.osd(g, xd, pd, base, method, order)
        ones = ops.osd_gated(g, xd, pd, torch.ones(B, dtype=torch.int32, device=DEV), base, method,
                             order)
        for a, b in zip(ones, full):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize('base,dtype', [('zero', 'float64'), ('hard', 'float32')])
def test_rank_deficient_graph(base, dtype):
    B = 4
    H, x, p = oc.inputs('bch_dup', B, dtype)
    V = H.shape[0]
    g = graph_of('bch_dup')
    xd, pd = _dev(x), _dev(p)
    for gate in ([1, 0, 1, 0], [0, 1, 0, 1], [1, 1, 1, 1]):
        gn = np.array(gate, np.int32)
        for method, order in (('cs', 10), ('e', 8)):
            got = ops.osd_gated(g, xd, pd, _dev(gn), base, method, order)
            host = ops.osd_gated_host(H, x, p, gn, base, method, order)
            for a, b in zip(got, host):
                assert np.array_equal(_np(a), b)
            assert _np(got[1]).tolist() == [a & b for a, b in zip(gate, [1, 0, 1, 0])]


def test_batch_beyond_the_grid_cap():
    """toric-5 fp32 B = 9 001 (the osd grid holds 8 192 waves, the compaction strides three chunks)
    with a min-sum gate: gated rows are the rows of the ungated osd, the others the hard decision
    of llr."""
    B = 9001
    g = graph_of('toric_5')
    V = g.V
    x, y = ops.sample_toric(g, B, [0.02, 0.06, 0.10], seed=5, dtype=torch.float32)
    pred, llr, its, gate = ops.minsum(g, x, 10)
    n = int(gate.sum())
    assert 0 < n < B
    full = ops.osd(g, x, pred, 'zero', 'cs', 10)
    got = ops.osd_gated(g, x, pred, gate, 'zero', 'cs', 10, llr=llr)
    on = gate != 0
    hard = (llr.view(B, V) < 0).to(pred.dtype)
    assert torch.equal(got[0].view(B, V)[on], full[0].view(B, V)[on])
    assert torch.equal(got[1][on], full[1][on]) and torch.equal(got[2][on], full[2][on])
    assert torch.equal(got[0].view(B, V)[~on], hard[~on])
    assert int(got[1][~on].abs().sum()) == 0 and bool((got[2][~on] == -1).all())


BPOSD_CASES = [('toric_5', 67, 'float32'), ('toric_5', 67, 'float64'), ('toric_5', 5, 'float64'),
               ('toric_7', 9, 'float64'), ('bch_63_45', 33, 'float32'),
               ('ldpc_648_324', 3, 'float32')]


def _bposd_case(code, B, dtype):
    alpha, beta, iters, early = bc.bp_params(code)
    H, x = mc.inputs(code, B, dtype)
    base = 'zero' if code.startswith('toric') else 'hard'
    return H, x, (iters, alpha, beta, bool(early), base, 'cs', 10)


@pytest.mark.parametrize('code,B,dtype', BPOSD_CASES)
def test_bposd_equals_its_two_stages_and_reference(code, B, dtype):
    """bposd is minsum followed by osd_gated bit for bit; it equals the numpy statement, and the
    host mirror wherever the contract fixes the bits: llr, iters_used and bp_status outright, and
    ehat / status / choice for the soft output the device returned (the OSD stage orders its
    columns by pred, whose exponential is each library's own)."""
    H, x, args = _bposd_case(code, B, dtype)
    V = H.shape[0]
    g = graph_of(code)
    xd = _dev(x).unsqueeze(1)
    ehat, status, choice, its, bp, pred, llr = ops.bposd(g, xd, *args)
    assert ehat.shape == (B * V, 1) and ehat.dtype == xd.dtype
    m = ops.minsum(g, xd, *args[:4])
    o = ops.osd_gated(g, xd, m[0], m[3], *args[4:], llr=m[1])
    for a, b in zip((pred, llr, its, bp, ehat, status, choice), m + o):
        assert np.array_equal(_np(a), _np(b), equal_nan=True)
    r_e, r_s, r_c, r_it, r_bp, r_llr = bc.bposd_reference(code, B, dtype, _np(pred), *args[4:])
    assert np.array_equal(_np(llr), r_llr) and np.array_equal(_np(its), r_it)
    assert np.array_equal(_np(bp), r_bp)
    np.testing.assert_allclose(_np(pred), mc.soft_output(r_llr), **mc.pred_tolerance(dtype))
    _same((ehat, status, choice), (r_e, r_s, r_c), B, V)
    host = ops.bposd_host(H, x, *args)
    for a, b in zip((its, bp, llr), host[3:5] + host[6:]):
        assert np.array_equal(_np(a), b)
    np.testing.assert_allclose(_np(pred), host[5], **mc.pred_tolerance(dtype))
    h2 = ops.osd_gated_host(H, x, _np(pred), _np(bp), *args[4:], llr=_np(llr))
    for a, b in zip((ehat, status, choice), h2):
        assert np.array_equal(_np(a), b)
    ok = _np(bp) == 0
    assert oc.satisfied(H, x, _np(ehat))[ok].all()
    assert oc.satisfied(H, x, _np(ehat))[_np(status) == 0].all()


@pytest.mark.parametrize('code,B,dtype', BPOSD_CASES)
def test_bposd_equals_host_mirror(code, B, dtype):
    """Every output but pred equals gnnd_bposd_host's, ehat / status / choice included; in fp64
    pred does too.  The OSD stage orders its columns by pred, so this needs the mirror's pred to
    be the device's: in fp64 the kernel's exponential is the project's own fixed sequence of
    fused multiply-adds, which gnnd_bposd_host repeats operation for operation.  In fp32 the
    device calls its math library's expf, which the host cannot repeat: pred then differs in the
    last place in some elements and the contract does not promise equal estimates, but on these
    inputs no column order depends on those elements and the comparison holds."""
    H, x, args = _bposd_case(code, B, dtype)
    got = ops.bposd(graph_of(code), _dev(x).unsqueeze(1), *args)
    host = ops.bposd_host(H, x, *args)
    diff = {n: int((_np(a) != b).sum()) for n, a, b in zip(
        ('ehat', 'status', 'choice', 'iters_used', 'bp_status', 'llr'), got[:5] + got[6:],
        host[:5] + host[6:])}
    V = H.shape[0]
    print(code, B, dtype, 'elements differing from the host mirror:', diff,
          'codewords with a differing ehat:',
          int((_np(got[0]).reshape(B, V) != host[0].reshape(B, V)).any(1).sum()),
          'pred elements differing:', int((_np(got[5]) != host[5]).sum()))
    assert not any(diff.values()), diff
    if dtype == 'float64':
        assert np.array_equal(_np(got[5]), host[5])


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_tiny_llr_on_the_device(dtype):
    alpha, beta, iters, early = bc.TINY_BP
    H, x, xs = bc.tiny_llr_inputs(dtype)
    V, C = H.shape
    B = x.size // (V + C)
    g = graph_of('toric_5')
    big = ops.minsum(g, _dev(x), iters, alpha, beta, True)
    ehat, status, choice, its, bp, pred, llr = ops.bposd(g, _dev(xs), iters, alpha, beta, True,
                                                         'zero', 'cs', 10)
    assert torch.equal(its, big[2]) and torch.equal(bp, big[3])
    assert bool((pred == 0.5).all())
    ok = _np(bp) == 0
    assert ok.any() and (~ok).any()
    e = _np(ehat).reshape(B, V)
    assert np.array_equal(e[ok], (_np(llr).reshape(B, V)[ok] < 0).astype(e.dtype)) and e[ok].any()
    assert oc.satisfied(H, xs, _np(ehat))[ok].all()
    assert oc.satisfied(H, xs, _np(ehat))[_np(status) == 0].all()
    host = ops.bposd_host(H, xs, iters, alpha, beta, True, 'zero', 'cs', 10)
    for a, b in zip((ehat, status, choice, its, bp, pred, llr), host):
        assert np.array_equal(_np(a), b)
    blind = ops.osd_gated(g, _dev(xs), pred, bp, 'zero', 'cs', 10)
    assert not _np(blind[0]).reshape(B, V)[ok].any()


def test_out_forms_null_outputs_work_and_raw_abi():
    alpha, beta, iters, early = bc.bp_params('toric_5')
    B, dtype = 67, 'float64'
    H, x = mc.inputs('toric_5', B, dtype)
    g = graph_of('toric_5')
    xd = _dev(x)
    ref = ops.bposd(g, xd, iters, alpha, beta, True, 'zero', 'cs', 10)

    def fresh():
        real = lambda: torch.full((B * g.V, 1), 7, dtype=xd.dtype, device=DEV)
        ints = lambda: torch.full((B,), 7, dtype=torch.int32, device=DEV)
        return [real(), ints(), ints(), ints(), ints(), real(), real()]

    out = fresh()
    r = ops.bposd(g, xd, iters, alpha, beta, True, 'zero', 'cs', 10, out=out)
    assert all(a is b for a, b in zip(r, out))
    assert all(torch.equal(a, b) for a, b in zip(out, ref))
    # choice and iters_used skipped, a caller-supplied scratch (larger than needed, int32)
    out = fresh()
    keep = (out[2], out[3])
    out[2] = out[3] = None
    work = torch.empty(B + 9, dtype=torch.int32, device=DEV)
    r = ops.bposd(g, xd, iters, alpha, beta, True, 'zero', 'cs', 10, out=out, work=work)
    assert r[2] is None and r[3] is None
    assert all(torch.equal(a, b) for a, b in zip(out, ref) if a is not None)
    assert all(bool((k == 7).all()) for k in keep)
    with pytest.raises(ValueError):
        ops.bposd(g, xd, iters, alpha, beta, True, out=fresh(),
                  work=torch.empty(B, dtype=torch.int32, device=DEV))
    pred, llr, bp = ref[5], ref[6], ref[4]
    og = ops.osd_gated(g, xd, pred, bp, 'zero', 'cs', 10, llr=llr, work=work)
    assert all(torch.equal(a, b) for a, b in zip(og, ref[:3]))
    two = (torch.full_like(pred, 7), torch.full_like(bp, 7))
    r = ops.osd_gated(g, xd, pred, bp, 'zero', 'cs', 10, llr=llr, out=two)
    assert r[2] is None and torch.equal(two[0], ref[0]) and torch.equal(two[1], ref[1])
    # the raw C calls
    lib = _lib.get()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = ops.osd_gated_workspace(B)
    assert need == 4 * (B + 1)
    out = fresh()
    torch.cuda.synchronize()
    assert lib.gnnd_bposd(g.handle, _lib.F64, p(xd), alpha, beta, iters, 1, 0, 1, 10, p(out[5]),
                          p(out[6]), p(out[3]), p(out[4]), p(out[0]), p(out[1]), p(out[2]), p(work),
                          need - 1, B, st) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_osd_gated(g.handle, _lib.F64, p(xd), p(pred), p(llr), p(bp), 0, 1, 10, p(out[0]),
                              p(out[1]), p(out[2]), p(work), need - 1, B,
                              st) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)           # nothing was launched
    assert lib.gnnd_bposd(g.handle, _lib.F64, p(xd), alpha, beta, iters, 1, 0, 1, 10, p(out[5]),
                          p(out[6]), p(out[3]), p(out[4]), p(out[0]), p(out[1]), p(out[2]), p(work),
                          need, B, st) == _lib.OK
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, ref))
    out = fresh()
    assert lib.gnnd_osd_gated(g.handle, _lib.F64, p(xd), p(pred), p(llr), p(bp), 0, 1, 10, p(out[0]),
                              p(out[1]), None, p(work), need, B, st) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
    assert bool((out[2] == 7).all())


def test_empty_batch_unsupported_graph_and_bad_arguments():
    g = graph_of('toric_5')
    empty = torch.empty(0, 1, dtype=torch.float64, device=DEV)
    r = ops.bposd(g, empty, 5)
    assert all(t.numel() == 0 for t in r)
    r = ops.osd_gated(g, empty, empty, torch.empty(0, dtype=torch.int32, device=DEV))
    assert all(t.numel() == 0 for t in r)
    Hd = np.zeros((3, 2), np.uint8)                         # a check of degree 1: min-sum refuses
    Hd[[0, 1, 2, 2], [0, 0, 0, 1]] = 1
    gdeg = gd.TannerGraph(Hd, device=DEV)
    with pytest.raises(_lib.GnndError) as e:
        ops.bposd(gdeg, torch.zeros(5, dtype=torch.float64, device=DEV), 5)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    xd = torch.zeros(g.N, 1, dtype=torch.float64, device=DEV)
    pd = torch.zeros(g.V, 1, dtype=torch.float64, device=DEV)
    gt = torch.zeros(1, dtype=torch.int32, device=DEV)
    for kw in ({'base': 'soft'}, {'method': 'x'}, {'order': 65}):
        with pytest.raises(ValueError):
            ops.osd_gated(g, xd, pd, gt, **kw)
        with pytest.raises(ValueError):
            ops.bposd(g, xd, 5, **kw)
    with pytest.raises(ValueError):
        ops.bposd(g, xd, 0)
    with pytest.raises(ValueError):
        ops.osd_gated(g, xd, pd, torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        ops.osd_gated(g, xd, pd, gt.long())
    with pytest.raises(TypeError):
        ops.osd_gated(g, xd, pd, gt, llr=pd.float())
    with pytest.raises(TypeError):
        ops.bposd(g, xd.bfloat16(), 5)
    with pytest.raises(RuntimeError):
        ops.bposd(g, xd.cpu(), 5)
    with pytest.raises(RuntimeError):
        ops.osd_gated(g, xd, pd, gt.cpu())


def test_sample_bposd_decision_errors_end_to_end():
    g = graph_of('toric_5')
    H = oc.code_matrix('toric_5')
    B = 256
    lg = torch.from_numpy(gd.codes.toric_logicals(H).astype(np.int32)).to(DEV)
    x, y = ops.sample_toric(g, B, [0.05], seed=11)
    ehat, status, choice, its, bp, pred, llr = ops.bposd(g, x, 12)
    assert int(status.abs().sum()) == 0
    counts = ops.decision_errors(g, lg, ehat, y).tolist()
    assert counts[2] == 0
    assert set(bp.cpu().tolist()) == {0, 1}
    assert bool((choice[bp == 0] == -1).all()) and bool((choice[bp != 0] >= 0).all())


def test_capture_follows_the_gate_at_replay():
    """bposd captured once; the input changes between the replays so that the gated count does:
    each replay gives the eager bits of its input (the count is read on the device)."""
    g = graph_of('toric_5')
    B = 256
    xa, _ = ops.sample_toric(g, B, [0.03], seed=21)
    xb, _ = ops.sample_toric(g, B, [0.09], seed=22)
    ea = ops.bposd(g, xa, 12)
    eb = ops.bposd(g, xb, 12)
    na, nb = int(ea[4].sum()), int(eb[4].sum())
    assert na != nb and 0 < na and 0 < nb
    sx = xa.clone()
    n = B * g.V
    real = lambda: torch.empty(n, 1, dtype=sx.dtype, device=DEV)
    ints = lambda: torch.empty(B, dtype=torch.int32, device=DEV)
    out = (real(), ints(), ints(), ints(), ints(), real(), real())
    work = torch.empty(B + 1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.bposd(g, sx, 12, out=out, work=work)
    for src, eager in ((xb, eb), (xa, ea)):
        sx.copy_(src)
        for t in out:
            t.fill_(7)
        cg.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)


def test_traces_as_registered_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    g = graph_of('toric_5')
    V, N = g.V, g.N

    def check(r, dt, device_type=None):
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
            r = torch.ops.gnnd.bposd(g.gid, x, 12, 0.75, 0.0, True, 'zero', 'cs', 10)
            check(r, dt)
            assert torch.ops.gnnd.bposd_out(g.gid, x, 12, 0.75, 0.0, True, 'zero', 'cs', 10,
                                            *r) is None
            o = torch.ops.gnnd.osd_gated(g.gid, x, r[5], r[4], 'zero', 'cs', 10, r[6])
            assert o[0].shape == (3 * V, 1) and o[0].dtype == dt
            assert o[1].shape == (3,) and o[2].shape == (3,) and o[2].dtype == torch.int32
            o = torch.ops.gnnd.osd_gated(g.gid, x, r[5], r[4], 'zero', 'cs', 10, None)
            assert torch.ops.gnnd.osd_gated_out(g.gid, x, r[5], r[4], 'zero', 'cs', 10, None,
                                                *o) is None
        xm = torch.empty(3 * N, 1, dtype=dt, device='meta')
        r = torch.ops.gnnd.bposd(g.gid, xm, 12, 0.75, 0.0, True, 'zero', 'cs', 10)
        check(r, dt, 'meta')
        o = torch.ops.gnnd.osd_gated(g.gid, xm, r[5], r[4], 'zero', 'cs', 10, r[6])
        assert o[0].shape == (3 * V, 1) and o[0].device.type == 'meta' and o[1].shape == (3,)
    alpha, beta, iters, early = bc.bp_params('toric_5')
    H, xs = mc.inputs('toric_5', 5, 'float64')
    xd = _dev(xs)
    eager = ops.bposd(g, xd, iters, alpha, beta, True, 'zero', 'cs', 10)
    r = torch.ops.gnnd.bposd(g.gid, xd, iters, alpha, beta, True, 'zero', 'cs', 10)
    assert all(torch.equal(a, b) for a, b in zip(r, eager))
    out = tuple(torch.empty_like(t) for t in r)
    torch.ops.gnnd.bposd_out(g.gid, xd, iters, alpha, beta, True, 'zero', 'cs', 10, *out)
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    o = torch.ops.gnnd.osd_gated(g.gid, xd, r[5], r[4], 'zero', 'cs', 10, r[6])
    assert all(torch.equal(a, b) for a, b in zip(o, eager[:3]))
    out = tuple(torch.empty_like(t) for t in o)
    torch.ops.gnnd.osd_gated_out(g.gid, xd, r[5], r[4], 'zero', 'cs', 10, r[6], *out)
    assert all(torch.equal(a, b) for a, b in zip(out, eager[:3]))


def test_debug_library_runs_bposd_clean():
    """toric-5 B = 67 and the rank-deficient graph under the bounds-checked build (GNND_LIB, a
    fresh child process): no index check fires and the bits are the host mirror's."""
    res = debug_child.run('decoder_debug_worker.py', 'bposd')
    assert res['equal'] == {'toric_5_bposd': True, 'toric_5_gated': True, 'bch_dup_gated': True}
