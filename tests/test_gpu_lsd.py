"""Localized-statistics decoding on the device (ops.lsd -> gnnd_lsd, ops.lsd_gated, ops.bplsd)
against the independent statement (tests/lsd_cases.py) and the host mirrors, exact equality of
every output: the shapes and batches of lsd_cases.SHAPES, both dtypes, both bases, bits_per_step
0, 1 and 3; the gate over sentinel-filled outputs; NULL outputs through the raw ABI; NaN and inf
in pred; bplsd on toric-5 against its mirror and against bposd on the pass-through rows; stream
capture; the registered ops; the LDS boundary on rings; the bounds-checked debug library."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import gnndecode as gd
from gnndecode import _lib, ops

import bposd_cases as bc
import debug_child
import lsd_cases as lc
import osd_cases as oc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

_GRAPHS = {}


def graph_of(code):
    if code not in _GRAPHS:
        _GRAPHS[code] = gd.TannerGraph(oc.code_matrix(code), device=DEV)
    return _GRAPHS[code]


def _np(t):
    return t.cpu().numpy().reshape(-1)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _sentinels(B, V, dtype, n_int=4, n_real=1):
    return (tuple(torch.full((B * V, 1), 7, dtype=dtype, device=DEV) for _ in range(n_real))
            + tuple(torch.full((B,), 7, dtype=torch.int32, device=DEV) for _ in range(n_int)))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B', lc.SHAPES)
def test_lsd_equals_statement_and_host_mirror(code, B, dtype):
    H, x, p = oc.inputs(code, B, dtype)
    g = graph_of(code)
    xd, pd = _dev(x).unsqueeze(1), _dev(p).unsqueeze(1)
    for base in ('zero', 'hard'):
        for bits in lc.BITS:
            out = ops.lsd(g, xd, pd, base, bits)
            assert len(out) == 5 and out[0].shape == pd.shape and out[0].dtype == pd.dtype
            for t in out[1:]:
                assert t.shape == (B,) and t.dtype == torch.int32
            got = tuple(_np(t) for t in out)
            what = (code, B, dtype, base, bits)
            lc.assert_equal(got, lc.as_tuple(lc.reference(code, B, dtype, base, bits), dtype), what)
            lc.assert_equal(got, ops.lsd_host(H, x, p, base, bits), what)
            assert torch.equal(out[1], ops.osd0(g, xd, pd, base)[1])


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_gate_over_sentinel_filled_outputs_and_null_outputs(dtype):
    code, B = 'toric_5', 67
    H, x, p = oc.inputs(code, B, dtype)
    g = graph_of(code)
    V = g.V
    llr = bc.llr_input(code, B, dtype)
    xd, pd, ld = (_dev(a).unsqueeze(1) for a in (x, p, llr))
    full = ops.lsd(g, xd, pd, 'zero', 1)
    for name in bc.GATES:
        gate_h = bc.gate(code, B, dtype, name) * np.resize(np.array([1, 5, -2], np.int32), B)
        gate = _dev(gate_h)
        on = _dev(gate_h != 0)
        for l in (ld, None):
            out = _sentinels(B, V, xd.dtype)
            r = ops.lsd_gated(g, xd, pd, gate, 'zero', 1, llr=l, out=out)
            assert all(a is b for a, b in zip(r, out))
            torch.cuda.synchronize()
            hard = ((l.view(B, V) < 0) if l is not None else (pd.view(B, V) > 0.5)).to(xd.dtype)
            assert torch.equal(out[0].view(B, V)[on], full[0].view(B, V)[on])
            assert torch.equal(out[0].view(B, V)[~on], hard[~on])
            for a, f in zip(out[1:], full[1:]):
                assert torch.equal(a[on], f[on]) and not bool(a[~on].any())
            lc.assert_equal(tuple(_np(t) for t in out),
                            ops.lsd_gated_host(H, x, p, gate_h, 'zero', 1,
                                               llr=None if l is None else llr), name)
    # a caller's workspace; a short one is refused
    work = torch.empty(ops.osd_gated_workspace(B), dtype=torch.uint8, device=DEV)
    gate = _dev(bc.gate(code, B, dtype, 'alt'))
    a = ops.lsd_gated(g, xd, pd, gate, llr=ld, work=work)
    b = ops.lsd_gated(g, xd, pd, gate, llr=ld)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    with pytest.raises(ValueError):
        ops.lsd_gated(g, xd, pd, gate, work=work[:-4])
    # every optional output skipped, through ops and through the raw C ABI
    out = _sentinels(B, V, xd.dtype)
    r = ops.lsd(g, xd, pd, 'zero', 1, out=(out[0], None, None, None, None))
    assert r[0] is out[0] and all(t is None for t in r[1:]) and torch.equal(out[0], full[0])
    out = _sentinels(B, V, xd.dtype)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code_t = _lib.F32 if dtype == 'float32' else _lib.F64
    torch.cuda.synchronize()
    lib = _lib.get()
    assert lib.gnnd_lsd(g.handle, code_t, ptr(xd), ptr(pd), 0, 1, ptr(out[0]), None, ptr(out[2]),
                        None, ptr(out[4]), B, stream) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out[0], full[0]) and torch.equal(out[2], full[2])
    assert torch.equal(out[4], full[4])
    assert bool((out[1] == 7).all()) and bool((out[3] == 7).all())
    out = _sentinels(B, V, xd.dtype)
    assert lib.gnnd_lsd_gated(g.handle, code_t, ptr(xd), ptr(pd), None, ptr(gate), 0, 1,
                              ptr(out[0]), ptr(out[1]), None, None, None, ptr(work),
                              work.numel(), B, stream) == _lib.OK
    torch.cuda.synchronize()
    want = ops.lsd_gated(g, xd, pd, gate)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    assert all(bool((t == 7).all()) for t in out[2:])
    # refusals before any device call leave the outputs alone
    out = _sentinels(B, V, xd.dtype)
    torch.cuda.synchronize()
    for args in ((0, -1, ptr(out[0]), ptr(work), work.numel()), (3, 1, ptr(out[0]), ptr(work), work.numel()),
                 (0, 1, None, ptr(work), work.numel()), (0, 1, ptr(out[0]), None, work.numel()),
                 (0, 1, ptr(out[0]), ptr(work), work.numel() - 1)):
        base, bits, eh, wk, wb = args
        assert lib.gnnd_lsd_gated(g.handle, code_t, ptr(xd), ptr(pd), None, ptr(gate), base, bits, eh,
                                  ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(out[4]), wk, wb, B,
                                  stream) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_lsd(g.handle, _lib.BF16, ptr(xd), ptr(pd), 0, 1, ptr(out[0]), None, None, None,
                        None, B, stream) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_nan_and_inf_in_pred_give_the_mirrors_bits(dtype):
    code, B = 'toric_7', 9
    H, x, p = oc.inputs(code, B, dtype)
    V = H.shape[0]
    p = p.copy().reshape(B, V)
    p[:, 0] = np.nan
    p[1::2, 3] = np.inf
    p[::2, 5] = -np.inf
    p[2, :] = np.nan
    p = p.reshape(-1)
    g = graph_of(code)
    for base in ('zero', 'hard'):
        for bits in (0, 1):
            got = tuple(_np(t) for t in ops.lsd(g, _dev(x), _dev(p), base, bits))
            lc.assert_equal(got, ops.lsd_host(H, x, p, base, bits), (base, bits))
            lc.assert_equal(got, lc.as_tuple(lc.ref_batch(H, x, p, base == 'hard', bits), dtype))
            assert oc.satisfied(H, x, got[0]).all() and not got[1].any()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_bplsd_on_toric_5(dtype):
    H, x, args = lc.bp_inputs(dtype)
    B = lc.BP_B
    V, C = H.shape
    g = graph_of(lc.BP_SHAPE)
    xd = _dev(x)
    names = ('ehat', 'status', 'rounds', 'nclus', 'ncols', 'iters_used', 'bp_status', 'pred', 'llr')
    for base, bits in (('zero', 1), ('hard', 0)):
        out = ops.bplsd(g, xd, *args, base, bits)
        got = dict(zip(names, (_np(t) for t in out)))
        solved = got['bp_status'] == 0
        assert solved.any() and (~solved).any()
        if dtype == 'float64':
            host = dict(zip(names, ops.bplsd_host(H, x, *args, base, bits)))
            for k in names:
                assert got[k].dtype == host[k].dtype and np.array_equal(got[k], host[k]), k
        # the stages by hand, and the mirror of the second stage on the device's own pred
        ms = ops.minsum(g, xd, *args)
        assert torch.equal(ms[1], out[8]) and torch.equal(ms[3], out[6]) and torch.equal(ms[2], out[5])
        assert torch.equal(ms[0], out[7])
        hand = ops.lsd_gated(g, xd, ms[0], ms[3], base, bits, llr=ms[1])
        assert all(torch.equal(a, b) for a, b in zip(hand, out[:5]))
        lc.assert_equal(tuple(_np(t) for t in out[:5]),
                        ops.lsd_gated_host(H, x, got['pred'], got['bp_status'], base, bits,
                                           llr=got['llr']))
        assert oc.satisfied(H, x, got['ehat']).all() and not got['status'].any()
        # bposd on the rows min-sum solved: every shared output
        po = ops.bposd(g, xd, *args, base, 'osd0', 0)
        sd = _dev(solved)
        assert torch.equal(out[0].view(B, V)[sd], po[0].view(B, V)[sd])
        assert torch.equal(out[1], po[1])
        for i, j in ((5, 3), (6, 4), (7, 5), (8, 6)):
            assert torch.equal(out[i], po[j])
        assert not got['rounds'][solved].any() and not got['ncols'][solved].any()
        assert (got['rounds'][~solved] >= 1).all()
    sent = tuple(torch.full_like(t, 7) for t in out)
    r = ops.bplsd(g, xd, *args, out=(sent[0], None, None, None, None, None, sent[6], sent[7], sent[8]))
    assert r[1] is None and torch.equal(r[0], ops.bplsd(g, xd, *args)[0])
    empty = torch.empty(0, 1, dtype=xd.dtype, device=DEV)
    assert len(ops.bplsd(g, empty, 5)) == 9 and len(ops.lsd(g, empty, empty)) == 5
    for kw in (dict(bits_per_step=-1), dict(base='x'), dict(iters=0), dict(alpha=0.0)):
        with pytest.raises(ValueError):
            ops.bplsd(g, xd, **{'iters': 5, **kw})
    with pytest.raises(TypeError):
        ops.bplsd(g, xd.bfloat16(), 5)
    with pytest.raises(RuntimeError):
        ops.lsd(g, xd.cpu(), out[7].cpu())


def test_capture_of_bplsd_gives_the_eager_bits_on_a_replay():
    H, x, args = lc.bp_inputs('float64')
    g = graph_of(lc.BP_SHAPE)
    xd = _dev(x)
    work = torch.empty(ops.osd_gated_workspace(lc.BP_B), dtype=torch.uint8, device=DEV)
    eager = ops.bplsd(g, xd, *args, 'zero', 1)
    out = tuple(torch.full_like(t, 7) for t in eager)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.bplsd(g, xd, *args, 'zero', 1, out=out, work=work)
    for t in out:
        t.fill_(7)
    cg.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    # release the graph and its private pool before returning, as tests/test_gpu_uf.py does
    del cg
    gc.collect()
    torch.cuda.empty_cache()


def test_lsd_and_bplsd_trace_as_registered_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    g = graph_of('toric_5')
    for dt in (torch.float32, torch.float64):
        with FakeTensorMode():
            x = torch.empty(3 * g.N, 1, dtype=dt, device=DEV)
            p = torch.empty(3 * g.V, 1, dtype=dt, device=DEV)
            gate = torch.empty(3, dtype=torch.int32, device=DEV)
            for out in (torch.ops.gnnd.lsd(g.gid, x, p, 'zero', 1),
                        torch.ops.gnnd.lsd_gated(g.gid, x, p, gate, 'hard', 0, None)):
                assert len(out) == 5 and out[0].shape == (3 * g.V, 1) and out[0].dtype == dt
                for t in out[1:]:
                    assert t.shape == (3,) and t.dtype == torch.int32
            assert torch.ops.gnnd.lsd_out(g.gid, x, p, 'zero', 1, *out) is None
            assert torch.ops.gnnd.lsd_gated_out(g.gid, x, p, gate, 'zero', 1, p, *out) is None
            bp = torch.ops.gnnd.bplsd(g.gid, x, 5, 0.75, 0.0, True, 'zero', 1)
            assert len(bp) == 9
            for i, t in enumerate(bp):
                if i in (0, 7, 8):
                    assert t.shape == (3 * g.V, 1) and t.dtype == dt
                else:
                    assert t.shape == (3,) and t.dtype == torch.int32
            assert torch.ops.gnnd.bplsd_out(g.gid, x, 5, 0.75, 0.0, True, 'zero', 1, *bp) is None
    B = 9
    H, xs, ps = oc.inputs('toric_5', B, 'float64')
    ref = lc.as_tuple(lc.reference('toric_5', B, 'float64', 'zero', 1), 'float64')
    xd, pd = _dev(xs), _dev(ps)
    out = torch.ops.gnnd.lsd(g.gid, xd, pd, 'zero', 1)
    lc.assert_equal(tuple(_np(t) for t in out), ref)
    out2 = tuple(torch.empty_like(t) for t in out)
    torch.ops.gnnd.lsd_out(g.gid, xd, pd, 'zero', 1, *out2)
    assert all(torch.equal(a, b) for a, b in zip(out2, out))
    gate = torch.tensor([1, 0, 1, 1, 0, 0, 1, 1, 1], dtype=torch.int32, device=DEV)
    gated = torch.ops.gnnd.lsd_gated(g.gid, xd, pd, gate, 'zero', 1, None)
    on = gate != 0
    assert torch.equal(gated[0].view(B, g.V)[on], out[0].view(B, g.V)[on])
    assert not bool(gated[2][~on].any())
    out3 = tuple(torch.empty_like(t) for t in out)
    torch.ops.gnnd.lsd_gated_out(g.gid, xd, pd, gate, 'zero', 1, None, *out3)
    assert all(torch.equal(a, b) for a, b in zip(out3, gated))
    H, x, args = lc.bp_inputs('float64')
    sb = _dev(x)
    eager = ops.bplsd(g, sb, *args, 'zero', 1)
    for a, b in zip(torch.ops.gnnd.bplsd(g.gid, sb, *args, 'zero', 1), eager):
        assert torch.equal(a, b)
    bp2 = tuple(torch.empty_like(t) for t in eager)
    torch.ops.gnnd.bplsd_out(g.gid, sb, *args, 'zero', 1, *bp2)
    assert all(torch.equal(a, b) for a, b in zip(bp2, eager))


def _ring(n):
    """H [n, n]: check c joins variables c - 1 and c."""
    H = np.zeros((n, n), np.uint8)
    H[np.arange(n), np.arange(n)] = 1
    H[np.arange(n) - 1, np.arange(n)] = 1
    return H


def _tile_bytes(V, C, elem):
    """One wave's LSD tile: the OSD tile (rows of an odd word count, keys, order, pivots, estimate,
    each a 16-byte multiple) and three int32 per check."""
    a16 = lambda k: (k + 15) // 16 * 16
    stride = ((V + 31) // 32 + 1) | 1
    return a16(C * stride * 4) + a16(V * elem) + a16(2 * V) + a16(2 * C) + a16(V) + 3 * a16(4 * C)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_lds_boundary_on_rings(dtype):
    elem = 4 if dtype == 'float32' else 8
    n = max(k for k in range(500, 800) if _tile_bytes(k, k, elem) <= 65536)
    over = n + 1
    assert _tile_bytes(over, over, elem) > 65536 and 65536 // _tile_bytes(n, n, elem) == 1
    B = 5
    rng = np.random.default_rng([n, elem])

    def case(k):
        H = _ring(k)
        e = (rng.random((B, k)) < 0.02).astype(np.int64)
        e[0] = 0
        x = np.ones((B, 2 * k))
        x[:, k:] = 1 - 2 * ((e @ H.astype(np.int64)) % 2)
        p = rng.random((B, k)) * 0.2 + 0.6 * e
        return H, x.reshape(-1).astype(dtype), p.reshape(-1).astype(dtype)

    H, x, p = case(n)
    g = gd.TannerGraph(H, device=DEV)
    got = tuple(_np(t) for t in ops.lsd(g, _dev(x), _dev(p), 'zero', 1))
    lc.assert_equal(got, ops.lsd_host(H, x, p, 'zero', 1), (dtype, n))
    assert oc.satisfied(H, x, got[0]).all() and not got[1].any()
    assert got[2][0] == 0 and got[2].max() >= 1 and got[3].max() >= 2
    H2, x2, p2 = case(over)
    g2 = gd.TannerGraph(H2, device=DEV)
    xd2, pd2 = _dev(x2), _dev(p2)
    poison = _sentinels(B, over, xd2.dtype)
    bp_poison = _sentinels(B, over, xd2.dtype, 6, 3)
    gate = torch.ones(B, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    for call in (lambda: ops.lsd(g2, xd2, pd2, out=poison),
                 lambda: ops.lsd_gated(g2, xd2, pd2, gate, out=poison),
                 lambda: ops.bplsd(g2, xd2, 3, out=(bp_poison[0], *bp_poison[3:], *bp_poison[1:3]))):
        with pytest.raises(_lib.GnndError) as err:
            call()
        assert err.value.status == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in poison + bp_poison)
    # the mirror has no tile and still decodes it
    assert not ops.lsd_host(H2, x2, p2, 'zero', 1)[1].any()


def test_debug_library_runs_lsd_clean():
    """toric-5 (fp64), syn_c65 (fp32) and syn_tall (fp64, with unsolvable codewords) through ops.lsd
    with bits_per_step 0 and 1, and bplsd on toric-5, under the bounds-checked build (GNND_LIB, a
    fresh child process): no index check fires and the bits are the statement's."""
    res = debug_child.run('decoder_debug_worker.py', 'lsd')
    assert res['equal'] and all(res['equal'].values()), res['equal']
