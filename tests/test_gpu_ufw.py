"""Weighted union-find and belief-find on the device (ops.ufw -> gnnd_ufw, ops.belief_find ->
gnnd_belief_find) against the independent unit-step statement (tests/ufw_cases.py) and the host
mirrors, exact equality of every output: the graphs of tests/uf_cases.py, B = 1, 3 and 67, both
dtypes, with llr and with the priors; the scale = 0 and wmax = 1 anchors against ops.uf; the gate in
both pass-through modes over sentinel-filled outputs; NULL outputs through the raw ABI; non-finite
inputs; the LDS boundary on rings; belief_find on toric-5; stream capture; the registered ops; the
bounds-checked debug library."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import gnndecode as gd
from gnndecode import _lib, ops

import debug_child
import minsum_cases as mc
import uf_cases as uc
import ufw_cases as wc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

_GRAPHS = {}


def graph_of(shape):
    if shape not in _GRAPHS:
        _GRAPHS[shape] = gd.TannerGraph(uc.code_matrix(shape), device=DEV)
    return _GRAPHS[shape]


def _np(t):
    return t.cpu().numpy().reshape(-1)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _sentinels(B, V, dtype, n_int=4):
    return ((torch.full((B * V, 1), 7, dtype=dtype, device=DEV),)
            + tuple(torch.full((B,), 7, dtype=torch.int32, device=DEV) for _ in range(n_int)))


@pytest.mark.parametrize('with_llr', [True, False], ids=['llr', 'priors'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('B', [1, 3, 67])
@pytest.mark.parametrize('shape', wc.SHAPES)
def test_ufw_equals_statement_and_host_mirror(shape, B, dtype, with_llr):
    H, x, llr = wc.inputs(shape, B, dtype)
    ref = wc.reference(shape, B, dtype, with_llr)
    g = graph_of(shape)
    xd = _dev(x).unsqueeze(1)
    ld = _dev(llr).unsqueeze(1) if with_llr else None
    out = ops.ufw(g, xd, ld, wc.SCALE, wc.WMAX)
    assert len(out) == 5 and out[0].shape == (B * g.V, 1) and out[0].dtype == xd.dtype
    for t in out[1:]:
        assert t.shape == (B,) and t.dtype == torch.int32
    got = tuple(_np(t) for t in out)
    wc.assert_equal(got, ref, 'device against the statement')
    wc.assert_equal(got, ops.ufw_host(H, x, llr if with_llr else None, wc.SCALE, wc.WMAX),
                    'device against the host mirror')
    V, C = H.shape
    t = x.reshape(B, V + C)[:, V:] < 0
    assert np.array_equal(uc.syndrome(H, got[0].reshape(B, V)), t)


@pytest.mark.parametrize('kw', [dict(scale=0.0, wmax=32), dict(scale=3.0, wmax=1)],
                         ids=['scale0', 'wmax1'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', wc.SHAPES)
def test_anchor_all_weights_one_is_uf_on_the_device(shape, dtype, kw):
    B = wc.B_ALL
    H, x, llr = wc.inputs(shape, B, dtype)
    g = graph_of(shape)
    xd = _dev(x)
    plain = ops.uf(g, xd)
    for ld in (_dev(llr), None):
        out = ops.ufw(g, xd, ld, **kw)
        for a, b in zip(out[:4], plain):
            assert torch.equal(a, b)
        assert bool((out[4] <= out[1]).all()) and bool(((out[4] == 0) == (out[1] == 0)).all())


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_gate_over_sentinel_filled_outputs_in_both_modes(dtype):
    shape, B = 'toric_5', 67
    H, x, llr = wc.inputs(shape, B, dtype)
    g = graph_of(shape)
    V = g.V
    llr = llr.copy()
    llr[V:V + 8] = [np.nan, -0.0, 0.0, -np.inf, np.inf, -1.0, 1.0, -1e-30]      # codeword 1: gated off
    xd, ld = _dev(x), _dev(llr)
    full = ops.ufw(g, xd, ld, wc.SCALE, wc.WMAX)
    gate_h = ((np.arange(B) % 3 != 1) * np.resize(np.array([1, 5, -2]), B)).astype(np.int32)
    gate = _dev(gate_h)
    on = _dev(gate_h != 0)
    assert bool(on.any()) and bool((~on).any()) and not gate_h[1]
    hard = (ld.view(B, V) < 0).to(xd.dtype)
    for passthrough in (False, True):
        out = _sentinels(B, V, xd.dtype)
        r = ops.ufw(g, xd, ld, wc.SCALE, wc.WMAX, gate=gate, passthrough=passthrough, out=out)
        assert all(a is b for a, b in zip(r, out))
        torch.cuda.synchronize()
        assert torch.equal(out[0].view(B, V)[on], full[0].view(B, V)[on])
        for a, f in zip(out[1:], full[1:]):
            assert torch.equal(a[on], f[on])
        if passthrough:
            assert torch.equal(out[0].view(B, V)[~on], hard[~on])
            assert out[0].view(B, V)[1, :8].tolist() == [0, 0, 0, 1, 0, 1, 0, 1]
            assert all(not bool(a[~on].any()) for a in out[1:])
        else:
            assert bool((out[0].view(B, V)[~on] == 7).all())
            assert all(bool((a[~on] == 7).all()) for a in out[1:])
    # every optional output skipped: the same ehat, nothing else written
    out = _sentinels(B, V, xd.dtype)
    r = ops.ufw(g, xd, ld, wc.SCALE, wc.WMAX, out=(out[0], None, None, None, None))
    assert r[0] is out[0] and all(t is None for t in r[1:])
    assert torch.equal(out[0], full[0])
    # NULL outputs through the raw C ABI: rounds and nfull skipped and left untouched
    out = _sentinels(B, V, xd.dtype)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    st = _lib.get().gnnd_ufw(g.handle, _lib.F32 if dtype == 'float32' else _lib.F64, p(xd), p(ld),
                             wc.SCALE, wc.WMAX, None, 0, p(out[0]), None, p(out[2]), None,
                             p(out[4]), B,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out[0], full[0]) and torch.equal(out[2], full[2])
    assert torch.equal(out[4], full[4])
    assert bool((out[1] == 7).all()) and bool((out[3] == 7).all())


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_non_finite_and_signed_zero_inputs_give_the_mirrors_bits(dtype):
    """NaN, +-0 and +-inf in llr, in the priors and in the syndrome rows are merely non-finite
    inputs: they change weights and syndrome bits, nothing else."""
    shape, B = 'toric_5', 9
    H, x, llr = wc.inputs(shape, B, dtype)
    xb, lb = wc.dirty_inputs(H, x, llr, B)
    V, C = H.shape
    with np.errstate(invalid='ignore'):
        t = xb[:, V:] < 0
    g = graph_of(shape)
    for l in (lb.reshape(-1), None):
        got = tuple(_np(o) for o in ops.ufw(g, _dev(xb.reshape(-1)), None if l is None else _dev(l),
                                            wc.SCALE, wc.WMAX))
        wc.assert_equal(got, ops.ufw_host(H, xb.reshape(-1), l, wc.SCALE, wc.WMAX))
        assert np.array_equal(uc.syndrome(H, got[0].reshape(B, V)), t) and not got[2].any()


@pytest.mark.parametrize('shape', ['ring_63', 'two_comp'])
def test_an_unsatisfiable_syndrome_stops_with_status_1(shape):
    H = uc.code_matrix(shape)
    V, C = H.shape
    x = np.ones((3, V + C))
    x[0, V + 2] = -1
    x[1, V + 1] = x[1, V + 3] = -1
    x[2, V + 0] = x[2, V + 1] = x[2, V + 4] = -1
    x = x.reshape(-1)
    llr = np.random.default_rng(3).normal(1.5, 2.5, 3 * V)
    got = tuple(_np(t) for t in ops.ufw(graph_of(shape), _dev(x), _dev(llr), wc.SCALE, wc.WMAX))
    wc.assert_equal(got, ops.ufw_host(H, x, llr, wc.SCALE, wc.WMAX))
    wc.assert_equal(got, wc.as_tuple(wc.ufw_ref(H, x, llr), 'float64'))
    assert got[2].tolist() == [1, 0, 1]


def _ring_case(n, B, dtype):
    """ring(n) with B sparse syndromes of short defect pairs (distances 1 .. 6) and llr from
    N(1.5, 2.5): a few dozen half-steps at wmax = 8."""
    H = uc.ring(n)
    rng = np.random.default_rng([n, B])
    x = np.ones((B, 2 * n))
    for b in range(B):
        for start in rng.choice(n // 16, size=(0, 1, 5, 40, 150)[b % 5], replace=False) * 16:
            x[b, n + start] = -1
            x[b, n + start + 1 + (start // 16) % 6] *= -1
    llr = rng.normal(1.5, 2.5, (B, n))
    return H, x.reshape(-1).astype(dtype), llr.reshape(-1).astype(dtype)


# the tile is gnnd_uf's: (V + 4 N) int32, each array a 16-byte multiple: 20 n bytes on ring(n) for
# n a multiple of 4.  3276 * 20 = 65 520 fits one wave per workgroup; 3277 rounds each array up to
# 13 120 bytes, 65 600 in all
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_lds_boundary_on_rings(dtype):
    n, n_over, B = 3276, 3277, 5
    tile = lambda k: 5 * ((4 * k + 15) // 16 * 16)
    assert tile(n) <= 65536 < tile(n_over) and 65536 // tile(n) == 1
    H, x, llr = _ring_case(n, B, dtype)
    g = gd.TannerGraph(H, device=DEV)
    got = tuple(_np(t) for t in ops.ufw(g, _dev(x), _dev(llr), wc.SCALE, wc.WMAX))
    wc.assert_equal(got, ops.ufw_host(H, x, llr, wc.SCALE, wc.WMAX), (dtype, n))
    t = x.reshape(B, 2 * n)[:, n:] < 0
    e = got[0].reshape(B, n) != 0
    assert np.array_equal(e ^ np.roll(e, 1, axis=1), t)      # check c joins variables c - 1 and c
    assert got[1].max() >= 3 and got[1].min() == 0 and not got[2].any()
    H2, x2, llr2 = _ring_case(n_over, B, dtype)
    g2 = gd.TannerGraph(H2, device=DEV)
    xd2, ld2 = _dev(x2), _dev(llr2)
    poison = _sentinels(B, n_over, xd2.dtype)
    bf_poison = _sentinels(B, n_over, xd2.dtype, 6) + tuple(
        torch.full((B * n_over, 1), 7, dtype=xd2.dtype, device=DEV) for _ in range(2))
    torch.cuda.synchronize()
    with pytest.raises(_lib.GnndError) as err:
        ops.ufw(g2, xd2, ld2, wc.SCALE, wc.WMAX, out=poison)
    assert err.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.GnndError) as err:           # the union of both stages' tile limits
        ops.belief_find(g2, xd2, 3, out=(bf_poison[0], *bf_poison[1:4], *bf_poison[7:],
                                         *bf_poison[4:7]))
    assert err.value.status == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((p == 7).all()) for p in poison + bf_poison)
    # the mirror has no tile and still decodes it
    assert not ops.ufw_host(H2, x2, llr2, wc.SCALE, wc.WMAX)[2].any()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_belief_find_on_toric_5(dtype):
    H, x = wc.bf_inputs(dtype)
    B = wc.B_ALL
    V, C = H.shape
    g = graph_of(wc.BF_SHAPE)
    xd = _dev(x)
    args = (wc.BF_ITERS, wc.BF_ALPHA, wc.BF_BETA, True, wc.SCALE, wc.WMAX)
    out = ops.belief_find(g, xd, *args)
    names = ('ehat', 'status', 'iters_used', 'bp_status', 'pred', 'llr', 'rounds', 'nfull', 'events')
    host = dict(zip(names, ops.belief_find_host(H, x, *args)))
    got = dict(zip(names, (_np(t) for t in out)))
    for k in names:
        if k == 'pred' and dtype == 'float32':
            np.testing.assert_allclose(got[k], host[k], rtol=1e-5)
            continue
        assert got[k].dtype == host[k].dtype and np.array_equal(got[k], host[k]), k
    t = x.reshape(B, V + C)[:, V:] < 0
    assert np.array_equal(uc.syndrome(H, got['ehat'].reshape(B, V)), t)
    assert not got['status'].any()
    solved = got['bp_status'] == 0
    assert solved.any() and (~solved).any()
    assert np.array_equal(got['ehat'].reshape(B, V)[solved], (got['llr'].reshape(B, V) < 0)[solved])
    assert not got['rounds'][solved].any() and not got['events'][solved].any()
    assert (got['rounds'][~solved] >= 1).all()
    # the stages by hand
    ms = ops.minsum(g, xd, wc.BF_ITERS, wc.BF_ALPHA, wc.BF_BETA, True)
    assert torch.equal(ms[1], out[5]) and torch.equal(ms[3], out[3]) and torch.equal(ms[2], out[2])
    hand = ops.ufw(g, xd, ms[1], wc.SCALE, wc.WMAX, gate=ms[3], passthrough=True)
    for a, k in zip(hand, ('ehat', 'rounds', 'status', 'nfull', 'events')):
        assert np.array_equal(_np(a), got[k]), k
    # optional outputs skipped
    sent = tuple(torch.full_like(t, 7) for t in out)
    r = ops.belief_find(g, xd, *args, out=(sent[0], None, None, sent[3], sent[4], sent[5], None,
                                           None, None))
    assert torch.equal(r[0], out[0]) and torch.equal(r[3], out[3]) and r[1] is None


def test_belief_find_refusals_leave_outputs_untouched():
    g = graph_of(wc.BF_SHAPE)
    H, x = wc.bf_inputs('float64')
    B = 3
    xd = _dev(x[:B * g.N])

    def sent():
        real = lambda: torch.full((B * g.V, 1), 7, dtype=xd.dtype, device=DEV)
        ints = lambda: torch.full((B,), 7, dtype=torch.int32, device=DEV)
        return (real(), ints(), ints(), ints(), real(), real(), ints(), ints(), ints())

    out = sent()
    torch.cuda.synchronize()
    for kw in (dict(wmax=0), dict(wmax=1025), dict(scale=-1.0), dict(scale=float('nan')),
               dict(iters=0), dict(alpha=0.0), dict(beta=-1.0)):
        with pytest.raises(ValueError):
            ops.belief_find(g, xd, **{'iters': 5, **kw}, out=out)
    with pytest.raises(ValueError):
        ops.belief_find(g, xd[:-1], 5, out=out)
    with pytest.raises(TypeError):
        ops.belief_find(g, xd.bfloat16(), 5, out=out)
    with pytest.raises(ValueError):
        ops.belief_find(g, xd, 5, out=out[:4] + (None,) + out[5:])
    # the raw ABI: a bad stage-two argument is refused before stage one launches
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = _lib.get()
    for scale, wmax, pred in ((2.0, 0, out[4]), (float('inf'), 8, out[4]), (2.0, 8, None)):
        st = lib.gnnd_belief_find(g.handle, _lib.F64, p(xd), 0.75, 0.0, 5, 1, scale, wmax,
                                  None if pred is None else p(pred), p(out[5]), p(out[2]), p(out[3]),
                                  p(out[0]), p(out[1]), p(out[6]), p(out[7]), p(out[8]), B, stream)
        assert st == _lib.ERR_INVALID_ARG
    # an unmatchable graph: min-sum alone would run
    Hb = mc.code_matrix('bch_63_45')
    gb = gd.TannerGraph(Hb, device=DEV)
    xb = torch.ones(B * gb.N, dtype=torch.float64, device=DEV)
    real = lambda: torch.full((B * gb.V, 1), 7, dtype=xb.dtype, device=DEV)
    outb = (real(),) + out[1:4] + (real(), real()) + out[6:]
    with pytest.raises(_lib.GnndError) as e:
        ops.belief_find(gb, xb, 5, out=outb)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.GnndError) as e:
        ops.ufw(gb, xb, out=(outb[0], None, None, None, None))
    assert e.value.status == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out + outb)


def test_bad_arguments_and_empty_batch():
    g = graph_of('toric_5')
    empty = torch.empty(0, 1, dtype=torch.float64, device=DEV)
    out = ops.ufw(g, empty)
    assert len(out) == 5 and all(t.numel() == 0 for t in out)
    assert len(ops.belief_find(g, empty, 5)) == 9
    xd = torch.zeros(2 * g.N, 1, dtype=torch.float64, device=DEV)
    ld = torch.zeros(2 * g.V, 1, dtype=torch.float64, device=DEV)
    gate = torch.ones(2, dtype=torch.int32, device=DEV)
    for kw in (dict(wmax=0), dict(wmax=1025), dict(scale=-1.0), dict(scale=float('nan')),
               dict(passthrough=True), dict(passthrough=True, gate=gate),
               dict(passthrough=True, llr=ld), dict(llr=ld[:-1]), dict(gate=gate[:1])):
        with pytest.raises(ValueError):
            ops.ufw(g, xd, **kw)
    with pytest.raises(ValueError):
        ops.ufw(g, xd[:-1])
    with pytest.raises(TypeError):
        ops.ufw(g, xd.bfloat16())
    with pytest.raises(TypeError):
        ops.ufw(g, xd, llr=ld.float())
    with pytest.raises(RuntimeError):
        ops.ufw(g, xd.cpu())
    with pytest.raises(TypeError):
        ops.ufw(g, xd, gate=gate.long())


def test_capture_gives_the_eager_bits_on_two_replays():
    shape, B = 'toric_5', 67
    H, x, llr = wc.inputs(shape, B, 'float64')
    g = graph_of(shape)
    sx, sl = _dev(x), _dev(llr)
    Hb, xb = wc.bf_inputs('float64')
    sb = _dev(xb)
    args = (wc.BF_ITERS, wc.BF_ALPHA, wc.BF_BETA, True, wc.SCALE, wc.WMAX)
    eager = ops.ufw(g, sx, sl, wc.SCALE, wc.WMAX) + ops.belief_find(g, sb, *args)
    out = tuple(torch.full_like(t, 7) for t in eager)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.ufw(g, sx, sl, wc.SCALE, wc.WMAX, out=out[:5])
        ops.belief_find(g, sb, *args, out=out[5:])
    for _ in range(2):
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


def test_ufw_and_belief_find_trace_as_registered_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    g = graph_of('toric_5')
    for dt in (torch.float32, torch.float64):
        with FakeTensorMode():
            x = torch.empty(3 * g.N, 1, dtype=dt, device=DEV)
            llr = torch.empty(3 * g.V, 1, dtype=dt, device=DEV)
            out = torch.ops.gnnd.ufw(g.gid, x, llr, 2.0, 8, None, False)
            assert len(out) == 5 and out[0].shape == (3 * g.V, 1) and out[0].dtype == dt
            for t in out[1:]:
                assert t.shape == (3,) and t.dtype == torch.int32
            assert torch.ops.gnnd.ufw_out(g.gid, x, llr, 2.0, 8, None, False, *out) is None
            bf = torch.ops.gnnd.belief_find(g.gid, x, 5, 0.75, 0.0, True, 2.0, 8)
            assert len(bf) == 9
            for i, t in enumerate(bf):
                if i in (0, 4, 5):
                    assert t.shape == (3 * g.V, 1) and t.dtype == dt
                else:
                    assert t.shape == (3,) and t.dtype == torch.int32
            assert torch.ops.gnnd.belief_find_out(g.gid, x, 5, 0.75, 0.0, True, 2.0, 8, *bf) is None
        xm = torch.empty(3 * g.N, 1, dtype=dt, device='meta')
        out = torch.ops.gnnd.ufw(g.gid, xm, None, 2.0, 8, None, False)
        assert out[0].shape == (3 * g.V, 1) and out[0].device.type == 'meta'
        assert out[4].shape == (3,) and out[4].dtype == torch.int32
    B = 9
    H, xs, ls = wc.inputs('toric_5', B, 'float64')
    ref = wc.reference('toric_5', B, 'float64', True)
    xd, ld = _dev(xs), _dev(ls)
    out = torch.ops.gnnd.ufw(g.gid, xd, ld, wc.SCALE, wc.WMAX, None, False)
    wc.assert_equal(tuple(_np(t) for t in out), ref)
    gate = torch.tensor([1, 0, 1, 1, 0, 0, 1, 1, 1], dtype=torch.int32, device=DEV)
    gated = torch.ops.gnnd.ufw(g.gid, xd, ld, wc.SCALE, wc.WMAX, gate, False)
    on = gate != 0
    assert torch.equal(gated[0].view(B, g.V)[on], out[0].view(B, g.V)[on])
    assert not bool(gated[0].view(B, g.V)[~on].any()) and not bool(gated[4][~on].any())
    out2 = tuple(torch.empty_like(t) for t in out)
    torch.ops.gnnd.ufw_out(g.gid, xd, ld, wc.SCALE, wc.WMAX, None, False, *out2)
    for a, b in zip(out2, out):
        assert torch.equal(a, b)
    Hb, xb = wc.bf_inputs('float64')
    sb = _dev(xb)
    args = (wc.BF_ITERS, wc.BF_ALPHA, wc.BF_BETA, True, wc.SCALE, wc.WMAX)
    eager = ops.belief_find(g, sb, *args)
    for a, b in zip(torch.ops.gnnd.belief_find(g.gid, sb, *args), eager):
        assert torch.equal(a, b)
    bf2 = tuple(torch.empty_like(t) for t in eager)
    torch.ops.gnnd.belief_find_out(g.gid, sb, *args, *bf2)
    for a, b in zip(bf2, eager):
        assert torch.equal(a, b)


def test_debug_library_runs_ufw_clean():
    """toric-5 (fp64, llr), ring-130 (fp32, priors), two_comp with unsatisfiable codewords and
    belief_find on toric-5 under the bounds-checked build (GNND_LIB, a fresh child process): no
    index check fires and the bits are the statement's."""
    res = debug_child.run('decoder_debug_worker.py', 'ufw')
    assert res['equal'] and all(res['equal'].values()), res['equal']
