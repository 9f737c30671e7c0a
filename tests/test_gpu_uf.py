"""The union-find decoder on the device (ops.uf -> gnnd_uf) against the independent statement of
the definition (tests/uf_cases.py) and the host mirror, exact equality of every output: toric-3 and
toric-5 (two virtual vertices), rings of 63, 64, 65 and 130 (lanes without work, exactly one wave,
more than one stride), a chain, parallel edges, two components of which one has a virtual vertex;
B = 1, 3 and 67 (a lone wave, a partial workgroup, the last partial workgroup); the gate over
sentinel-filled outputs; an unsatisfiable syndrome (status 1, no hang); NaN and signed zeros; the
LDS boundary on rings; stream capture; the registered ops; the bounds-checked debug library; and
the composition with bpgd."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import gnndecode as gd
from gnndecode import _lib, ops

import bpgd_cases as bc
import debug_child
import minsum_cases as mc
import uf_cases as uc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

_GRAPHS = {}


def graph_of(shape):
    if shape not in _GRAPHS:
        _GRAPHS[shape] = gd.TannerGraph(uc.code_matrix(shape), device=DEV)
    return _GRAPHS[shape]


def _np(t):
    return t.cpu().numpy().reshape(-1)


def _sentinels(B, V, dtype):
    return ((torch.full((B * V, 1), 7, dtype=dtype, device=DEV),)
            + tuple(torch.full((B,), 7, dtype=torch.int32, device=DEV) for _ in range(3)))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('B', [1, 3, 67])
@pytest.mark.parametrize('shape', uc.SHAPES)
def test_uf_equals_reference_and_host_mirror(shape, B, dtype):
    H, x = uc.inputs(shape, B, dtype)
    ref = uc.reference(shape, B, dtype)
    g = graph_of(shape)
    xd = torch.from_numpy(x.copy()).to(DEV).unsqueeze(1)
    out = ops.uf(g, xd)
    assert out[0].shape == (B * g.V, 1) and out[0].dtype == xd.dtype
    for t in out[1:]:
        assert t.shape == (B,) and t.dtype == torch.int32
    got = tuple(_np(t) for t in out)
    uc.assert_equal(got, ref, 'device against the statement')
    uc.assert_equal(got, ops.uf_host(H, x), 'device against the host mirror')
    V, C = H.shape
    t = x.reshape(B, V + C)[:, V:] < 0
    assert np.array_equal(uc.syndrome(H, got[0].reshape(B, V)), t)


@pytest.mark.parametrize('shape', uc.SHAPES)
def test_matching_is_the_hosts_decoding_graph(shape):
    g = graph_of(shape)
    N, ends = g.matching()
    hN, hends = ops.matching_host(uc.code_matrix(shape))
    assert N == hN and np.array_equal(ends, hends) and ends.dtype == np.int32
    if shape == 'toric_5':
        assert N == 50
        H = uc.code_matrix(shape)
        for v in range(g.V):
            checks = np.nonzero(H[v])[0].tolist()
            assert ends[v, :len(checks)].tolist() == checks


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_gated_run_over_sentinel_filled_outputs(dtype):
    shape, B = 'toric_5', 67
    H, x = uc.inputs(shape, B, dtype)
    g = graph_of(shape)
    V = g.V
    xd = torch.from_numpy(x.copy()).to(DEV)
    full = ops.uf(g, xd)
    gate_h = ((np.arange(B) % 3 != 1) * np.resize(np.array([1, 5, -2]), B)).astype(np.int32)
    gate = torch.from_numpy(gate_h).to(DEV)
    out = _sentinels(B, V, xd.dtype)
    r = ops.uf(g, xd, gate=gate, out=out)
    assert all(a is b for a, b in zip(r, out))
    torch.cuda.synchronize()
    on = torch.from_numpy(gate_h != 0).to(DEV)
    assert bool(on.any()) and bool((~on).any())
    assert torch.equal(out[0].view(B, V)[on], full[0].view(B, V)[on])
    assert bool((out[0].view(B, V)[~on] == 7).all())
    for a, f in zip(out[1:], full[1:]):
        assert torch.equal(a[on], f[on]) and bool((a[~on] == 7).all())
    # every optional output skipped: the same ehat, nothing else written
    out = _sentinels(B, V, xd.dtype)
    r = ops.uf(g, xd, out=(out[0], None, None, None))
    assert r[0] is out[0] and all(t is None for t in r[1:])
    assert torch.equal(out[0], full[0])
    # NULL outputs through the raw C ABI: rounds and nfull skipped and left untouched
    out = _sentinels(B, V, xd.dtype)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    st = _lib.get().gnnd_uf(g.handle, _lib.F32 if dtype == 'float32' else _lib.F64, p(xd), None,
                            p(out[0]), None, p(out[2]), None, B,
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out[0], full[0]) and torch.equal(out[2], full[2])
    assert bool((out[1] == 7).all()) and bool((out[3] == 7).all())


@pytest.mark.parametrize('code', ['bch_63_45', 'syn_hub'])
def test_unmatchable_graph_is_refused_with_outputs_untouched(code):
    H = mc.code_matrix(code)
    g = gd.TannerGraph(H, device=DEV)
    B = 3
    x = torch.zeros(B * g.N, dtype=torch.float64, device=DEV)
    out = _sentinels(B, g.V, x.dtype)
    torch.cuda.synchronize()
    with pytest.raises(_lib.GnndError) as e:
        ops.uf(g, x, out=out)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.GnndError) as e:
        g.matching()
    assert e.value.status == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)


def test_bad_arguments_and_empty_batch():
    g = graph_of('toric_5')
    empty = torch.empty(0, 1, dtype=torch.float64, device=DEV)
    out = ops.uf(g, empty)
    assert len(out) == 4 and all(t.numel() == 0 for t in out)
    xd = torch.zeros(2 * g.N, 1, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        ops.uf(g, xd[:-1])
    with pytest.raises(TypeError):
        ops.uf(g, xd.bfloat16())
    with pytest.raises(RuntimeError):
        ops.uf(g, xd.cpu())
    with pytest.raises(TypeError):
        ops.uf(g, xd, gate=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ops.uf(g, xd, gate=torch.zeros(3, dtype=torch.int32, device=DEV))
    # bf16 through the raw ABI: refused, nothing launched
    p = ctypes.c_void_p(xd.data_ptr())
    assert _lib.get().gnnd_uf(g.handle, _lib.BF16, p, None, p, None, None, None, 2,
                              None) == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize('shape', ['ring_63', 'two_comp'])
def test_an_unsatisfiable_syndrome_stops_with_status_1(shape):
    """Odd parity on a component without a virtual vertex: the kernel stops when a round changes
    nothing and reports status 1, the bits of the mirror and of the statement."""
    H = uc.code_matrix(shape)
    V, C = H.shape
    x = np.ones((3, V + C))
    x[0, V + 2] = -1
    x[1, V + 1] = x[1, V + 3] = -1
    x[2, V + 0] = x[2, V + 1] = x[2, V + 4] = -1
    x = x.reshape(-1)
    got = tuple(_np(t) for t in ops.uf(graph_of(shape), torch.from_numpy(x.copy()).to(DEV)))
    uc.assert_equal(got, ops.uf_host(H, x))
    r = uc.uf_ref(H, x)
    uc.assert_equal(got, (r['ehat01'].reshape(-1).astype('float64'), r['rounds'], r['status'],
                          r['nfull']))
    assert got[2].tolist() == [1, 0, 1]


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_nan_and_signed_zeros_in_the_syndrome_rows(dtype):
    shape, B = 'toric_5', 9
    H, x = uc.inputs(shape, B, dtype)
    V, C = H.shape
    xb = x.reshape(B, V + C).copy()
    t = xb[:, V:] < 0
    rng = np.random.default_rng(5)
    kind = rng.integers(0, 4, t.shape)
    for k, val in ((1, np.nan), (2, 0.0), (3, -0.0)):
        xb[:, V:][(kind == k) & ~t] = val
    xb[:, :V][::2] = np.nan
    xb[1, :V] = np.inf
    xb[:, V:][t & (kind == 1)] = np.nan                     # and some 1 bits cleared by a NaN
    with np.errstate(invalid='ignore'):
        t2 = xb[:, V:] < 0
    g = graph_of(shape)
    got = tuple(_np(o) for o in ops.uf(g, torch.from_numpy(xb.reshape(-1)).to(DEV)))
    uc.assert_equal(got, ops.uf_host(H, xb.reshape(-1)))
    assert np.array_equal(uc.syndrome(H, got[0].reshape(B, V)), t2) and not got[2].any()


def _ring_case(n, B, dtype):
    """ring(n) with B sparse syndromes of short defect pairs: distances 1 .. 6, so a few rounds."""
    H = uc.ring(n)
    rng = np.random.default_rng([n, B])
    x = np.ones((B, 2 * n))
    for b in range(B):
        for start in rng.choice(n // 16, size=(0, 1, 5, 40, 150)[b % 5], replace=False) * 16:
            x[b, n + start] = -1
            x[b, n + start + 1 + (start // 16) % 6] *= -1
    return H, x.reshape(-1).astype(dtype)


# the tile is (V + 4 N) int32, each array a 16-byte multiple: 20 n bytes on ring(n) for n a
# multiple of 4.  3276 * 20 = 65 520 fits one wave per workgroup; 3277 rounds each array up to
# 13 120 bytes, 65 600 in all
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_lds_boundary_on_rings(dtype):
    n, n_over, B = 3276, 3277, 5
    tile = lambda k: 5 * ((4 * k + 15) // 16 * 16)
    assert tile(n) <= 65536 < tile(n_over) and 65536 // tile(n) == 1
    H, x = _ring_case(n, B, dtype)
    g = gd.TannerGraph(H, device=DEV)
    out = ops.uf(g, torch.from_numpy(x.copy()).to(DEV))
    got = tuple(_np(t) for t in out)
    host = ops.uf_host(H, x)
    uc.assert_equal(got, host, (dtype, n))
    t = x.reshape(B, 2 * n)[:, n:] < 0
    e = got[0].reshape(B, n) != 0
    assert np.array_equal(e ^ np.roll(e, 1, axis=1), t)      # check c joins variables c - 1 and c
    assert got[1].max() >= 3 and got[1].min() == 0 and not got[2].any()
    H2, x2 = _ring_case(n_over, B, dtype)
    g2 = gd.TannerGraph(H2, device=DEV)
    xd2 = torch.from_numpy(x2.copy()).to(DEV)
    poison = _sentinels(B, n_over, xd2.dtype)
    torch.cuda.synchronize()
    with pytest.raises(_lib.GnndError) as err:
        ops.uf(g2, xd2, out=poison)
    assert err.value.status == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((p == 7).all()) for p in poison)
    # the mirror has no tile and still decodes it
    assert not ops.uf_host(H2, x2)[2].any()


def test_capture_gives_the_eager_bits_on_two_replays():
    shape, B = 'toric_5', 67
    H, x = uc.inputs(shape, B, 'float64')
    g = graph_of(shape)
    sx = torch.from_numpy(x.copy()).to(DEV)
    eager = ops.uf(g, sx)
    out = _sentinels(B, g.V, sx.dtype)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.uf(g, sx, out=out)
    for _ in range(2):
        for t in out:
            t.fill_(7)
        cg.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
    # release the graph and its private pool before returning, as tests/test_gpu_bpgd.py does
    del cg
    gc.collect()
    torch.cuda.empty_cache()


def test_uf_traces_as_registered_ops():
    """gnnd::uf and gnnd::uf_out have fake kernels: shapes and dtypes without a launch, under
    FakeTensorMode and on the meta device; the real ops give the reference's bits."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    g = graph_of('toric_5')
    for dt in (torch.float32, torch.float64):
        with FakeTensorMode():
            x = torch.empty(3 * g.N, 1, dtype=dt, device=DEV)
            out = torch.ops.gnnd.uf(g.gid, x, None)
            assert len(out) == 4 and out[0].shape == (3 * g.V, 1) and out[0].dtype == dt
            for t in out[1:]:
                assert t.shape == (3,) and t.dtype == torch.int32
            assert torch.ops.gnnd.uf_out(g.gid, x, None, *out) is None
        xm = torch.empty(3 * g.N, 1, dtype=dt, device='meta')
        out = torch.ops.gnnd.uf(g.gid, xm, None)
        assert out[0].shape == (3 * g.V, 1) and out[0].device.type == 'meta'
        assert out[3].shape == (3,) and out[3].dtype == torch.int32
    B = 9
    H, xs = uc.inputs('toric_5', B, 'float64')
    ref = uc.reference('toric_5', B, 'float64')
    xd = torch.from_numpy(xs.copy()).to(DEV)
    out = torch.ops.gnnd.uf(g.gid, xd, None)
    uc.assert_equal(tuple(_np(t) for t in out), ref)
    gate = torch.tensor([1, 0, 1, 1, 0, 0, 1, 1, 1], dtype=torch.int32, device=DEV)
    gated = torch.ops.gnnd.uf(g.gid, xd, gate)
    on = gate != 0
    assert torch.equal(gated[0].view(B, g.V)[on], out[0].view(B, g.V)[on])
    assert not bool(gated[0].view(B, g.V)[~on].any()) and not bool(gated[1][~on].any())
    out2 = tuple(torch.empty_like(t) for t in out)
    torch.ops.gnnd.uf_out(g.gid, xd, None, *out2)
    for a, b in zip(out2, out):
        assert torch.equal(a, b)


def test_debug_library_runs_uf_clean():
    """toric-5 B = 67 (fp64), ring-130 (fp32) and two_comp with an unsatisfiable codeword under the
    bounds-checked build (GNND_LIB, a fresh child process): no index check fires and the bits are
    the statement's."""
    res = debug_child.run('decoder_debug_worker.py', 'uf')
    assert res['equal'] and all(res['equal'].values()), res['equal']


def test_uf_finishes_what_bpgd_left():
    """bpgd on toric-5 (B = 67), then uf gated by its status into the same ehat and status: every
    codeword then satisfies its syndrome, and the rows bpgd solved are unchanged."""
    shape, B = 'toric_5', 67
    H, x = bc.inputs(shape, B, 'float64')     # its recorded coverage: status 0 and status 1 both
    g = graph_of(shape)
    V, C = H.shape
    xd = torch.from_numpy(x.copy()).to(DEV)
    ehat, llr, pred, its, status, ndec = ops.bpgd(g, xd, *bc.params(V)[1], bc.CLAMP, bc.ALPHA,
                                                  bc.BETA)
    before, st = ehat.clone(), _np(status).copy()
    assert set(st.tolist()) == {0, 1}
    rounds = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ops.uf(g, xd, gate=status, out=(ehat, rounds, status, None))
    torch.cuda.synchronize()
    t = x.reshape(B, V + C)[:, V:] < 0
    assert np.array_equal(uc.syndrome(H, _np(ehat).reshape(B, V)), t)
    assert not bool(status.any())
    solved = torch.from_numpy(st == 0).to(DEV)
    assert torch.equal(ehat.view(B, V)[solved], before.view(B, V)[solved])
    assert bool((rounds[solved] == -1).all()) and bool((rounds[~solved] >= 1).all())
    # the rows it overwrote are the ungated decoder's
    alone = ops.uf(g, xd)[0]
    assert torch.equal(ehat.view(B, V)[~solved], alone.view(B, V)[~solved])
