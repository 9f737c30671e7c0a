"""Min-sum BP with guided decimation on the device (ops.bpgd -> gnnd_bpgd) against the numpy
statement of the definition (tests/bpgd_cases.py) and the host mirror, exact equality of ehat / llr
/ iters / status / ndec and, in fp64, of pred: the shapes where the one-wave-per-codeword plan and
the pick's butterfly can go wrong (V = 63 and 64: lanes with no variable or exactly one; V = 100
and 196: a lane's own run of two to four variables and ties inside it; a partial workgroup and the
grid-stride tail; irregular degrees; tiles at the 64 KiB limit with one and two waves per workgroup
and the refusal just over it), the rounds == 0 case against ops.minsum, NULL outputs through
the raw ABI, a non-finite codeword, stream capture, the registered ops, the bounds-checked debug
library, and the hand-over to ops.osd_gated."""
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

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

# toric-5 (V = 100: lanes 36 .. 63 own one variable, the others two) at B = 9 (three workgroups, the
# last with one wave) and B = 67 (the last partial workgroup); toric-7 (V = 196: three or four
# variables per lane, ties across a lane's own run); syn_wide and syn_hub (irregular degrees, V =
# 243 and 300); BCH (V = 63: lane 63 has no variable and takes part in the butterfly); syn_sq64
# (V = 64: one variable per lane, degree-0 variables)
SHAPES = (('toric_5', 9), ('toric_5', 67), ('toric_7', 9), ('syn_wide', 9), ('syn_hub', 9),
          ('bch_63_45', 33), ('syn_sq64', 9))

_GRAPHS = {}


def graph_of(code):
    if code not in _GRAPHS:
        _GRAPHS[code] = gd.TannerGraph(mc.code_matrix(code), device=DEV)
    return _GRAPHS[code]


def _np(t):
    return t.cpu().numpy().reshape(-1)


def _run(code, B, dtype, pset, **kw):
    H, x = bc.inputs(code, B, dtype)
    g = graph_of(code)
    iters0, iters_round, rounds, per_round, pick = bc.params(g.V)[pset]
    xd = torch.from_numpy(x.copy()).to(DEV)
    return ops.bpgd(g, xd, iters0, iters_round, rounds, per_round, pick, bc.CLAMP, bc.ALPHA,
                    bc.BETA, **kw)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('pset', [0, 1, 2, 3])
@pytest.mark.parametrize('code,B', SHAPES)
def test_bpgd_equals_reference_and_host_mirror(code, B, pset, dtype):
    H, x = bc.inputs(code, B, dtype)
    ref = bc.reference(code, B, dtype, pset)
    g = graph_of(code)
    iters0, iters_round, rounds, per_round, pick = bc.params(g.V)[pset]
    xd = torch.from_numpy(x.copy()).to(DEV).unsqueeze(1)
    out = ops.bpgd(g, xd, iters0, iters_round, rounds, per_round, pick, bc.CLAMP, bc.ALPHA, bc.BETA)
    for t in out[:3]:
        assert t.shape == (B * g.V, 1) and t.dtype == xd.dtype
    for t in out[3:]:
        assert t.shape == (B,) and t.dtype == torch.int32
    got = tuple(_np(t) for t in out)
    bc.assert_equal(got, ref, 'device against the numpy statement')
    ehat, llr, pred, its, status, ndec = got
    assert np.array_equal(ehat, (llr < 0).astype(ehat.dtype))
    assert np.array_equal(status == 0, bc.satisfied(H, x, llr))
    mirror = ops.bpgd_host(H, x, iters0, iters_round, rounds, per_round, pick, bc.CLAMP, bc.ALPHA,
                           bc.BETA)
    bc.assert_equal(got, mirror, 'device against the host mirror')
    if dtype == 'float64':
        assert np.array_equal(pred, mirror[2]), 'fp64 pred: the fixed exponential'
    else:
        assert np.allclose(pred, ref['pred'], **mc.pred_tolerance(dtype))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B', [('toric_5', 67), ('bch_63_45', 33)])
def test_no_rounds_is_minsum(code, B, dtype):
    H, x = mc.inputs(code, B, dtype)
    g = graph_of(code)
    xd = torch.from_numpy(x.copy()).to(DEV)
    ehat, llr, pred, its, status, ndec = ops.bpgd(g, xd, 12, 7, 0, 3, 'most', 2.0)
    m_pred, m_llr, m_its, m_st = ops.minsum(g, xd, 12)
    assert torch.equal(llr, m_llr) and torch.equal(torch.signbit(llr), torch.signbit(m_llr))
    assert torch.equal(its, m_its) and torch.equal(status, m_st)
    assert torch.equal(ehat, (m_llr < 0).to(xd.dtype)) and torch.equal(pred, m_pred)
    assert not bool(ndec.any())


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_out_forms_null_outputs_and_raw_abi(dtype):
    code, B, pset = 'toric_5', 67, 1
    g = graph_of(code)
    iters0, iters_round, rounds, per_round, pick = bc.params(g.V)[pset]
    H, x = bc.inputs(code, B, dtype)
    xd = torch.from_numpy(x.copy()).to(DEV)
    base = _run(code, B, dtype, pset)

    def fresh():
        return (tuple(torch.full_like(base[0], 7) for _ in range(3))
                + tuple(torch.full((B,), 7, dtype=torch.int32, device=DEV) for _ in range(3)))

    out = fresh()
    r = _run(code, B, dtype, pset, out=out)
    assert all(a is b for a, b in zip(r, out))
    for a, b in zip(out, base):
        assert torch.equal(a, b)
    # every optional output skipped: the same ehat, nothing else written
    out = fresh()
    r = _run(code, B, dtype, pset, out=(out[0],) + (None,) * 5)
    assert r[0] is out[0] and all(t is None for t in r[1:])
    assert torch.equal(out[0], base[0])
    # NULL outputs through the raw C ABI: llr, iters and ndec skipped and left untouched
    out = fresh()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    st = _lib.get().gnnd_bpgd(g.handle, _lib.F32 if dtype == 'float32' else _lib.F64, p(xd),
                              bc.ALPHA, bc.BETA, iters0, iters_round, rounds, per_round,
                              _lib.BPGD_PICK[pick], bc.CLAMP, p(out[0]), None, p(out[2]), None,
                              p(out[4]), None, B,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.OK
    torch.cuda.synchronize()
    for i in (0, 2, 4):
        assert torch.equal(out[i], base[i])
    assert all(bool((out[i] == 7).all()) for i in (1, 3, 5))


def test_unsupported_graph_bad_arguments_and_empty_batch():
    # a check of degree 1: refused with nothing launched
    Hd = np.zeros((3, 2), np.uint8)
    Hd[[0, 1, 2, 2], [0, 0, 0, 1]] = 1
    gdeg = gd.TannerGraph(Hd, device=DEV)
    x = torch.zeros(5, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.GnndError) as e:
        ops.bpgd(gdeg, x, 5, 2, 3)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    g = graph_of('toric_5')
    empty = torch.empty(0, 1, dtype=torch.float64, device=DEV)
    out = ops.bpgd(g, empty, 5, 2, 3)
    assert len(out) == 6 and all(t.numel() == 0 for t in out)
    xd = torch.zeros(g.N, 1, dtype=torch.float64, device=DEV)
    for kw in ({'iters0': 0}, {'iters_round': 0}, {'rounds': -1}, {'per_round': 0},
               {'iters0': 2.5}, {'pick': 'any'}, {'clamp': 0.0}, {'clamp': float('inf')},
               {'alpha': 0.0}, {'alpha': 1.5}, {'beta': -1.0}):
        args = dict(iters0=5, iters_round=2, rounds=3)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.bpgd(g, xd, **args)
    with pytest.raises(ValueError):
        ops.bpgd(g, xd[:-1], 5, 2, 3)
    with pytest.raises(TypeError):
        ops.bpgd(g, xd.bfloat16(), 5, 2, 3)
    with pytest.raises(RuntimeError):
        ops.bpgd(g, xd.cpu(), 5, 2, 3)


def _pairs_case(V, B, dtype):
    """The pairs graph (check c joins variables 2c and 2c + 1, E = V) with priors quantised to
    multiples of 0.25 (exact ties between lanes) and a syndrome of weight growing with the
    codeword: the batch holds codewords solved at once, some that need decimations and some that
    run every round, and a lane scans V / 64 variables per pick."""
    H = np.zeros((V, V // 2), np.uint8)
    H[np.arange(V), np.arange(V) // 2] = 1
    rng = np.random.default_rng([V, B])
    x = np.empty((B, V + V // 2))
    x[:, :V] = np.round(rng.normal(3.0, 1.0, (B, V)) * 4) / 4
    for b in range(B):
        x[b, V:] = 1 - 2 * (rng.random(V // 2) < (0.0, 0.001, 0.002, 0.005, 0.02)[b % 5])
    return H, x.reshape(-1).astype(dtype)


# the tile is E + 2 V values of T and V int32, each array a 16-byte multiple here: 28 V bytes in
# fp64, 16 V in fp32.  (V that runs, waves per workgroup it gets, V that is refused); 16 * 4096 is
# the 64 KiB limit exactly
LDS_CASES = (('float64', 1000, 2, None), ('float64', 2340, 1, 2344), ('float32', 4096, 1, 4100))


@pytest.mark.parametrize('pick', ['least', 'most'])
@pytest.mark.parametrize('dtype,V,waves,V_over', LDS_CASES)
def test_lds_boundary_of_the_tile(dtype, V, waves, V_over, pick):
    """Large tiles: two waves and one wave per workgroup (B = 5: a partial last workgroup under two
    waves), 16 to 64 variables per lane in the pick's scan, the mirror's bits; a tile just over
    64 KiB is refused with nothing launched and poisoned outputs left as they were."""
    elem = 8 if dtype == 'float64' else 4
    tile = lambda v: v * elem + 2 * v * elem + 4 * v
    assert tile(V) % 16 == 0 and 65536 // tile(V) == waves
    B = 5
    H, x = _pairs_case(V, B, dtype)
    g = gd.TannerGraph(H, device=DEV)
    xd = torch.from_numpy(x.copy()).to(DEV)
    args = (3, 2, 12, 5, pick)
    out = ops.bpgd(g, xd, *args)
    host = ops.bpgd_host(H, x, *args)
    got = tuple(_np(t) for t in out)
    bc.assert_equal(got, host, (dtype, V, pick))
    if dtype == 'float64':
        assert np.array_equal(got[2], host[2])
    assert np.array_equal(got[4] == 0, _satisfied_pairs(H, x, got[1]))
    assert set(got[4].tolist()) == {0, 1} and (got[5] == 60).any() and (got[5] == 0).any()
    if V_over is None:
        return
    assert tile(V) <= 65536 < tile(V_over) and tile(V_over) % 16 == 0
    H2, x2 = _pairs_case(V_over, B, dtype)
    g2 = gd.TannerGraph(H2, device=DEV)
    xd2 = torch.from_numpy(x2.copy()).to(DEV)
    poison = (tuple(torch.full((B * V_over, 1), 7, dtype=xd2.dtype, device=DEV) for _ in range(3))
              + tuple(torch.full((B,), 7, dtype=torch.int32, device=DEV) for _ in range(3)))
    torch.cuda.synchronize()
    with pytest.raises(_lib.GnndError) as e:
        ops.bpgd(g2, xd2, *args, out=poison)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in poison)
    # the mirror has no tile and still decodes it
    assert len(ops.bpgd_host(H2, x2, *args)) == 6


def _satisfied_pairs(H, x, llr):
    """bpgd_cases.satisfied without the dense matrix product: check c holds variables 2c, 2c + 1."""
    V, C = H.shape
    t = x.reshape(-1, V + C)[:, V:] < 0
    h = llr.reshape(-1, V) < 0
    return ((h[:, 0::2] ^ h[:, 1::2]) == t).all(axis=1)


@pytest.mark.parametrize('pick', ['least', 'most'])
def test_nonfinite_codeword_stays_in_its_codeword(pick):
    """A NaN and an infinity in codeword 4 of 9: the call completes and the other eight codewords'
    outputs are the bits of the clean batch (only the neighbours are compared)."""
    B = 9
    H, x = bc.inputs('toric_5', B, 'float64')
    g = graph_of('toric_5')
    xd = torch.from_numpy(x.copy()).to(DEV)
    clean = ops.bpgd(g, xd, 10, 5, 16, 2, pick)
    xb = xd.clone()
    xb[4 * g.N + 3] = float('nan')
    xb[4 * g.N + 17] = float('inf')
    dirty = ops.bpgd(g, xb, 10, 5, 16, 2, pick)
    torch.cuda.synchronize()
    keep = torch.tensor([b for b in range(B) if b != 4], device=DEV)
    V = g.V
    for c, d in zip(clean[:3], dirty[:3]):
        assert torch.equal(c.view(B, V)[keep], d.view(B, V)[keep])
    for c, d in zip(clean[3:], dirty[3:]):
        assert torch.equal(c[keep], d[keep])
    assert 1 <= int(dirty[3][4]) <= 10 + 16 * 5
    assert int(dirty[4][4]) in (0, 1) and 0 <= int(dirty[5][4]) <= 32


def test_capture_gives_the_eager_bits_on_two_replays():
    code, B, pset = 'toric_5', 67, 2
    eager = _run(code, B, 'float64', pset)
    out = (tuple(torch.empty_like(eager[0]) for _ in range(3))
           + tuple(torch.empty(B, dtype=torch.int32, device=DEV) for _ in range(3)))
    H, x = bc.inputs(code, B, 'float64')
    g = graph_of(code)
    iters0, iters_round, rounds, per_round, pick = bc.params(g.V)[pset]
    sx = torch.from_numpy(x.copy()).to(DEV)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.bpgd(g, sx, iters0, iters_round, rounds, per_round, pick, bc.CLAMP, bc.ALPHA, bc.BETA,
                 out=out)
    for _ in range(2):
        for t in out:
            t.fill_(7)
        cg.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
    # Release the graph and its private pool here rather than whenever the collector next runs.
    # Without this, tests/test_gpu_bposd.py::test_capture_follows_the_gate_at_replay, which runs
    # after this file, failed with hipErrorStreamCaptureInvalidated in the full suite (and passed
    # alone, or with any one of several tests of this file deselected).  That a late release landed
    # inside its capture is a supposition: the order dependence itself is not explained yet.
    del cg
    gc.collect()
    torch.cuda.empty_cache()


def test_bpgd_traces_as_registered_ops():
    """gnnd::bpgd and gnnd::bpgd_out have fake kernels: shapes and dtypes without a launch, under
    FakeTensorMode and on the meta device; the real ops give the reference's bits."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    g = graph_of('toric_5')
    args = (10, 5, 16, 1, 'least', 25.0, 0.75, 0.0)
    for dt in (torch.float32, torch.float64):
        with FakeTensorMode():
            x = torch.empty(3 * g.N, 1, dtype=dt, device=DEV)
            out = torch.ops.gnnd.bpgd(g.gid, x, *args)
            assert len(out) == 6
            for t in out[:3]:
                assert t.shape == (3 * g.V, 1) and t.dtype == dt
            for t in out[3:]:
                assert t.shape == (3,) and t.dtype == torch.int32
            assert torch.ops.gnnd.bpgd_out(g.gid, x, *args, *out) is None
        xm = torch.empty(3 * g.N, 1, dtype=dt, device='meta')
        out = torch.ops.gnnd.bpgd(g.gid, xm, *args)
        assert out[0].shape == (3 * g.V, 1) and out[0].dtype == dt and out[0].device.type == 'meta'
        assert out[5].shape == (3,) and out[5].dtype == torch.int32
    H, xs = bc.inputs('toric_5', 9, 'float64')
    ref = bc.reference('toric_5', 9, 'float64', 1)
    xd = torch.from_numpy(xs.copy()).to(DEV)
    out = torch.ops.gnnd.bpgd(g.gid, xd, *bc.params(g.V)[1], bc.CLAMP, bc.ALPHA, bc.BETA)
    bc.assert_equal(tuple(_np(t) for t in out), ref)
    out2 = tuple(torch.empty_like(t) for t in out)
    torch.ops.gnnd.bpgd_out(g.gid, xd, *bc.params(g.V)[1], bc.CLAMP, bc.ALPHA, bc.BETA, *out2)
    for a, b in zip(out2, out):
        assert torch.equal(a, b)


def test_debug_library_runs_bpgd_clean():
    """toric-5 B = 67 (fp64, both picks) and syn_hub B = 9 (fp32, every variable decimated) under
    the bounds-checked build (GNND_LIB, a fresh child process): no index check fires and the bits
    are the numpy reference's."""
    res = debug_child.run('decoder_debug_worker.py', 'bpgd')
    assert res['equal'] and all(res['equal'].values()), res['equal']


def test_status0_satisfies_the_syndrome_and_osd_gated_takes_the_outputs():
    """sample_toric (toric-5, p = 0.05, B = 256, seed 11) -> bpgd (10, 5, 16, 1, least): every
    status-0 codeword has zero residual syndrome and bpgd solves more codewords than
    ops.minsum(g, x, 10) on the same x; ops.osd_gated takes pred, status and llr as they are, passes
    the status-0 decisions through and leaves no residual syndrome where its own status is 0."""
    g = graph_of('toric_5')
    H = mc.code_matrix('toric_5')
    B = 256
    x, y = ops.sample_toric(g, B, [0.05], seed=11)
    ehat, llr, pred, its, status, ndec = ops.bpgd(g, x, 10, 5, 16, 1, 'least')
    m_status = ops.minsum(g, x, 10)[3]
    solved, m_solved = int(status.eq(0).sum()), int(m_status.eq(0).sum())
    print(f'bpgd status 0: {solved} of {B}; minsum status 0: {m_solved}; '
          f'mean decimations {float(ndec.double().mean()):.2f}')
    V, C = H.shape
    t = (_np(x).reshape(B, V + C)[:, V:] < 0).astype(np.int64)
    Hi = H.astype(np.int64)
    st = _np(status)
    residual = (((_np(ehat).reshape(B, V).astype(np.int64) @ Hi) % 2) != t).any(axis=1)
    assert np.array_equal(residual, st == 1)
    assert solved > m_solved
    o_ehat, o_status, o_choice = ops.osd_gated(g, x, pred, status, llr=llr)
    oe, os_ = _np(o_ehat).reshape(B, V), _np(o_status)
    assert np.array_equal(oe[st == 0], _np(ehat).reshape(B, V)[st == 0])
    assert (_np(o_choice)[st == 0] == -1).all() and not os_[st == 0].any()
    o_residual = (((oe.astype(np.int64) @ Hi) % 2) != t).any(axis=1)
    assert not o_residual[os_ == 0].any()
