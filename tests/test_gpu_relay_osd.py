"""Soft relay and relay+OSD on the device (ops.relay_soft -> gnnd_relay_soft, ops.relay_osd ->
gnnd_relay_osd) against ops.relay, the numpy statement (tests/relay_osd_cases.py) and the host
mirrors: the shapes where the one-wave-per-codeword plan can go wrong (V not a multiple of 64, two
checks per lane, C < 64, eleven variables per lane with one or three waves per workgroup, hub
variables, exact wave boundaries), both dtypes, both soft modes, every parameter set; the
composition from the public ops, the guarantees, the one-leg zero-gamma case against ops.bposd, the
LDS boundary of the MEAN tile, out= / work= forms, refusals, a non-finite codeword, stream capture
with the gate changing between replays, the registered ops and the bounds-checked debug library."""
import ctypes

import numpy as np
import pytest
import torch

import gnndecode as gd
from gnndecode import _lib, ops

import debug_child
import minsum_cases as mc
import relay_cases as rc
import relay_osd_cases as roc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

CASES = [(code, B, dt, p) for _, code, B in roc.SHAPES for dt in ('float32', 'float64')
         for p in rc.PARAMS]

_GRAPHS = {}


def graph_of(code):
    if code not in _GRAPHS:
        _GRAPHS[code] = gd.TannerGraph(mc.code_matrix(code), device=DEV)
    return _GRAPHS[code]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def _np(t):
    return t.cpu().numpy().reshape(-1)


def _case(code, B, dtype, params):
    legs, iters0, iters_leg, S = params
    H, x = roc.inputs(code, B, dtype, params)
    g = graph_of(code)
    return H, x, g, _dev(x).unsqueeze(1), (_dev(rc.gammas(g.V, params, dtype)), iters0, iters_leg,
                                           S, rc.ALPHA, rc.BETA)


def _host_args(args):
    return (_np(args[0]).reshape(args[0].shape),) + tuple(args[1:])


@pytest.mark.parametrize('code,B,dtype,params', CASES)
def test_relay_soft_equals_relay_reference_and_mirror(code, B, dtype, params):
    """The relay outputs are ops.relay's bits; soft is the numpy statement's and the mirror's in
    both dtypes; pred is the mirror's bits in fp64 and within the project's soft-output tolerance
    of it in fp32 (the device's expf), as the bposd tests hold min-sum's."""
    H, x, g, xd, args = _case(code, B, dtype, params)
    ref = roc.reference(code, B, dtype, params)
    plain = ops.relay(g, xd, *args)
    for mode in roc.MODES:
        out = ops.relay_soft(g, xd, *args, soft=mode)
        pred, soft = out[:2]
        for t in out[:4]:
            assert t.shape == (B * g.V, 1) and t.dtype == xd.dtype
        for t in out[4:]:
            assert t.shape == (B,) and t.dtype == torch.int32
        for a, b in zip(out[2:], plain):
            assert torch.equal(a, b)
        assert torch.equal(torch.signbit(out[3]), torch.signbit(plain[1]))
        rc.assert_equal(tuple(_np(t) for t in out[2:]), ref, (code, B, dtype, params, mode))
        host = ops.relay_soft_host(H, x, *_host_args(args), soft=mode)
        for want in (ref['soft_' + mode], host[1]):
            assert np.array_equal(_np(soft), want)
            assert np.array_equal(np.signbit(_np(soft)), np.signbit(want))
        print(code, B, dtype, params, mode, 'pred elements differing from the mirror:',
              int((_np(pred) != host[0]).sum()))
        if dtype == 'float64':
            assert np.array_equal(_np(pred), host[0])
        else:
            np.testing.assert_allclose(_np(pred), host[0], **mc.pred_tolerance(dtype))


@pytest.mark.parametrize('code,B,dtype,params', CASES)
def test_relay_osd_equals_its_parts_and_mirror(code, B, dtype, params):
    """relay_osd is relay_soft followed by osd_gated(gate=status, llr=llr), composed from the
    public ops, bit for bit; in fp64 every output is relay_osd_host's; in fp32 the relay outputs
    and the pass-through codewords are.  Every status-0 estimate satisfies the syndrome; solved
    codewords keep relay's estimate with choice -1."""
    H, x, g, xd, args = _case(code, B, dtype, params)
    V = g.V
    base = roc.base_of(code)
    for mode in roc.MODES:
        got = ops.relay_osd(g, xd, *args, soft=mode, base=base, method=roc.METHOD, order=roc.ORDER)
        ehat, status, choice, pred, llr, its, rst, leg, nsol = got
        assert ehat.shape == (B * V, 1) and ehat.dtype == xd.dtype
        s = ops.relay_soft(g, xd, *args, soft=mode)
        o = ops.osd_gated(g, xd, s[0], s[5], base, roc.METHOD, roc.ORDER, llr=s[3])
        for a, b in zip((pred, llr, its, rst, leg, nsol, ehat, status, choice),
                        (s[0],) + s[3:] + o):
            assert np.array_equal(_np(a), _np(b), equal_nan=True)
        host = ops.relay_osd_host(H, x, *_host_args(args), soft=mode, base=base,
                                  method=roc.METHOD, order=roc.ORDER)
        names = ('ehat', 'status', 'choice', 'pred', 'llr', 'iters', 'relay_status', 'leg', 'nsol')
        solved = _np(rst) == 0
        for name, a, b in zip(names, got, host):
            a = _np(a)
            if dtype == 'float64' or name in ('llr', 'iters', 'relay_status', 'leg', 'nsol'):
                assert np.array_equal(a, b), (mode, name)
            elif name == 'pred':
                np.testing.assert_allclose(a, b, **mc.pred_tolerance(dtype))
            else:                                           # fp32: pass-through codewords
                rows = (lambda t: t.reshape(B, V)) if name == 'ehat' else (lambda t: t)
                assert np.array_equal(rows(a)[solved], rows(b)[solved]), (mode, name)
        e = _np(ehat)
        assert rc.satisfied(H, x, -e)[_np(status) == 0].all()
        assert (_np(choice)[solved] == -1).all() and (_np(status)[solved] == 0).all()
        assert np.array_equal(e.reshape(B, V)[solved], _np(s[2]).reshape(B, V)[solved])
        assert set(_np(rst).tolist()) == {0, 1}


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('code,B', [('toric_5', 67), ('bch_63_45', 33)])
def test_one_leg_zero_gamma_last_is_bposd(code, B, dtype):
    H, x = mc.inputs(code, B, dtype)
    g = graph_of(code)
    xd = _dev(x)
    base = roc.base_of(code)
    zero = torch.zeros(1, g.V, dtype=xd.dtype, device=DEV)
    ehat, status, choice, pred, llr, its, rst, leg, nsol = ops.relay_osd(g, xd, zero, 12,
                                                                        soft='last', base=base)
    b_ehat, b_status, b_choice, b_its, b_bp, b_pred, b_llr = ops.bposd(g, xd, 12, early_stop=True,
                                                                       base=base)
    for a, b in ((ehat, b_ehat), (status, b_status), (choice, b_choice), (pred, b_pred),
                 (llr, b_llr), (its, b_its), (rst, b_bp)):
        assert torch.equal(a, b)
    assert torch.equal(torch.signbit(llr), torch.signbit(b_llr))
    assert set(_np(rst).tolist()) == {0, 1}


def test_lds_boundary_of_the_mean_tile():
    """The pairs graph V = 1400, C = 700, E = 1400 (check c joins variables 2c and 2c + 1) in
    fp64: LAST needs (1400 + 5600) * 8 = 56 000 B and runs, one wave per workgroup and 22 variables
    per lane, with the mirror's bits; MEAN needs (1400 + 7000) * 8 = 67 200 B and is refused with
    nothing launched; relay_osd is refused in both modes (the OSD rows alone, 700 x 45 words, are
    over 64 KiB)."""
    V, C, B = 1400, 700, 2
    H = np.zeros((V, C), np.uint8)
    H[np.arange(V), np.arange(V) // 2] = 1
    g = gd.TannerGraph(H, device=DEV)
    rng = np.random.default_rng(3)
    x = np.empty((B, V + C))
    x[:, :V] = rng.normal(1.0, 1.5, (B, V))
    x[:, V:] = 1 - 2 * (rng.random((B, C)) < 0.3)
    x = x.reshape(-1)
    gm = rc.gammas(V, rc.PARAMS[3], 'float64')
    legs, iters0, iters_leg, S = rc.PARAMS[3]
    xd, gd_ = _dev(x), _dev(gm)
    out = ops.relay_soft(g, xd, gd_, iters0, iters_leg, S, soft='last')
    host = ops.relay_soft_host(H, x, gm, iters0, iters_leg, S, soft='last')
    for a, b in zip(out, host):
        assert np.array_equal(_np(a), b)
    poison = tuple(torch.full_like(t, 7) for t in out)
    torch.cuda.synchronize()
    with pytest.raises(_lib.GnndError) as e:
        ops.relay_soft(g, xd, gd_, iters0, iters_leg, S, soft='mean', out=poison)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in poison)
    for mode in roc.MODES:
        with pytest.raises(_lib.GnndError) as e:
            ops.relay_osd(g, xd, gd_, iters0, iters_leg, S, soft=mode)
        assert e.value.status == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_out_and_work_forms(dtype):
    code, B, params = 'toric_5', 9, rc.PARAMS[1]
    H, x, g, xd, args = _case(code, B, dtype, params)
    base_s = ops.relay_soft(g, xd, *args, soft='mean')
    base_o = ops.relay_osd(g, xd, *args, soft='mean')

    def fresh(like):
        return tuple(torch.full_like(t, 7) for t in like)

    out = fresh(base_s)
    r = ops.relay_soft(g, xd, *args, soft='mean', out=out)
    assert all(a is b for a, b in zip(r, out))
    for a, b in zip(out, base_s):
        assert torch.equal(a, b)
    out = fresh(base_s)
    r = ops.relay_soft(g, xd, *args, soft='mean', out=(out[0], None, out[2]) + (None,) * 5)
    assert r[0] is out[0] and r[2] is out[2] and all(t is None for t in r[3:]) and r[1] is None
    assert torch.equal(out[0], base_s[0]) and torch.equal(out[2], base_s[2])
    out = fresh(base_o)
    work = torch.empty(ops.osd_gated_workspace(B) + 8, dtype=torch.uint8, device=DEV)
    r = ops.relay_osd(g, xd, *args, soft='mean', out=out, work=work)
    assert all(a is b for a, b in zip(r, out))
    for a, b in zip(out, base_o):
        assert torch.equal(a, b)
    out = fresh(base_o)
    r = ops.relay_osd(g, xd, *args, soft='mean',
                      out=(out[0], out[1], None, out[3], out[4], None, out[6], None, None))
    for i in (0, 1, 3, 4, 6):
        assert torch.equal(out[i], base_o[i])
    assert all(r[i] is None for i in (2, 5, 7, 8))
    for bad in ((out[0], out[1], out[2], None) + out[4:], (out[0], None) + out[2:], out[:8],
                out[:6] + (None,) + out[7:]):
        with pytest.raises(ValueError):
            ops.relay_osd(g, xd, *args, out=bad)
    with pytest.raises(ValueError):
        ops.relay_osd(g, xd, *args, work=torch.empty(4, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.relay_soft(g, xd, *args, out=(None,) + base_s[1:])
    # the raw C ABI: a NULL d_pred and a soft mode outside the enum are refused before any launch
    lib = _lib.get()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out = fresh(base_s)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code_dt = _lib.F32 if dtype == 'float32' else _lib.F64
    call = lambda soft, pred: lib.gnnd_relay_soft(
        g.handle, code_dt, p(xd), p(args[0]), 6, 12, 12, 1, 0.75, 0.0, soft, pred,
        *(p(t) for t in out[1:]), B, stream)
    assert call(2, p(out[0])) == _lib.ERR_INVALID_ARG
    assert call(1, None) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)
    assert call(1, p(out[0])) == _lib.OK
    torch.cuda.synchronize()
    for a, b in zip(out, base_s):
        assert torch.equal(a, b)


def test_bad_arguments_and_empty_batch():
    g = graph_of('toric_5')
    gm = ops.relay_gammas(g.V, 3, device=DEV)
    empty = torch.empty(0, 1, dtype=torch.float64, device=DEV)
    out = ops.relay_soft(g, empty, gm, 5)
    assert len(out) == 8 and all(t.numel() == 0 for t in out)
    out = ops.relay_osd(g, empty, gm, 5)
    assert len(out) == 9 and all(t.numel() == 0 for t in out)
    xd = torch.zeros(g.N, 1, dtype=torch.float64, device=DEV)
    for fn in (ops.relay_soft, ops.relay_osd):
        for kw in ({'iters0': 0}, {'iters_leg': 0}, {'stop_after': 0}, {'iters0': 2.5},
                   {'alpha': 0.0}, {'alpha': 1.5}, {'beta': -1.0}, {'soft': 'median'},
                   {'soft': 1}):
            kwargs = dict(iters0=5)
            kwargs.update(kw)
            with pytest.raises(ValueError):
                fn(g, xd, gm, **kwargs)
        with pytest.raises(ValueError):
            fn(g, xd[:-1], gm, 5)
        with pytest.raises(ValueError):
            fn(g, xd, gm[:, :-1], 5)
        with pytest.raises(ValueError):
            fn(g, xd, gm[:0], 5)
        with pytest.raises(TypeError):
            fn(g, xd, gm.float(), 5)
        with pytest.raises(TypeError):
            fn(g, xd.bfloat16(), gm.bfloat16(), 5)
        with pytest.raises(RuntimeError):
            fn(g, xd.cpu(), gm, 5)
    for kw in ({'base': 'soft'}, {'method': 'osd9'}, {'order': -1}, {'order': 65}):
        with pytest.raises(ValueError):
            ops.relay_osd(g, xd, gm, 5, **kw)
    # a check of degree 1: refused with nothing launched
    Hd = np.zeros((3, 2), np.uint8)
    Hd[[0, 1, 2, 2], [0, 0, 0, 1]] = 1
    gdeg = gd.TannerGraph(Hd, device=DEV)
    x = torch.zeros(5, dtype=torch.float64, device=DEV)
    for fn in (ops.relay_soft, ops.relay_osd):
        with pytest.raises(_lib.GnndError) as e:
            fn(gdeg, x, torch.zeros(2, 3, dtype=torch.float64, device=DEV), 5)
        assert e.value.status == _lib.ERR_UNSUPPORTED


def test_nonfinite_codeword_stays_in_its_codeword():
    """A NaN and an infinity in codeword 4 of 9: the calls complete and the other eight codewords'
    outputs are the bits of the clean batch, in both modes."""
    code, B, params = 'toric_5', 9, rc.PARAMS[1]
    H, x, g, xd, args = _case(code, B, 'float64', params)
    xb = xd.clone()
    xb[4 * g.N + 3] = float('nan')
    xb[4 * g.N + 17] = float('inf')
    keep = torch.tensor([b for b in range(B) if b != 4], device=DEV)
    for mode in roc.MODES:
        for fn in (ops.relay_soft, ops.relay_osd):
            clean = fn(g, xd, *args, soft=mode)
            dirty = fn(g, xb, *args, soft=mode)
            torch.cuda.synchronize()
            for c, d in zip(clean, dirty):
                rows = (lambda t: t.view(B, g.V)) if c.numel() == B * g.V else (lambda t: t)
                assert torch.equal(rows(c)[keep], rows(d)[keep])


def test_capture_replay_follows_the_new_gate():
    """One capture of relay_osd, replayed on a second input written into the captured x: every
    output is the eager call's on that input, and the gate differs between the two."""
    code, B, dtype = 'toric_5', 9, 'float64'
    H, x1, g, xd, args = _case(code, B, dtype, rc.PARAMS[1])
    x2 = roc.inputs(code, B, dtype, rc.PARAMS[0])[1]
    sx = xd.clone()
    eager = [ops.relay_osd(g, _dev(x).unsqueeze(1), *args, soft='mean') for x in (x1, x2)]
    assert not torch.equal(eager[0][6], eager[1][6])
    out = tuple(torch.empty_like(t) for t in eager[0])
    work = torch.empty(ops.osd_gated_workspace(B), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.relay_osd(g, sx, *args, soft='mean', out=out, work=work)
    for x, want in zip((x1, x2), eager):
        sx.copy_(_dev(x).unsqueeze(1))
        for t in out:
            t.fill_(7)
        cg.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, want):
            assert torch.equal(a, b)


def test_ops_trace_as_registered_ops():
    """The four torch ops have fake kernels: shapes and dtypes without a launch, under
    FakeTensorMode and on the meta device; the real ops give the public entries' bits."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    g = graph_of('toric_5')
    for dt in (torch.float32, torch.float64):
        for dev, ctx in ((DEV, FakeTensorMode), ('meta', None)):
            with (ctx() if ctx else torch.no_grad()):
                x = torch.empty(3 * g.N, 1, dtype=dt, device=dev)
                gm = torch.empty(4, g.V, dtype=dt, device=dev)
                s = torch.ops.gnnd.relay_soft(g.gid, x, gm, 12, 10, 2, 0.75, 0.0, 'mean')
                o = torch.ops.gnnd.relay_osd(g.gid, x, gm, 12, 10, 2, 0.75, 0.0, 'mean', 'zero',
                                             'cs', 10)
                assert len(s) == 8 and len(o) == 9
                for t in s[:4] + (o[0], o[3], o[4]):
                    assert t.shape == (3 * g.V, 1) and t.dtype == dt and t.device.type == x.device.type
                for t in s[4:] + o[1:3] + o[5:]:
                    assert t.shape == (3,) and t.dtype == torch.int32
                if ctx:
                    assert torch.ops.gnnd.relay_soft_out(g.gid, x, gm, 12, 10, 2, 0.75, 0.0, 'mean',
                                                         *s) is None
                    assert torch.ops.gnnd.relay_osd_out(g.gid, x, gm, 12, 10, 2, 0.75, 0.0, 'mean',
                                                        'zero', 'cs', 10, *o) is None
    H, xs, g, xd, args = _case('toric_5', 9, 'float64', rc.PARAMS[1])
    for mode in roc.MODES:
        want = ops.relay_soft(g, xd, *args, soft=mode)
        got = torch.ops.gnnd.relay_soft(g.gid, xd, *args, mode)
        out = tuple(torch.empty_like(t) for t in want)
        torch.ops.gnnd.relay_soft_out(g.gid, xd, *args, mode, *out)
        for a, b, c in zip(want, got, out):
            assert torch.equal(a, b) and torch.equal(a, c)
        want = ops.relay_osd(g, xd, *args, soft=mode)
        got = torch.ops.gnnd.relay_osd(g.gid, xd, *args, mode, 'zero', 'cs', 10)
        out = tuple(torch.empty_like(t) for t in want)
        torch.ops.gnnd.relay_osd_out(g.gid, xd, *args, mode, 'zero', 'cs', 10, *out)
        for a, b, c in zip(want, got, out):
            assert torch.equal(a, b) and torch.equal(a, c)


def test_debug_library_runs_relay_osd_clean():
    """toric-5 B = 9 (fp64) and LDPC B = 3 (fp32) in both modes under the bounds-checked build
    (GNND_LIB, a fresh child process): no index check fires in any translation unit, and soft is
    the numpy statement's."""
    res = debug_child.run('decoder_debug_worker.py', 'relay_osd')
    assert res['equal'] == {'toric_5': True, 'ldpc_648_324': True}
