"""Every decoder of the table in gnndecode.decoders on the device, three ways: the eager call
with out=None, the eager call into sentinel-filled `out` tensors and the generated torch ops
gnnd::X / gnnd::X_out must give bit-identical tensors, and an optional output left None must not
change the others.  toric-4, B = 3, both dtypes: well inside every kernel's plan.  This guards the
argument order and the allocation of the generated code, nothing else; what the decoders compute
is the business of their own tests."""
import numpy as np
import pytest
import torch

import gnndecode as gd
from gnndecode import decoders, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
L, B = 4, 3
FLIP = (0.04, 0.10, 0.16)       # one flip probability per codeword
SCALARS = dict(iters=8, alpha=0.75, beta=0.0, early_stop=True, base='zero', method='cs', order=4,
               iters0=5, iters_leg=4, stop_after=1, soft='last', iters_round=3, rounds=3,
               per_round=1, pick='least', clamp=25.0, scale=2.0, wmax=8, passthrough=False,
               bits_per_step=1)
# (decoder, op suffix, optional tensor inputs given): both where the decoder has optional tensors
CASES = [(d, s, opt) for d in decoders.DECODERS for s in ([''] + ['_layered'] * d.layered)
         for opt in ([False, True] if any(o for _, o in d.tensors) else [False])]
_CACHE = {}


def _graph():
    if 'g' not in _CACHE:
        _CACHE['g'] = gd.TannerGraph(gd.codes.toric_code(L), device=DEV)
    return _CACHE['g']


def _tensors(dtype):
    """x: the channel LLR on the variable rows, +/-1 for a syndrome bit 0 / 1 of a random error on
    the check rows; pred and llr: a short min-sum run on x; gate [1, 0, 1]; gammas: three legs."""
    if dtype not in _CACHE:
        g = _graph()
        H = np.asarray(gd.codes.toric_code(L))
        rng = np.random.default_rng(20264)
        p = np.array(FLIP)
        e = rng.random((B, g.V)) < p[:, None]
        x = np.empty((B, g.N))
        x[:, :g.V] = np.log((1 - p) / p)[:, None]
        x[:, g.V:] = 1 - 2 * ((e.astype(np.int64) @ (H != 0)) % 2)
        x = torch.from_numpy(x.reshape(-1, 1)).to(device=DEV, dtype=dtype)
        pred, llr, _, _ = ops.minsum(g, x, 2)
        _CACHE[dtype] = dict(x=x, pred=pred, llr=llr, gammas=ops.relay_gammas(g.V, 3, dtype=dtype,
                                                                             device=DEV),
                             gate=torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV))
    return _CACHE[dtype]


def _args(d, dtype, with_optional):
    """(names, values) of d's arguments after the graph, in schema order."""
    t = _tensors(dtype)
    names, values = [], []
    for a in d.args.split(', '):
        kind, name = a.split()
        names.append(name)
        if not kind.startswith('Tensor'):
            values.append(SCALARS[name])
        else:
            values.append(None if kind == 'Tensor?' and not with_optional else t[name])
    return names, values


def _sentinels(d, dtype):
    g = _graph()
    return tuple(torch.full((B * g.V, 1), 7, dtype=dtype, device=DEV) if o.kind == 'real'
                 else torch.full((B,), 7, dtype=torch.int32, device=DEV) for o in d.outs)


def _same(a, b, rows, what):
    assert len(a) == len(b), what
    for o, s, t in zip(what[0].outs, a, b):
        assert s.dtype == t.dtype and s.shape == t.shape, (what[1:], o.name)
        assert torch.equal(s.view(B, -1)[rows], t.view(B, -1)[rows]), (what[1:], o.name)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('d,suffix,with_optional', CASES,
                         ids=[d.name + s + '-given' * opt for d, s, opt in CASES])
def test_eager_into_out_and_the_generated_ops_agree(d, suffix, with_optional, dtype):
    g = _graph()
    names, values = _args(d, dtype, with_optional)
    kw = dict(zip(names, values), **({'schedule': 'layered'} if suffix else {}))
    eager = getattr(ops, d.name)(g, **kw)
    assert isinstance(eager, tuple) and len(eager) == len(d.outs)
    # a gate of uf / ufw leaves the rows it skips unwritten: compare the rows it lets in
    gated = d.zeros and kw.get('gate') is not None
    rows = kw['gate'].bool() if gated else slice(None)
    filled = _sentinels(d, dtype)
    got = getattr(ops, d.name)(g, **kw, out=filled)
    assert all(a is b for a, b in zip(got, filled))
    _same(eager, filled, rows, (d, suffix, 'eager into out'))
    op = getattr(torch.ops.gnnd, d.name + suffix)(g.gid, *values)
    _same(eager, op, rows, (d, suffix, 'gnnd::X'))
    if gated:
        for t in op:                            # the op returns zeros in the skipped rows
            assert not t.view(B, -1)[~rows].any()
        for t in filled:
            assert bool((t.view(B, -1)[~rows] == 7).all())
    op_out = _sentinels(d, dtype)
    assert getattr(torch.ops.gnnd, d.name + suffix + '_out')(g.gid, *values, *op_out) is None
    _same(eager, op_out, rows, (d, suffix, 'gnnd::X_out'))
    # an optional output left out comes back as None and the others keep their bits
    for i, o in enumerate(d.outs):
        if o.optional:
            part = tuple(None if j == i else t for j, t in enumerate(_sentinels(d, dtype)))
            res = getattr(ops, d.name)(g, **kw, out=part)
            assert len(res) == len(d.outs) and res[i] is None, o.name
            keep = [j for j in range(len(d.outs)) if j != i]
            _same([eager[j] for j in keep], [res[j] for j in keep], rows,
                  (d._replace(outs=tuple(d.outs[j] for j in keep)), suffix, 'without ' + o.name))
    torch.cuda.synchronize()
