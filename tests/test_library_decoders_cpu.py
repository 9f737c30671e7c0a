"""The decoder table of gnndecode.decoders and the torch ops gnndecode.library generates from it,
without a GPU and without libgnnd.so: the schema of every gnnd:: op is pinned to the literal string
it had when the ops were written by hand, and every generated fake kernel gives the outputs its
decoder declares (count, shapes, dtypes) on meta tensors."""
import pytest
import torch

from gnndecode import decoders, library

# str(torch.ops.gnnd.NAME.default._schema) of every op, recorded from the hand-written registrations
SCHEMAS = {
    'belief_find': (
        'gnnd::belief_find(SymInt graph_id, Tensor x, SymInt iters, float alpha, float beta, bool '
        'early_stop, float scale, SymInt wmax) -> (Tensor, Tensor, Tensor, Tensor, Tensor, '
        'Tensor, Tensor, Tensor, Tensor)'),
    'belief_find_out': (
        'gnnd::belief_find_out(SymInt graph_id, Tensor x, SymInt iters, float alpha, float beta, '
        'bool early_stop, float scale, SymInt wmax, Tensor(a8!) ehat, Tensor(a9!) status, '
        'Tensor(a10!) iters_used, Tensor(a11!) bp_status, Tensor(a12!) pred, Tensor(a13!) llr, '
        'Tensor(a14!) rounds, Tensor(a15!) nfull, Tensor(a16!) events) -> ()'),
    'bpgd': (
        'gnnd::bpgd(SymInt graph_id, Tensor x, SymInt iters0, SymInt iters_round, SymInt rounds, '
        'SymInt per_round, str pick, float clamp, float alpha, float beta) -> (Tensor, Tensor, '
        'Tensor, Tensor, Tensor, Tensor)'),
    'bpgd_out': (
        'gnnd::bpgd_out(SymInt graph_id, Tensor x, SymInt iters0, SymInt iters_round, SymInt '
        'rounds, SymInt per_round, str pick, float clamp, float alpha, float beta, Tensor(a10!) '
        'ehat, Tensor(a11!) llr, Tensor(a12!) pred, Tensor(a13!) iters_used, Tensor(a14!) status, '
        'Tensor(a15!) ndec) -> ()'),
    'bplsd': (
        'gnnd::bplsd(SymInt graph_id, Tensor x, SymInt iters, float alpha, float beta, bool '
        'early_stop, str base, SymInt bits_per_step) -> (Tensor, Tensor, Tensor, Tensor, Tensor, '
        'Tensor, Tensor, Tensor, Tensor)'),
    'bplsd_out': (
        'gnnd::bplsd_out(SymInt graph_id, Tensor x, SymInt iters, float alpha, float beta, bool '
        'early_stop, str base, SymInt bits_per_step, Tensor(a8!) ehat, Tensor(a9!) status, '
        'Tensor(a10!) rounds, Tensor(a11!) nclus, Tensor(a12!) ncols, Tensor(a13!) iters_used, '
        'Tensor(a14!) bp_status, Tensor(a15!) pred, Tensor(a16!) llr) -> ()'),
    'bposd': (
        'gnnd::bposd(SymInt graph_id, Tensor x, SymInt iters, float alpha, float beta, bool '
        'early_stop, str base, str method, SymInt order) -> (Tensor, Tensor, Tensor, Tensor, '
        'Tensor, Tensor, Tensor)'),
    'bposd_layered': (
        'gnnd::bposd_layered(SymInt graph_id, Tensor x, SymInt iters, float alpha, float beta, '
        'bool early_stop, str base, str method, SymInt order) -> (Tensor, Tensor, Tensor, Tensor, '
        'Tensor, Tensor, Tensor)'),
    'bposd_layered_out': (
        'gnnd::bposd_layered_out(SymInt graph_id, Tensor x, SymInt iters, float alpha, float '
        'beta, bool early_stop, str base, str method, SymInt order, Tensor(a9!) ehat, '
        'Tensor(a10!) status, Tensor(a11!) choice, Tensor(a12!) iters_used, Tensor(a13!) '
        'bp_status, Tensor(a14!) pred, Tensor(a15!) llr) -> ()'),
    'bposd_out': (
        'gnnd::bposd_out(SymInt graph_id, Tensor x, SymInt iters, float alpha, float beta, bool '
        'early_stop, str base, str method, SymInt order, Tensor(a9!) ehat, Tensor(a10!) status, '
        'Tensor(a11!) choice, Tensor(a12!) iters_used, Tensor(a13!) bp_status, Tensor(a14!) pred, '
        'Tensor(a15!) llr) -> ()'),
    'decode': (
        'gnnd::decode(SymInt graph_id, str model, Tensor x, SymInt iters, Tensor? weights) -> '
        'Tensor'),
    'decode_out': (
        'gnnd::decode_out(SymInt graph_id, str model, Tensor x, SymInt iters, Tensor? weights, '
        'Tensor(a5!) out) -> ()'),
    'lsd': (
        'gnnd::lsd(SymInt graph_id, Tensor x, Tensor pred, str base, SymInt bits_per_step) -> '
        '(Tensor, Tensor, Tensor, Tensor, Tensor)'),
    'lsd_gated': (
        'gnnd::lsd_gated(SymInt graph_id, Tensor x, Tensor pred, Tensor gate, str base, SymInt '
        'bits_per_step, Tensor? llr) -> (Tensor, Tensor, Tensor, Tensor, Tensor)'),
    'lsd_gated_out': (
        'gnnd::lsd_gated_out(SymInt graph_id, Tensor x, Tensor pred, Tensor gate, str base, '
        'SymInt bits_per_step, Tensor? llr, Tensor(a7!) ehat, Tensor(a8!) status, Tensor(a9!) '
        'rounds, Tensor(a10!) nclus, Tensor(a11!) ncols) -> ()'),
    'lsd_out': (
        'gnnd::lsd_out(SymInt graph_id, Tensor x, Tensor pred, str base, SymInt bits_per_step, '
        'Tensor(a5!) ehat, Tensor(a6!) status, Tensor(a7!) rounds, Tensor(a8!) nclus, Tensor(a9!) '
        'ncols) -> ()'),
    'minsum': (
        'gnnd::minsum(SymInt graph_id, Tensor x, SymInt iters, float alpha, float beta, bool '
        'early_stop) -> (Tensor, Tensor, Tensor, Tensor)'),
    'minsum_layered': (
        'gnnd::minsum_layered(SymInt graph_id, Tensor x, SymInt iters, float alpha, float beta, '
        'bool early_stop) -> (Tensor, Tensor, Tensor, Tensor)'),
    'minsum_layered_out': (
        'gnnd::minsum_layered_out(SymInt graph_id, Tensor x, SymInt iters, float alpha, float '
        'beta, bool early_stop, Tensor(a6!) pred, Tensor(a7!) llr, Tensor(a8!) iters_used, '
        'Tensor(a9!) status) -> ()'),
    'minsum_out': (
        'gnnd::minsum_out(SymInt graph_id, Tensor x, SymInt iters, float alpha, float beta, bool '
        'early_stop, Tensor(a6!) pred, Tensor(a7!) llr, Tensor(a8!) iters_used, Tensor(a9!) '
        'status) -> ()'),
    'osd': (
        'gnnd::osd(SymInt graph_id, Tensor x, Tensor pred, str base, str method, SymInt order) -> '
        '(Tensor, Tensor, Tensor)'),
    'osd0': (
        'gnnd::osd0(SymInt graph_id, Tensor x, Tensor pred, str base) -> (Tensor, Tensor)'),
    'osd0_out': (
        'gnnd::osd0_out(SymInt graph_id, Tensor x, Tensor pred, str base, Tensor(a4!) ehat, '
        'Tensor(a5!) status) -> ()'),
    'osd_gated': (
        'gnnd::osd_gated(SymInt graph_id, Tensor x, Tensor pred, Tensor gate, str base, str '
        'method, SymInt order, Tensor? llr) -> (Tensor, Tensor, Tensor)'),
    'osd_gated_out': (
        'gnnd::osd_gated_out(SymInt graph_id, Tensor x, Tensor pred, Tensor gate, str base, str '
        'method, SymInt order, Tensor? llr, Tensor(a8!) ehat, Tensor(a9!) status, Tensor(a10!) '
        'choice) -> ()'),
    'osd_out': (
        'gnnd::osd_out(SymInt graph_id, Tensor x, Tensor pred, str base, str method, SymInt '
        'order, Tensor(a6!) ehat, Tensor(a7!) status, Tensor(a8!) choice) -> ()'),
    'propagate': (
        'gnnd::propagate(str variant, str flow, str aggr, Tensor edge_index, Tensor msg, Tensor? '
        'extra, SymInt dim_size, SymInt graph_id, SymInt chk_shift) -> Tensor'),
    'propagate_bwd': (
        'gnnd::propagate_bwd(str variant, str flow, str aggr, Tensor edge_index, Tensor msg, '
        'Tensor? extra, Tensor grad_out, SymInt dim_size, SymInt graph_id, SymInt chk_shift) -> '
        'Tensor'),
    'relay': (
        'gnnd::relay(SymInt graph_id, Tensor x, Tensor gammas, SymInt iters0, SymInt iters_leg, '
        'SymInt stop_after, float alpha, float beta) -> (Tensor, Tensor, Tensor, Tensor, Tensor, '
        'Tensor)'),
    'relay_osd': (
        'gnnd::relay_osd(SymInt graph_id, Tensor x, Tensor gammas, SymInt iters0, SymInt '
        'iters_leg, SymInt stop_after, float alpha, float beta, str soft, str base, str method, '
        'SymInt order) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, '
        'Tensor)'),
    'relay_osd_out': (
        'gnnd::relay_osd_out(SymInt graph_id, Tensor x, Tensor gammas, SymInt iters0, SymInt '
        'iters_leg, SymInt stop_after, float alpha, float beta, str soft, str base, str method, '
        'SymInt order, Tensor(a12!) ehat, Tensor(a13!) status, Tensor(a14!) choice, Tensor(a15!) '
        'pred, Tensor(a16!) llr, Tensor(a17!) iters_used, Tensor(a18!) relay_status, Tensor(a19!) '
        'leg, Tensor(a20!) nsol) -> ()'),
    'relay_out': (
        'gnnd::relay_out(SymInt graph_id, Tensor x, Tensor gammas, SymInt iters0, SymInt '
        'iters_leg, SymInt stop_after, float alpha, float beta, Tensor(a8!) ehat, Tensor(a9!) '
        'llr, Tensor(a10!) iters_used, Tensor(a11!) status, Tensor(a12!) leg, Tensor(a13!) nsol) '
        '-> ()'),
    'relay_soft': (
        'gnnd::relay_soft(SymInt graph_id, Tensor x, Tensor gammas, SymInt iters0, SymInt '
        'iters_leg, SymInt stop_after, float alpha, float beta, str soft) -> (Tensor, Tensor, '
        'Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)'),
    'relay_soft_out': (
        'gnnd::relay_soft_out(SymInt graph_id, Tensor x, Tensor gammas, SymInt iters0, SymInt '
        'iters_leg, SymInt stop_after, float alpha, float beta, str soft, Tensor(a9!) pred, '
        'Tensor(a10!) soft_out, Tensor(a11!) ehat, Tensor(a12!) llr, Tensor(a13!) iters_used, '
        'Tensor(a14!) status, Tensor(a15!) leg, Tensor(a16!) nsol) -> ()'),
    'uf': (
        'gnnd::uf(SymInt graph_id, Tensor x, Tensor? gate) -> (Tensor, Tensor, Tensor, Tensor)'),
    'uf_out': (
        'gnnd::uf_out(SymInt graph_id, Tensor x, Tensor? gate, Tensor(a3!) ehat, Tensor(a4!) '
        'rounds, Tensor(a5!) status, Tensor(a6!) nfull) -> ()'),
    'ufw': (
        'gnnd::ufw(SymInt graph_id, Tensor x, Tensor? llr, float scale, SymInt wmax, Tensor? '
        'gate, bool passthrough) -> (Tensor, Tensor, Tensor, Tensor, Tensor)'),
    'ufw_out': (
        'gnnd::ufw_out(SymInt graph_id, Tensor x, Tensor? llr, float scale, SymInt wmax, Tensor? '
        'gate, bool passthrough, Tensor(a7!) ehat, Tensor(a8!) rounds, Tensor(a9!) status, '
        'Tensor(a10!) nfull, Tensor(a11!) events) -> ()'),
}

# the returned order of three decoders, spelled out: a reordered table cannot agree with itself here
OUT_NAMES = {
    'bposd': ['ehat', 'status', 'choice', 'iters_used', 'bp_status', 'pred', 'llr'],
    'relay_osd': ['ehat', 'status', 'choice', 'pred', 'llr', 'iters_used', 'relay_status', 'leg',
                  'nsol'],
    'belief_find': ['ehat', 'status', 'iters_used', 'bp_status', 'pred', 'llr', 'rounds', 'nfull',
                    'events'],
}

L, B = 4, 3
V, C = 2 * L * L, L * L                       # toric-4
DIMS = (V, C, V + C, 2 * V)                   # (32, 16, 48, 64): every variable sits in two checks
SCALARS = dict(iters=5, alpha=0.75, beta=0.0, early_stop=True, base='zero', method='cs', order=3,
               iters0=4, iters_leg=3, stop_after=1, soft='last', iters_round=2, rounds=2,
               per_round=1, pick='least', clamp=25.0, scale=2.0, wmax=8, passthrough=False,
               bits_per_step=1)
ROWS = [(d, s) for d in decoders.DECODERS for s in ([''] + ['_layered'] * d.layered)]


def _registered():
    return {n for n in dir(torch.ops.gnnd) if hasattr(getattr(torch.ops.gnnd, n), 'default')}


def test_every_schema_is_the_hand_written_one():
    assert DIMS == (32, 16, 48, 64)
    assert _registered() == set(SCHEMAS)
    for name, schema in SCHEMAS.items():
        assert str(getattr(torch.ops.gnnd, name).default._schema) == schema, name


def test_table_covers_the_decoder_ops_and_keeps_the_spelled_out_orders():
    names = {d.name + s + o for d, s in ROWS for o in ('', '_out')}
    assert names == set(SCHEMAS) - {'propagate', 'propagate_bwd', 'decode', 'decode_out'}
    by_name = {d.name: d for d in decoders.DECODERS}
    for name, outs in OUT_NAMES.items():
        assert [o.name for o in by_name[name].outs] == outs, name
    assert [d.name for d in decoders.DECODERS if d.zeros] == ['uf', 'ufw']
    assert [d.name for d in decoders.DECODERS if d.short_out] == ['osd', 'osd_gated']


def _meta_args(d, dtype, with_optional):
    """The arguments of gnnd::X after graph_id, in schema order, tensors on the meta device."""
    real = dict(x=(B * (V + C), 1), pred=(B * V, 1), llr=(B * V, 1), gammas=(3, V))
    args = []
    for a in d.args.split(', '):
        kind, name = a.split()
        if not kind.startswith('Tensor'):
            args.append(SCALARS[name])
        elif kind == 'Tensor?' and not with_optional:
            args.append(None)
        elif name == 'gate':
            args.append(torch.empty(B, dtype=torch.int32, device='meta'))
        else:
            args.append(torch.empty(real[name], dtype=dtype, device='meta'))
    return args


@pytest.mark.parametrize('with_optional', [False, True], ids=['none', 'given'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('d,suffix', ROWS, ids=[d.name + s for d, s in ROWS])
def test_fake_kernels_give_the_declared_outputs(d, suffix, dtype, with_optional):
    gid = 20_000 + len(library._DIMS)
    library._DIMS[gid] = DIMS
    args = _meta_args(d, dtype, with_optional)
    outs = getattr(torch.ops.gnnd, d.name + suffix)(gid, *args)
    assert isinstance(outs, tuple) and len(outs) == len(d.outs)
    for o, t in zip(d.outs, outs):
        assert o.kind in ('real', 'int') and t.device.type == 'meta', o.name
        if o.kind == 'real':
            assert tuple(t.shape) == (B * V, 1) and t.dtype == dtype, o.name
        else:
            assert tuple(t.shape) == (B,) and t.dtype == torch.int32, o.name
    assert getattr(torch.ops.gnnd, d.name + suffix + '_out')(gid, *args, *outs) is None
