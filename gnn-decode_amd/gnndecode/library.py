"""torch.library registration of the device operators.

The public entries of `gnndecode.ops` dispatch to these custom ops whenever they are traced
(torch.compile / FX: `torch.compiler.is_compiling()`), so the decoder is a set of named
operators with fake kernels for shape propagation instead of opaque ctypes calls; eager
calls run the same implementation functions directly (the Python dispatcher round trip of
a custom op costs more than the 0.47 ms headline kernel, measured r02n):

  gnnd::propagate(variant, flow, aggr, edge_index, msg, extra?, dim_size, graph_id, chk_shift)
      one reference `propagate` body (quantum/decoder_v2_4.py:85-148 and the other scripts'
      copies); autograd through gnnd::propagate_bwd
  gnnd::propagate_bwd(..., grad_out, ...)  d out / d msg (HIP backward kernels)
  gnnd::decode(graph_id, model, x, iters, weights?)          fused T-iteration decoder
  gnnd::decode_out(graph_id, model, x, iters, weights?, out)  the same into `out` (mutates)
  gnnd::osd0(graph_id, x, pred, base) -> (ehat, status)      OSD-0 post-processing of a decode
  gnnd::osd0_out(graph_id, x, pred, base, ehat, status)       the same into its outputs (mutates)
  gnnd::osd(graph_id, x, pred, base, method, order) -> (ehat, status, choice)   higher-order OSD
  gnnd::osd_out(graph_id, x, pred, base, method, order, ehat, status, choice)   the same, mutating
  gnnd::minsum(graph_id, x, iters, alpha, beta, early_stop) -> (pred, llr, iters_used, status)
      min-sum BP with the syndrome-converged early stop
  gnnd::minsum_out(graph_id, x, iters, alpha, beta, early_stop, pred, llr, iters_used, status)
      the same into its outputs (mutates)
  gnnd::osd_gated(graph_id, x, pred, gate, base, method, order, llr?) -> (ehat, status, choice)
      osd on the codewords with gate != 0, the hard decision passed through elsewhere
  gnnd::osd_gated_out(graph_id, x, pred, gate, base, method, order, llr?, ehat, status, choice)
  gnnd::bposd(graph_id, x, iters, alpha, beta, early_stop, base, method, order)
      -> (ehat, status, choice, iters_used, bp_status, pred, llr)   minsum, then osd_gated
  gnnd::bposd_out(graph_id, x, iters, alpha, beta, early_stop, base, method, order, ehat, status,
      choice, iters_used, bp_status, pred, llr)                     the same, mutating

  gnnd::minsum_layered, gnnd::minsum_layered_out, gnnd::bposd_layered, gnnd::bposd_layered_out
      minsum / bposd on the layered schedule (gnnd_minsum_layered, gnnd_bposd_layered): the
      signatures, outputs and fake kernels of the flooding ops

  gnnd::relay(graph_id, x, gammas, iters0, iters_leg, stop_after, alpha, beta)
      -> (ehat, llr, iters_used, status, leg, nsol)   relay min-sum BP: memory-strength legs, the
      lightest solution kept
  gnnd::relay_out(graph_id, x, gammas, iters0, iters_leg, stop_after, alpha, beta, ehat, llr,
      iters_used, status, leg, nsol)                  the same into its outputs (mutates)
  gnnd::relay_soft(graph_id, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft)
      -> (pred, soft, ehat, llr, iters_used, status, leg, nsol)   relay with a soft output ('last' /
      'mean' posteriors for the unsolved codewords); gnnd::relay_soft_out mutates its eight outputs
  gnnd::relay_osd(graph_id, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft, base,
      method, order) -> (ehat, status, choice, pred, llr, iters_used, relay_status, leg, nsol)
      relay_soft, then osd_gated on the unsolved codewords; gnnd::relay_osd_out mutates its nine
  gnnd::bpgd(graph_id, x, iters0, iters_round, rounds, per_round, pick, clamp, alpha, beta)
      -> (ehat, llr, pred, iters_used, status, ndec)   min-sum BP with guided decimation: priors
      frozen between BP rounds; gnnd::bpgd_out mutates its six outputs
  gnnd::uf(graph_id, x, gate?) -> (ehat, rounds, status, nfull)   the union-find decoder of a
      matchable graph; rows a gate skips come back as zeros.  gnnd::uf_out(graph_id, x, gate?,
      ehat, rounds, status, nfull) mutates its four outputs and leaves the skipped rows as they were
  gnnd::ufw(graph_id, x, llr?, scale, wmax, gate?, passthrough) -> (ehat, rounds, status, nfull,
      events)   weighted union-find: uf with an edge's length its quantised reliability (llr, else
      the priors in x); rows a gate skips come back as zeros.  gnnd::ufw_out mutates its five outputs
  gnnd::belief_find(graph_id, x, iters, alpha, beta, early_stop, scale, wmax)
      -> (ehat, status, iters_used, bp_status, pred, llr, rounds, nfull, events)   minsum, then ufw
      on its posteriors for the codewords it left unsolved; gnnd::belief_find_out mutates its nine
  gnnd::lsd(graph_id, x, pred, base, bits_per_step) -> (ehat, status, rounds, nclus, ncols)
      localized-statistics decoding: clusters around the unsatisfied checks, each solved by osd0's
      elimination over its own columns; gnnd::lsd_out mutates its five outputs
  gnnd::lsd_gated(graph_id, x, pred, gate, base, bits_per_step, llr?) -> the same five, lsd on the
      codewords with gate != 0, the hard decision passed through elsewhere; gnnd::lsd_gated_out
  gnnd::bplsd(graph_id, x, iters, alpha, beta, early_stop, base, bits_per_step)
      -> (ehat, status, rounds, nclus, ncols, iters_used, bp_status, pred, llr)   minsum, then
      lsd_gated; gnnd::bplsd_out mutates its nine

The single-codeword Tanner graph is a device object owned by libgnnd, not a tensor: ops
take the integer id that `register_graph` hands out (TannerGraph does this on creation;
-1 = no graph: the generic kernels).  Implementations are the ctypes launches in
`gnndecode.ops` (`_propagate_impl`, `_decode_impl`, and each decoder's `_X_impl`): no CPU kernel
is registered, so a CPU tensor reaching an op fails in the dispatcher instead of falling back.
propagate and decode are registered by hand below; every op from gnnd::osd0 on is generated
from the decoder's declaration in `gnndecode.decoders` (`_register`).
"""
import weakref
from typing import Optional

import torch
from torch import Tensor

from . import decoders

_GRAPHS = {}          # id -> weakref(TannerGraph)
_DIMS = {}            # id -> (V, C, N, E): shapes for the fake kernels
_NEXT = [0]


def register_graph(graph) -> int:
    gid = _NEXT[0]
    _NEXT[0] += 1
    _GRAPHS[gid] = weakref.ref(graph)
    _DIMS[gid] = (graph.V, graph.C, graph.N, graph.E)
    return gid


def graph_of(gid):
    if gid < 0:
        return None
    ref = _GRAPHS.get(gid)
    g = ref() if ref is not None else None
    if g is None:
        raise RuntimeError(f'gnnd: Tanner graph {gid} no longer exists')
    return g


def _out_rows(gid, model, B, iters=1):
    V, C, N, E = _DIMS[gid]
    if model == 'v30':
        return 2 * B * N
    return iters * B * V if model == 'v22' else B * V


# ---------------------------------------------------------------------------------------
# propagate
# ---------------------------------------------------------------------------------------
@torch.library.custom_op('gnnd::propagate', mutates_args=(), device_types='cuda')
def propagate(variant: str, flow: str, aggr: str, edge_index: Tensor, msg: Tensor,
              extra: Optional[Tensor], dim_size: int, graph_id: int, chk_shift: int) -> Tensor:
    from . import ops
    return ops._propagate_impl(variant, flow, aggr, edge_index, msg, extra, dim_size,
                               graph_of(graph_id), None if chk_shift < 0 else chk_shift)


@propagate.register_fake
def _propagate_fake(variant, flow, aggr, edge_index, msg, extra, dim_size, graph_id, chk_shift):
    from . import ops
    return msg.new_empty(msg.size(0), ops.propagate_width(variant, flow))


@torch.library.custom_op('gnnd::propagate_bwd', mutates_args=(), device_types='cuda')
def propagate_bwd(variant: str, flow: str, aggr: str, edge_index: Tensor, msg: Tensor,
                  extra: Optional[Tensor], grad_out: Tensor, dim_size: int, graph_id: int,
                  chk_shift: int) -> Tensor:
    from . import ops
    return ops._propagate_bwd_impl(variant, flow, aggr, edge_index, msg, extra, grad_out,
                                   dim_size, graph_of(graph_id),
                                   None if chk_shift < 0 else chk_shift)


@propagate_bwd.register_fake
def _propagate_bwd_fake(variant, flow, aggr, edge_index, msg, extra, grad_out, dim_size,
                        graph_id, chk_shift):
    return torch.empty_like(msg)


def _prop_setup(ctx, inputs, output):
    variant, flow, aggr, edge_index, msg, extra, dim_size, graph_id, chk_shift = inputs
    ctx.save_for_backward(edge_index, msg, extra)
    ctx.args = (variant, flow, aggr, dim_size, graph_id, chk_shift)


def _prop_backward(ctx, grad_out):
    edge_index, msg, extra = ctx.saved_tensors
    variant, flow, aggr, dim_size, graph_id, chk_shift = ctx.args
    if aggr != 'add':
        raise NotImplementedError(f'no backward for aggr={aggr!r}')
    gmsg = torch.ops.gnnd.propagate_bwd(variant, flow, aggr, edge_index, msg, extra,
                                        grad_out.contiguous(), dim_size, graph_id, chk_shift)
    return None, None, None, None, gmsg, None, None, None, None


torch.library.register_autograd('gnnd::propagate', _prop_backward, setup_context=_prop_setup)


# ---------------------------------------------------------------------------------------
# fused decoder
# ---------------------------------------------------------------------------------------
@torch.library.custom_op('gnnd::decode', mutates_args=(), device_types='cuda')
def decode(graph_id: int, model: str, x: Tensor, iters: int, weights: Optional[Tensor]) -> Tensor:
    from . import ops
    g = graph_of(graph_id)
    out = torch.empty(ops.decode_out_rows(g, model, x.numel() // g.N, iters), 1, dtype=x.dtype,
                      device=x.device)
    ops._decode_impl(g, model, x, iters, weights, out)
    return out


@decode.register_fake
def _decode_fake(graph_id, model, x, iters, weights):
    N = _DIMS[graph_id][2]
    return x.new_empty(_out_rows(graph_id, model, x.numel() // N, iters), 1)


@torch.library.custom_op('gnnd::decode_out', mutates_args=('out',), device_types='cuda')
def decode_out(graph_id: int, model: str, x: Tensor, iters: int, weights: Optional[Tensor],
               out: Tensor) -> None:
    from . import ops
    ops._decode_impl(graph_of(graph_id), model, x, iters, weights, out)


@decode_out.register_fake
def _decode_out_fake(graph_id, model, x, iters, weights, out):
    return None


# ---------------------------------------------------------------------------------------
# the decoders: gnnd::X, gnnd::X_out and both fake kernels, generated from the declarations in
# gnndecode.decoders; the layered ops are further rows that reuse the flooding declaration
# ---------------------------------------------------------------------------------------
def _contiguous(args):
    return tuple(a.contiguous() if isinstance(a, Tensor) else a for a in args)


def _register(d, suffix=''):
    """Register gnnd::X{suffix} (allocates d's outputs and returns them) and gnnd::X{suffix}_out
    (writes into them, returns None) over ops._X_impl, each with its fake kernel.  The ops take
    graph_id, then d.args; X_out then d's outputs, all required."""
    name = d.name + suffix
    impl = getattr(decoders, f'_{d.name}_impl')
    kw = {'schedule': 'layered'} if suffix else {}
    arg_names = [a.split()[1] for a in d.args.split(', ')]
    nin, iref = len(arg_names), arg_names.index(d.batch)
    new = torch.zeros if d.zeros else torch.empty    # zeros: the rows a gate skips are not written

    def outputs(graph_id, ref, new):
        V, C, N, E = _DIMS[graph_id]
        return decoders._new_outputs(d, ref, ref.numel() // (N if d.batch == 'x' else V), V, new)

    def op(graph_id, *args):
        args = _contiguous(args)
        outs = outputs(graph_id, args[iref], new)
        impl(graph_of(graph_id), *args, *outs, **kw)
        return outs

    def op_out(graph_id, *args):
        impl(graph_of(graph_id), *_contiguous(args[:nin]), *args[nin:], **kw)

    returns = ', '.join(['Tensor'] * len(d.outs))
    mutated = ', '.join(f'Tensor(a{1 + nin + i}!) {o.arg}' for i, o in enumerate(d.outs))
    new_op = torch.library.custom_op(
        f'gnnd::{name}', op, mutates_args=(), device_types='cuda',
        schema=f'(SymInt graph_id, {d.args}) -> ({returns})')
    new_op.register_fake(lambda graph_id, *args: outputs(graph_id, args[iref], torch.empty))
    out_op = torch.library.custom_op(
        f'gnnd::{name}_out', op_out, mutates_args=tuple(o.arg for o in d.outs),
        device_types='cuda', schema=f'(SymInt graph_id, {d.args}, {mutated}) -> ()')
    out_op.register_fake(lambda graph_id, *args: None)
    globals()[name], globals()[name + '_out'] = new_op, out_op


for _d in decoders.DECODERS:
    _register(_d)
    if _d.layered:
        _register(_d, '_layered')
