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
`gnndecode.ops` (`_propagate_impl`, `_decode_impl`): no CPU kernel is registered, so a CPU
tensor reaching an op fails in the dispatcher instead of falling back.
"""
import weakref
from typing import Optional, Tuple

import torch
from torch import Tensor

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
# OSD-0 post-processing
# ---------------------------------------------------------------------------------------
@torch.library.custom_op('gnnd::osd0', mutates_args=(), device_types='cuda')
def osd0(graph_id: int, x: Tensor, pred: Tensor, base: str) -> Tuple[Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    pred = pred.contiguous()
    ehat = torch.empty_like(pred)
    status = torch.empty(pred.numel() // g.V, dtype=torch.int32, device=pred.device)
    ops._osd0_impl(g, x.contiguous(), pred, base, ehat, status)
    return ehat, status


@osd0.register_fake
def _osd0_fake(graph_id, x, pred, base):
    V = _DIMS[graph_id][0]
    return (torch.empty_like(pred, memory_format=torch.contiguous_format),
            pred.new_empty(pred.numel() // V, dtype=torch.int32))


@torch.library.custom_op('gnnd::osd0_out', mutates_args=('ehat', 'status'), device_types='cuda')
def osd0_out(graph_id: int, x: Tensor, pred: Tensor, base: str, ehat: Tensor,
             status: Tensor) -> None:
    from . import ops
    ops._osd0_impl(graph_of(graph_id), x.contiguous(), pred.contiguous(), base, ehat, status)


@osd0_out.register_fake
def _osd0_out_fake(graph_id, x, pred, base, ehat, status):
    return None


# ---------------------------------------------------------------------------------------
# higher-order OSD post-processing (combination sweep, exhaustive)
# ---------------------------------------------------------------------------------------
@torch.library.custom_op('gnnd::osd', mutates_args=(), device_types='cuda')
def osd(graph_id: int, x: Tensor, pred: Tensor, base: str, method: str,
        order: int) -> Tuple[Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    pred = pred.contiguous()
    B = pred.numel() // g.V
    ehat = torch.empty_like(pred)
    status = torch.empty(B, dtype=torch.int32, device=pred.device)
    choice = torch.empty(B, dtype=torch.int32, device=pred.device)
    ops._osd_impl(g, x.contiguous(), pred, base, method, order, ehat, status, choice)
    return ehat, status, choice


@osd.register_fake
def _osd_fake(graph_id, x, pred, base, method, order):
    V = _DIMS[graph_id][0]
    B = pred.numel() // V
    return (torch.empty_like(pred, memory_format=torch.contiguous_format),
            pred.new_empty(B, dtype=torch.int32), pred.new_empty(B, dtype=torch.int32))


@torch.library.custom_op('gnnd::osd_out', mutates_args=('ehat', 'status', 'choice'),
                         device_types='cuda')
def osd_out(graph_id: int, x: Tensor, pred: Tensor, base: str, method: str, order: int,
            ehat: Tensor, status: Tensor, choice: Tensor) -> None:
    from . import ops
    ops._osd_impl(graph_of(graph_id), x.contiguous(), pred.contiguous(), base, method, order,
                  ehat, status, choice)


@osd_out.register_fake
def _osd_out_fake(graph_id, x, pred, base, method, order, ehat, status, choice):
    return None


# ---------------------------------------------------------------------------------------
# min-sum BP with the syndrome-converged early stop
# ---------------------------------------------------------------------------------------
@torch.library.custom_op('gnnd::minsum', mutates_args=(), device_types='cuda')
def minsum(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float,
           early_stop: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    pred = torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device)
    llr = torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device)
    iters_used = torch.empty(B, dtype=torch.int32, device=x.device)
    status = torch.empty(B, dtype=torch.int32, device=x.device)
    ops._minsum_impl(g, x, iters, alpha, beta, early_stop, pred, llr, iters_used, status)
    return pred, llr, iters_used, status


@minsum.register_fake
def _minsum_fake(graph_id, x, iters, alpha, beta, early_stop):
    V, C, N, E = _DIMS[graph_id]
    B = x.numel() // N
    return (x.new_empty(B * V, 1), x.new_empty(B * V, 1), x.new_empty(B, dtype=torch.int32),
            x.new_empty(B, dtype=torch.int32))


@torch.library.custom_op('gnnd::minsum_out',
                         mutates_args=('pred', 'llr', 'iters_used', 'status'), device_types='cuda')
def minsum_out(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float, early_stop: bool,
               pred: Tensor, llr: Tensor, iters_used: Tensor, status: Tensor) -> None:
    from . import ops
    ops._minsum_impl(graph_of(graph_id), x.contiguous(), iters, alpha, beta, early_stop, pred,
                     llr, iters_used, status)


@minsum_out.register_fake
def _minsum_out_fake(graph_id, x, iters, alpha, beta, early_stop, pred, llr, iters_used, status):
    return None


# ---------------------------------------------------------------------------------------
# gated OSD and the one-call BP+OSD decoder
# ---------------------------------------------------------------------------------------
@torch.library.custom_op('gnnd::osd_gated', mutates_args=(), device_types='cuda')
def osd_gated(graph_id: int, x: Tensor, pred: Tensor, gate: Tensor, base: str, method: str,
              order: int, llr: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    pred = pred.contiguous()
    B = pred.numel() // g.V
    ehat = torch.empty_like(pred)
    status = torch.empty(B, dtype=torch.int32, device=pred.device)
    choice = torch.empty(B, dtype=torch.int32, device=pred.device)
    ops._osd_gated_impl(g, x.contiguous(), pred, gate.contiguous(), base, method, order,
                        None if llr is None else llr.contiguous(), ehat, status, choice)
    return ehat, status, choice


@osd_gated.register_fake
def _osd_gated_fake(graph_id, x, pred, gate, base, method, order, llr):
    V = _DIMS[graph_id][0]
    B = pred.numel() // V
    return (torch.empty_like(pred, memory_format=torch.contiguous_format),
            pred.new_empty(B, dtype=torch.int32), pred.new_empty(B, dtype=torch.int32))


@torch.library.custom_op('gnnd::osd_gated_out', mutates_args=('ehat', 'status', 'choice'),
                         device_types='cuda')
def osd_gated_out(graph_id: int, x: Tensor, pred: Tensor, gate: Tensor, base: str, method: str,
                  order: int, llr: Optional[Tensor], ehat: Tensor, status: Tensor,
                  choice: Tensor) -> None:
    from . import ops
    ops._osd_gated_impl(graph_of(graph_id), x.contiguous(), pred.contiguous(), gate.contiguous(),
                        base, method, order, None if llr is None else llr.contiguous(), ehat,
                        status, choice)


@osd_gated_out.register_fake
def _osd_gated_out_fake(graph_id, x, pred, gate, base, method, order, llr, ehat, status, choice):
    return None


@torch.library.custom_op('gnnd::bposd', mutates_args=(), device_types='cuda')
def bposd(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float, early_stop: bool,
          base: str, method: str, order: int
          ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    ehat, pred, llr = (torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device) for _ in range(3))
    status, choice, iters_used, bp_status = (torch.empty(B, dtype=torch.int32, device=x.device)
                                             for _ in range(4))
    ops._bposd_impl(g, x, iters, alpha, beta, early_stop, base, method, order, ehat, status, choice,
                    iters_used, bp_status, pred, llr)
    return ehat, status, choice, iters_used, bp_status, pred, llr


@bposd.register_fake
def _bposd_fake(graph_id, x, iters, alpha, beta, early_stop, base, method, order):
    V, C, N, E = _DIMS[graph_id]
    B = x.numel() // N

    def ints():
        return x.new_empty(B, dtype=torch.int32)
    return (x.new_empty(B * V, 1), ints(), ints(), ints(), ints(), x.new_empty(B * V, 1),
            x.new_empty(B * V, 1))


@torch.library.custom_op('gnnd::bposd_out',
                         mutates_args=('ehat', 'status', 'choice', 'iters_used', 'bp_status',
                                       'pred', 'llr'), device_types='cuda')
def bposd_out(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float, early_stop: bool,
              base: str, method: str, order: int, ehat: Tensor, status: Tensor, choice: Tensor,
              iters_used: Tensor, bp_status: Tensor, pred: Tensor, llr: Tensor) -> None:
    from . import ops
    ops._bposd_impl(graph_of(graph_id), x.contiguous(), iters, alpha, beta, early_stop, base, method,
                    order, ehat, status, choice, iters_used, bp_status, pred, llr)


@bposd_out.register_fake
def _bposd_out_fake(graph_id, x, iters, alpha, beta, early_stop, base, method, order, ehat, status,
                    choice, iters_used, bp_status, pred, llr):
    return None


# ---------------------------------------------------------------------------------------
# the layered schedule: the same signatures, outputs and fake kernels as the flooding ops
# ---------------------------------------------------------------------------------------
@torch.library.custom_op('gnnd::minsum_layered', mutates_args=(), device_types='cuda')
def minsum_layered(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float,
                   early_stop: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    pred = torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device)
    llr = torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device)
    iters_used = torch.empty(B, dtype=torch.int32, device=x.device)
    status = torch.empty(B, dtype=torch.int32, device=x.device)
    ops._minsum_impl(g, x, iters, alpha, beta, early_stop, pred, llr, iters_used, status,
                     schedule='layered')
    return pred, llr, iters_used, status


minsum_layered.register_fake(_minsum_fake)


@torch.library.custom_op('gnnd::minsum_layered_out',
                         mutates_args=('pred', 'llr', 'iters_used', 'status'), device_types='cuda')
def minsum_layered_out(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float,
                       early_stop: bool, pred: Tensor, llr: Tensor, iters_used: Tensor,
                       status: Tensor) -> None:
    from . import ops
    ops._minsum_impl(graph_of(graph_id), x.contiguous(), iters, alpha, beta, early_stop, pred,
                     llr, iters_used, status, schedule='layered')


minsum_layered_out.register_fake(_minsum_out_fake)


@torch.library.custom_op('gnnd::bposd_layered', mutates_args=(), device_types='cuda')
def bposd_layered(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float,
                  early_stop: bool, base: str, method: str, order: int
                  ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    ehat, pred, llr = (torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device) for _ in range(3))
    status, choice, iters_used, bp_status = (torch.empty(B, dtype=torch.int32, device=x.device)
                                             for _ in range(4))
    ops._bposd_impl(g, x, iters, alpha, beta, early_stop, base, method, order, ehat, status, choice,
                    iters_used, bp_status, pred, llr, schedule='layered')
    return ehat, status, choice, iters_used, bp_status, pred, llr


bposd_layered.register_fake(_bposd_fake)


@torch.library.custom_op('gnnd::bposd_layered_out',
                         mutates_args=('ehat', 'status', 'choice', 'iters_used', 'bp_status',
                                       'pred', 'llr'), device_types='cuda')
def bposd_layered_out(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float,
                      early_stop: bool, base: str, method: str, order: int, ehat: Tensor,
                      status: Tensor, choice: Tensor, iters_used: Tensor, bp_status: Tensor,
                      pred: Tensor, llr: Tensor) -> None:
    from . import ops
    ops._bposd_impl(graph_of(graph_id), x.contiguous(), iters, alpha, beta, early_stop, base, method,
                    order, ehat, status, choice, iters_used, bp_status, pred, llr,
                    schedule='layered')


bposd_layered_out.register_fake(_bposd_out_fake)



# ---------------------------------------------------------------------------------------
# relay min-sum BP
# ---------------------------------------------------------------------------------------
@torch.library.custom_op('gnnd::relay', mutates_args=(), device_types='cuda')
def relay(graph_id: int, x: Tensor, gammas: Tensor, iters0: int, iters_leg: int, stop_after: int,
          alpha: float, beta: float) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    ehat = torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device)
    llr = torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device)
    ints = tuple(torch.empty(B, dtype=torch.int32, device=x.device) for _ in range(4))
    ops._relay_impl(g, x, gammas.contiguous(), iters0, iters_leg, stop_after, alpha, beta, ehat,
                    llr, *ints)
    return (ehat, llr) + ints


@relay.register_fake
def _relay_fake(graph_id, x, gammas, iters0, iters_leg, stop_after, alpha, beta):
    V, C, N, E = _DIMS[graph_id]
    B = x.numel() // N
    return ((x.new_empty(B * V, 1), x.new_empty(B * V, 1))
            + tuple(x.new_empty(B, dtype=torch.int32) for _ in range(4)))


@torch.library.custom_op('gnnd::relay_out',
                         mutates_args=('ehat', 'llr', 'iters_used', 'status', 'leg', 'nsol'),
                         device_types='cuda')
def relay_out(graph_id: int, x: Tensor, gammas: Tensor, iters0: int, iters_leg: int,
              stop_after: int, alpha: float, beta: float, ehat: Tensor, llr: Tensor,
              iters_used: Tensor, status: Tensor, leg: Tensor, nsol: Tensor) -> None:
    from . import ops
    ops._relay_impl(graph_of(graph_id), x.contiguous(), gammas.contiguous(), iters0, iters_leg,
                    stop_after, alpha, beta, ehat, llr, iters_used, status, leg, nsol)


@relay_out.register_fake
def _relay_out_fake(graph_id, x, gammas, iters0, iters_leg, stop_after, alpha, beta, ehat, llr,
                    iters_used, status, leg, nsol):
    return None


# ---------------------------------------------------------------------------------------
# relay with a soft output, and relay followed by gated OSD
# ---------------------------------------------------------------------------------------
@torch.library.custom_op('gnnd::relay_soft', mutates_args=(), device_types='cuda')
def relay_soft(graph_id: int, x: Tensor, gammas: Tensor, iters0: int, iters_leg: int,
               stop_after: int, alpha: float, beta: float, soft: str
               ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    real = tuple(torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device) for _ in range(4))
    ints = tuple(torch.empty(B, dtype=torch.int32, device=x.device) for _ in range(4))
    ops._relay_soft_impl(g, x, gammas.contiguous(), iters0, iters_leg, stop_after, alpha, beta,
                         soft, *real, *ints)
    return real + ints


@relay_soft.register_fake
def _relay_soft_fake(graph_id, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft):
    V, C, N, E = _DIMS[graph_id]
    B = x.numel() // N
    return (tuple(x.new_empty(B * V, 1) for _ in range(4))
            + tuple(x.new_empty(B, dtype=torch.int32) for _ in range(4)))


@torch.library.custom_op('gnnd::relay_soft_out',
                         mutates_args=('pred', 'soft_out', 'ehat', 'llr', 'iters_used', 'status',
                                       'leg', 'nsol'), device_types='cuda')
def relay_soft_out(graph_id: int, x: Tensor, gammas: Tensor, iters0: int, iters_leg: int,
                   stop_after: int, alpha: float, beta: float, soft: str, pred: Tensor,
                   soft_out: Tensor, ehat: Tensor, llr: Tensor, iters_used: Tensor, status: Tensor,
                   leg: Tensor, nsol: Tensor) -> None:
    from . import ops
    ops._relay_soft_impl(graph_of(graph_id), x.contiguous(), gammas.contiguous(), iters0, iters_leg,
                         stop_after, alpha, beta, soft, pred, soft_out, ehat, llr, iters_used,
                         status, leg, nsol)


@relay_soft_out.register_fake
def _relay_soft_out_fake(graph_id, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft,
                         pred, soft_out, ehat, llr, iters_used, status, leg, nsol):
    return None


@torch.library.custom_op('gnnd::relay_osd', mutates_args=(), device_types='cuda')
def relay_osd(graph_id: int, x: Tensor, gammas: Tensor, iters0: int, iters_leg: int,
              stop_after: int, alpha: float, beta: float, soft: str, base: str, method: str,
              order: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor,
                                   Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    ehat, pred, llr = (torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device) for _ in range(3))
    status, choice, iters_used, relay_status, leg, nsol = (
        torch.empty(B, dtype=torch.int32, device=x.device) for _ in range(6))
    ops._relay_osd_impl(g, x, gammas.contiguous(), iters0, iters_leg, stop_after, alpha, beta, soft,
                        base, method, order, ehat, status, choice, pred, llr, iters_used,
                        relay_status, leg, nsol)
    return ehat, status, choice, pred, llr, iters_used, relay_status, leg, nsol


@relay_osd.register_fake
def _relay_osd_fake(graph_id, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft, base,
                    method, order):
    V, C, N, E = _DIMS[graph_id]
    B = x.numel() // N

    def ints():
        return x.new_empty(B, dtype=torch.int32)
    return (x.new_empty(B * V, 1), ints(), ints(), x.new_empty(B * V, 1), x.new_empty(B * V, 1),
            ints(), ints(), ints(), ints())


@torch.library.custom_op('gnnd::relay_osd_out',
                         mutates_args=('ehat', 'status', 'choice', 'pred', 'llr', 'iters_used',
                                       'relay_status', 'leg', 'nsol'), device_types='cuda')
def relay_osd_out(graph_id: int, x: Tensor, gammas: Tensor, iters0: int, iters_leg: int,
                  stop_after: int, alpha: float, beta: float, soft: str, base: str, method: str,
                  order: int, ehat: Tensor, status: Tensor, choice: Tensor, pred: Tensor,
                  llr: Tensor, iters_used: Tensor, relay_status: Tensor, leg: Tensor,
                  nsol: Tensor) -> None:
    from . import ops
    ops._relay_osd_impl(graph_of(graph_id), x.contiguous(), gammas.contiguous(), iters0, iters_leg,
                        stop_after, alpha, beta, soft, base, method, order, ehat, status, choice,
                        pred, llr, iters_used, relay_status, leg, nsol)


@relay_osd_out.register_fake
def _relay_osd_out_fake(graph_id, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft, base,
                        method, order, ehat, status, choice, pred, llr, iters_used, relay_status,
                        leg, nsol):
    return None


# ---------------------------------------------------------------------------------------
# min-sum BP with guided decimation
# ---------------------------------------------------------------------------------------
@torch.library.custom_op('gnnd::bpgd', mutates_args=(), device_types='cuda')
def bpgd(graph_id: int, x: Tensor, iters0: int, iters_round: int, rounds: int, per_round: int,
         pick: str, clamp: float, alpha: float, beta: float
         ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    real = tuple(torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device) for _ in range(3))
    ints = tuple(torch.empty(B, dtype=torch.int32, device=x.device) for _ in range(3))
    ops._bpgd_impl(g, x, iters0, iters_round, rounds, per_round, pick, clamp, alpha, beta, *real,
                   *ints)
    return real + ints


@bpgd.register_fake
def _bpgd_fake(graph_id, x, iters0, iters_round, rounds, per_round, pick, clamp, alpha, beta):
    V, C, N, E = _DIMS[graph_id]
    B = x.numel() // N
    return (tuple(x.new_empty(B * V, 1) for _ in range(3))
            + tuple(x.new_empty(B, dtype=torch.int32) for _ in range(3)))


@torch.library.custom_op('gnnd::bpgd_out',
                         mutates_args=('ehat', 'llr', 'pred', 'iters_used', 'status', 'ndec'),
                         device_types='cuda')
def bpgd_out(graph_id: int, x: Tensor, iters0: int, iters_round: int, rounds: int, per_round: int,
             pick: str, clamp: float, alpha: float, beta: float, ehat: Tensor, llr: Tensor,
             pred: Tensor, iters_used: Tensor, status: Tensor, ndec: Tensor) -> None:
    from . import ops
    ops._bpgd_impl(graph_of(graph_id), x.contiguous(), iters0, iters_round, rounds, per_round, pick,
                   clamp, alpha, beta, ehat, llr, pred, iters_used, status, ndec)


@bpgd_out.register_fake
def _bpgd_out_fake(graph_id, x, iters0, iters_round, rounds, per_round, pick, clamp, alpha, beta,
                   ehat, llr, pred, iters_used, status, ndec):
    return None


# ---------------------------------------------------------------------------------------
# union-find decoding of a matchable code
# ---------------------------------------------------------------------------------------
@torch.library.custom_op('gnnd::uf', mutates_args=(), device_types='cuda')
def uf(graph_id: int, x: Tensor, gate: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    # zeros, not empty: the rows a gate skips are not written
    ehat = torch.zeros(B * g.V, 1, dtype=x.dtype, device=x.device)
    ints = tuple(torch.zeros(B, dtype=torch.int32, device=x.device) for _ in range(3))
    ops._uf_impl(g, x, None if gate is None else gate.contiguous(), ehat, *ints)
    return (ehat,) + ints


@uf.register_fake
def _uf_fake(graph_id, x, gate):
    V, C, N, E = _DIMS[graph_id]
    B = x.numel() // N
    return (x.new_empty(B * V, 1),) + tuple(x.new_empty(B, dtype=torch.int32) for _ in range(3))


@torch.library.custom_op('gnnd::uf_out', mutates_args=('ehat', 'rounds', 'status', 'nfull'),
                         device_types='cuda')
def uf_out(graph_id: int, x: Tensor, gate: Optional[Tensor], ehat: Tensor, rounds: Tensor,
           status: Tensor, nfull: Tensor) -> None:
    from . import ops
    ops._uf_impl(graph_of(graph_id), x.contiguous(), None if gate is None else gate.contiguous(),
                 ehat, rounds, status, nfull)


@uf_out.register_fake
def _uf_out_fake(graph_id, x, gate, ehat, rounds, status, nfull):
    return None


# ---------------------------------------------------------------------------------------
# weighted union-find and the one-call belief-find decoder
# ---------------------------------------------------------------------------------------
def _opt(t):
    return None if t is None else t.contiguous()


@torch.library.custom_op('gnnd::ufw', mutates_args=(), device_types='cuda')
def ufw(graph_id: int, x: Tensor, llr: Optional[Tensor], scale: float, wmax: int,
        gate: Optional[Tensor], passthrough: bool
        ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    # zeros, not empty: the rows a gate skips are not written
    ehat = torch.zeros(B * g.V, 1, dtype=x.dtype, device=x.device)
    ints = tuple(torch.zeros(B, dtype=torch.int32, device=x.device) for _ in range(4))
    ops._ufw_impl(g, x, _opt(llr), scale, wmax, _opt(gate), passthrough, ehat, *ints)
    return (ehat,) + ints


@ufw.register_fake
def _ufw_fake(graph_id, x, llr, scale, wmax, gate, passthrough):
    V, C, N, E = _DIMS[graph_id]
    B = x.numel() // N
    return (x.new_empty(B * V, 1),) + tuple(x.new_empty(B, dtype=torch.int32) for _ in range(4))


@torch.library.custom_op('gnnd::ufw_out',
                         mutates_args=('ehat', 'rounds', 'status', 'nfull', 'events'),
                         device_types='cuda')
def ufw_out(graph_id: int, x: Tensor, llr: Optional[Tensor], scale: float, wmax: int,
            gate: Optional[Tensor], passthrough: bool, ehat: Tensor, rounds: Tensor,
            status: Tensor, nfull: Tensor, events: Tensor) -> None:
    from . import ops
    ops._ufw_impl(graph_of(graph_id), x.contiguous(), _opt(llr), scale, wmax, _opt(gate),
                  passthrough, ehat, rounds, status, nfull, events)


@ufw_out.register_fake
def _ufw_out_fake(graph_id, x, llr, scale, wmax, gate, passthrough, ehat, rounds, status, nfull,
                  events):
    return None


@torch.library.custom_op('gnnd::belief_find', mutates_args=(), device_types='cuda')
def belief_find(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float, early_stop: bool,
                scale: float, wmax: int
                ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    ehat, pred, llr = (torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device) for _ in range(3))
    status, iters_used, bp_status, rounds, nfull, events = (
        torch.empty(B, dtype=torch.int32, device=x.device) for _ in range(6))
    ops._belief_find_impl(g, x, iters, alpha, beta, early_stop, scale, wmax, ehat, status,
                          iters_used, bp_status, pred, llr, rounds, nfull, events)
    return ehat, status, iters_used, bp_status, pred, llr, rounds, nfull, events


@belief_find.register_fake
def _belief_find_fake(graph_id, x, iters, alpha, beta, early_stop, scale, wmax):
    V, C, N, E = _DIMS[graph_id]
    B = x.numel() // N

    def ints():
        return x.new_empty(B, dtype=torch.int32)
    return (x.new_empty(B * V, 1), ints(), ints(), ints(), x.new_empty(B * V, 1),
            x.new_empty(B * V, 1), ints(), ints(), ints())


@torch.library.custom_op('gnnd::belief_find_out',
                         mutates_args=('ehat', 'status', 'iters_used', 'bp_status', 'pred', 'llr',
                                       'rounds', 'nfull', 'events'), device_types='cuda')
def belief_find_out(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float,
                    early_stop: bool, scale: float, wmax: int, ehat: Tensor, status: Tensor,
                    iters_used: Tensor, bp_status: Tensor, pred: Tensor, llr: Tensor,
                    rounds: Tensor, nfull: Tensor, events: Tensor) -> None:
    from . import ops
    ops._belief_find_impl(graph_of(graph_id), x.contiguous(), iters, alpha, beta, early_stop,
                          scale, wmax, ehat, status, iters_used, bp_status, pred, llr, rounds,
                          nfull, events)


@belief_find_out.register_fake
def _belief_find_out_fake(graph_id, x, iters, alpha, beta, early_stop, scale, wmax, ehat, status,
                          iters_used, bp_status, pred, llr, rounds, nfull, events):
    return None


# ---------------------------------------------------------------------------------------
# localized-statistics decoding and the one-call BP+LSD decoder
# ---------------------------------------------------------------------------------------
def _lsd_new(pred, V):
    pred = pred.contiguous()
    B = pred.numel() // V
    return pred, (torch.empty_like(pred),) + tuple(
        torch.empty(B, dtype=torch.int32, device=pred.device) for _ in range(4))


def _lsd_fake_outs(graph_id, pred):
    B = pred.numel() // _DIMS[graph_id][0]
    return (torch.empty_like(pred, memory_format=torch.contiguous_format),) + tuple(
        pred.new_empty(B, dtype=torch.int32) for _ in range(4))


@torch.library.custom_op('gnnd::lsd', mutates_args=(), device_types='cuda')
def lsd(graph_id: int, x: Tensor, pred: Tensor, base: str, bits_per_step: int
        ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    pred, out = _lsd_new(pred, g.V)
    ops._lsd_impl(g, x.contiguous(), pred, base, bits_per_step, *out)
    return out


@lsd.register_fake
def _lsd_fake(graph_id, x, pred, base, bits_per_step):
    return _lsd_fake_outs(graph_id, pred)


@torch.library.custom_op('gnnd::lsd_out',
                         mutates_args=('ehat', 'status', 'rounds', 'nclus', 'ncols'),
                         device_types='cuda')
def lsd_out(graph_id: int, x: Tensor, pred: Tensor, base: str, bits_per_step: int, ehat: Tensor,
            status: Tensor, rounds: Tensor, nclus: Tensor, ncols: Tensor) -> None:
    from . import ops
    ops._lsd_impl(graph_of(graph_id), x.contiguous(), pred.contiguous(), base, bits_per_step, ehat,
                  status, rounds, nclus, ncols)


@lsd_out.register_fake
def _lsd_out_fake(graph_id, x, pred, base, bits_per_step, ehat, status, rounds, nclus, ncols):
    return None


@torch.library.custom_op('gnnd::lsd_gated', mutates_args=(), device_types='cuda')
def lsd_gated(graph_id: int, x: Tensor, pred: Tensor, gate: Tensor, base: str, bits_per_step: int,
              llr: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    pred, out = _lsd_new(pred, g.V)
    ops._lsd_gated_impl(g, x.contiguous(), pred, gate.contiguous(), base, bits_per_step,
                        None if llr is None else llr.contiguous(), *out)
    return out


@lsd_gated.register_fake
def _lsd_gated_fake(graph_id, x, pred, gate, base, bits_per_step, llr):
    return _lsd_fake_outs(graph_id, pred)


@torch.library.custom_op('gnnd::lsd_gated_out',
                         mutates_args=('ehat', 'status', 'rounds', 'nclus', 'ncols'),
                         device_types='cuda')
def lsd_gated_out(graph_id: int, x: Tensor, pred: Tensor, gate: Tensor, base: str,
                  bits_per_step: int, llr: Optional[Tensor], ehat: Tensor, status: Tensor,
                  rounds: Tensor, nclus: Tensor, ncols: Tensor) -> None:
    from . import ops
    ops._lsd_gated_impl(graph_of(graph_id), x.contiguous(), pred.contiguous(), gate.contiguous(),
                        base, bits_per_step, None if llr is None else llr.contiguous(), ehat,
                        status, rounds, nclus, ncols)


@lsd_gated_out.register_fake
def _lsd_gated_out_fake(graph_id, x, pred, gate, base, bits_per_step, llr, ehat, status, rounds,
                        nclus, ncols):
    return None


@torch.library.custom_op('gnnd::bplsd', mutates_args=(), device_types='cuda')
def bplsd(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float, early_stop: bool,
          base: str, bits_per_step: int
          ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    from . import ops
    g = graph_of(graph_id)
    x = x.contiguous()
    B = x.numel() // g.N
    ehat, pred, llr = (torch.empty(B * g.V, 1, dtype=x.dtype, device=x.device) for _ in range(3))
    status, rounds, nclus, ncols, iters_used, bp_status = (
        torch.empty(B, dtype=torch.int32, device=x.device) for _ in range(6))
    ops._bplsd_impl(g, x, iters, alpha, beta, early_stop, base, bits_per_step, ehat, status, rounds,
                    nclus, ncols, iters_used, bp_status, pred, llr)
    return ehat, status, rounds, nclus, ncols, iters_used, bp_status, pred, llr


@bplsd.register_fake
def _bplsd_fake(graph_id, x, iters, alpha, beta, early_stop, base, bits_per_step):
    V, C, N, E = _DIMS[graph_id]
    B = x.numel() // N

    def ints():
        return x.new_empty(B, dtype=torch.int32)
    return (x.new_empty(B * V, 1), ints(), ints(), ints(), ints(), ints(), ints(),
            x.new_empty(B * V, 1), x.new_empty(B * V, 1))


@torch.library.custom_op('gnnd::bplsd_out',
                         mutates_args=('ehat', 'status', 'rounds', 'nclus', 'ncols', 'iters_used',
                                       'bp_status', 'pred', 'llr'), device_types='cuda')
def bplsd_out(graph_id: int, x: Tensor, iters: int, alpha: float, beta: float, early_stop: bool,
              base: str, bits_per_step: int, ehat: Tensor, status: Tensor, rounds: Tensor,
              nclus: Tensor, ncols: Tensor, iters_used: Tensor, bp_status: Tensor, pred: Tensor,
              llr: Tensor) -> None:
    from . import ops
    ops._bplsd_impl(graph_of(graph_id), x.contiguous(), iters, alpha, beta, early_stop, base,
                    bits_per_step, ehat, status, rounds, nclus, ncols, iters_used, bp_status, pred,
                    llr)


@bplsd_out.register_fake
def _bplsd_out_fake(graph_id, x, iters, alpha, beta, early_stop, base, bits_per_step, ehat, status,
                    rounds, nclus, ncols, iters_used, bp_status, pred, llr):
    return None
