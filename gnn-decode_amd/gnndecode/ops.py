"""Tensor-level entry points over the C ABI (torch tensors only as device-memory plumbing).

Every function here launches HIP kernels from libgnnd.so on the current HIP stream and
never synchronises the host.  Inputs must already be on the GPU: there is no CPU path.
"""
import ctypes

import torch

from . import _lib
from .graph import TannerGraph, current_stream, dtype_code

MODELS = ('v24', 'qgnni', 'qbp', 'cgnni', 'cbp', 'nbp', 'v10', 'v30', 'v22')
WEIGHTED_BP = ('nbp', 'v10', 'v22')      # per-edge weight tables: count depends on the graph and T


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('gnndecode runs on the GPU only (HIP/gfx950); got a CPU tensor')


def propagate_width(variant, flow):
    return _lib.get().gnnd_propagate_width(_lib.VARIANT[variant], _lib.FLOW[flow])


def _tiled_batch(graph, edge_index, nE, dim_size, extra, aggr, chk_shift):
    """Batch size if edge_index is `graph` tiled over codewords, else None."""
    if graph is None or aggr == 'mean':
        return None
    shift = graph.V if chk_shift is None else chk_shift
    if (dim_size == (nE // graph.E) * graph.N and (extra is None or extra.size(0) == dim_size)
            and graph.is_tiled(edge_index, shift)):
        return nE // graph.E
    return None


def _propagate_fwd(variant, flow, aggr, edge_index, msg, extra, dim_size, B):
    nE = msg.size(0)
    F = propagate_width(variant, flow)
    out = torch.empty(nE, F, dtype=msg.dtype, device=msg.device)
    v, f, a = _lib.VARIANT[variant], _lib.FLOW[flow], _lib.AGGR[aggr]
    dt = dtype_code(msg.dtype)
    stream = current_stream(msg.device)
    if B is not None:
        _lib.call('gnnd_propagate_tiled', B[0].handle, v, f, a, dt, _ptr(msg), _ptr(extra),
                  _ptr(out), B[1], stream)
        return out
    ei = edge_index if edge_index.stride(1) == 1 else edge_index.contiguous()
    ws_bytes = ctypes.c_int64()
    _lib.call('gnnd_propagate_generic_workspace', v, f, a, dt, nE, dim_size, ctypes.byref(ws_bytes))
    ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=msg.device)
    _lib.call('gnnd_propagate_generic', v, f, a, dt, _ptr(ei), ei.stride(0), nE, _ptr(msg),
              _ptr(extra), dim_size, _ptr(out), _ptr(ws), ws_bytes.value, stream)
    return out


def _propagate_bwd(variant, flow, aggr, edge_index, msg, extra, grad_out, dim_size, B):
    grad_out = grad_out.contiguous()
    gmsg = torch.empty_like(msg)
    v, f, a = _lib.VARIANT[variant], _lib.FLOW[flow], _lib.AGGR[aggr]
    dt = dtype_code(msg.dtype)
    stream = current_stream(msg.device)
    if B is not None:
        _lib.call('gnnd_propagate_tiled_bwd', B[0].handle, v, f, a, dt, _ptr(msg), _ptr(extra),
                  _ptr(grad_out), _ptr(gmsg), B[1], stream)
        return gmsg
    ei = edge_index if edge_index.stride(1) == 1 else edge_index.contiguous()
    nb = ctypes.c_int64()
    _lib.call('gnnd_propagate_generic_bwd_workspace', v, f, a, dt, msg.size(0), dim_size,
              ctypes.byref(nb))
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=msg.device)
    _lib.call('gnnd_propagate_generic_bwd', v, f, a, dt, _ptr(ei), ei.stride(0), msg.size(0),
              _ptr(msg), _ptr(extra), _ptr(grad_out), dim_size, _ptr(gmsg), _ptr(ws),
              nb.value, stream)
    return gmsg


def _propagate_impl(variant, flow, aggr, edge_index, msg, extra, dim_size, graph, chk_shift):
    """gnnd::propagate implementation (gnndecode.library): tiled kernel when `graph` matches
    the batched edge_index, else the generic kernels."""
    b = _tiled_batch(graph, edge_index, msg.size(0), dim_size, extra, aggr, chk_shift)
    return _propagate_fwd(variant, flow, aggr, edge_index, msg, extra, dim_size,
                          (graph, b) if b is not None else None)


def _propagate_bwd_impl(variant, flow, aggr, edge_index, msg, extra, grad_out, dim_size, graph,
                        chk_shift):
    b = _tiled_batch(graph, edge_index, msg.size(0), dim_size, extra, aggr, chk_shift)
    return _propagate_bwd(variant, flow, aggr, edge_index, msg, extra, grad_out, dim_size,
                          (graph, b) if b is not None else None)


def propagate(variant, flow, aggr, edge_index, msg, extra, dim_size, graph=None, chk_shift=None):
    """One reference `propagate` body on the device (torch op gnnd::propagate).

    msg [nE, 1] per-edge message, extra [dim_size, 1] node tensor (or None for CGNNI's
    `post=None`), edge_index int64 [2, nE].  Uses the tiled LDS kernel when `graph` matches
    the batched edge_index, otherwise the generic (atomic) kernels.  Differentiable w.r.t.
    `msg` (aggr 'add') through HIP backward kernels (gnnd::propagate_bwd).
    Returns [nE, F] with F = propagate_width(variant, flow).
    """
    _require_gpu(edge_index, msg, extra)
    if msg.dim() == 1:
        msg = msg.unsqueeze(1)
    if msg.size(-1) != 1:
        raise ValueError('per-edge message must have one feature column (reference models)')
    msg = msg.contiguous()
    dtype_code(msg.dtype)
    if extra is not None:
        if extra.dim() == 1:
            extra = extra.unsqueeze(1)
        extra = extra.detach().to(msg.dtype).contiguous()
    nE = msg.size(0)
    if edge_index.size(1) != nE:
        raise ValueError('edge_index and message disagree on the number of edges')
    if extra is None and variant != 'cgnni':
        raise ValueError(f'{variant}: propagate needs `extra`')
    if msg.requires_grad and torch.is_grad_enabled() and aggr != 'add':
        raise NotImplementedError(f'no backward for aggr={aggr!r}')
    if torch.compiler.is_compiling():
        # traced (torch.compile / FX): the registered op gnnd::propagate (gnndecode.library)
        return torch.ops.gnnd.propagate(variant, flow, aggr, edge_index, msg, extra,
                                        int(dim_size), graph.gid if graph is not None else -1,
                                        -1 if chk_shift is None else int(chk_shift))
    # eager: the same implementation without the dispatcher round trip
    if msg.requires_grad and torch.is_grad_enabled():
        return _PropagateFn.apply(msg, variant, flow, aggr, edge_index, extra, int(dim_size),
                                  graph, chk_shift)
    return _propagate_impl(variant, flow, aggr, edge_index, msg, extra, dim_size, graph, chk_shift)


class _PropagateFn(torch.autograd.Function):
    """Eager autograd of propagate (the traced path uses gnnd::propagate's registered
    autograd): HIP backward w.r.t. the per-edge message, extra is data."""

    @staticmethod
    def forward(ctx, msg, variant, flow, aggr, edge_index, extra, dim_size, graph, chk_shift):
        ctx.save_for_backward(msg, edge_index, extra)
        ctx.args = (variant, flow, aggr, dim_size, graph, chk_shift)
        return _propagate_impl(variant, flow, aggr, edge_index, msg, extra, dim_size, graph,
                               chk_shift)

    @staticmethod
    def backward(ctx, grad_out):
        msg, edge_index, extra = ctx.saved_tensors
        variant, flow, aggr, dim_size, graph, chk_shift = ctx.args
        gmsg = _propagate_bwd_impl(variant, flow, aggr, edge_index, msg, extra,
                                   grad_out.contiguous(), dim_size, graph, chk_shift)
        return gmsg, None, None, None, None, None, None, None, None


def weights_count(model, graph=None, iters=None):
    """Packed weight count of a fused decoder (gnnd.h); the weighted-BP models need the
    graph and the iteration count."""
    n = ctypes.c_int64()
    if model in WEIGHTED_BP:
        if graph is None or iters is None:
            raise ValueError(f'{model}: the weight count depends on the graph and T')
        _lib.call('gnnd_decode_weights_count', graph.handle, _lib.VARIANT[model], int(iters),
                  ctypes.byref(n))
    else:
        _lib.call('gnnd_weights_count', _lib.VARIANT[model], ctypes.byref(n))
    return n.value


def prepared_count(model, dtype, graph=None, iters=None, priors=0):
    """Elements of the kernel-layout weights (gnnd_prepared_weights_count[_priors]): the packed
    count, except decoder_v2_4, whose prepared weights carry the check-MLP table and the
    channel-prior section (fp64: `priors` tables of the variable-side MLP)."""
    if model in WEIGHTED_BP:
        return weights_count(model, graph, iters)
    n = ctypes.c_int64()
    _lib.call('gnnd_prepared_weights_count_priors', _lib.VARIANT[model],
              dtype_code(torch.float32 if dtype == torch.bfloat16 else dtype), int(priors),
              ctypes.byref(n))
    return n.value


def prepare_weights(model, flat, priors=None):
    """Kernel-layout copy of a packed weight vector (gnnd_prepare_weights).  The weighted-BP
    tables are used as packed.  `priors` (fp64 decoder_v2_4): the channel-prior LLRs x_v the
    inputs will carry (e.g. channel_priors(graph, x)); the prepared weights then hold the
    variable-side MLP tabulated per prior (gnnd_prepare_weights_priors)."""
    _require_gpu(flat)
    flat = flat.contiguous()
    if model in WEIGHTED_BP:
        return flat
    n = weights_count(model)
    if n == 0:
        return None
    if flat.numel() != n:
        raise ValueError(f'{model}: expected {n} packed weights, got {flat.numel()}')
    pv = [float(v) for v in (priors if priors is not None else [])]
    out = torch.empty(prepared_count(model, flat.dtype, priors=len(pv)), dtype=flat.dtype,
                      device=flat.device)
    arr = (ctypes.c_double * max(len(pv), 1))(*pv)
    _lib.call('gnnd_prepare_weights_priors', _lib.VARIANT[model], dtype_code(flat.dtype), _ptr(flat),
              _ptr(out), arr, len(pv), current_stream(flat.device))
    return out


def channel_priors(graph, x, limit=64):
    """The distinct variable-node inputs x_v of a batch x [B*N] (the channel-prior LLRs of the
    reference's gen_syn inputs: one per codeword, from a short p list) -- the keys for
    prepare_weights(priors=...).  One device-to-host copy (setup, not the decode path); raises
    ValueError when there are more than `limit` (<= 64) distinct values."""
    xv = x.reshape(-1, graph.N)[:, :graph.V]
    u = torch.unique(xv).cpu().tolist()
    if len(u) > limit:
        raise ValueError(f'{len(u)} distinct priors (at most {limit} tables)')
    return u


MAX_PRIORS = 64      # channel-prior tables one prepared buffer holds (kVtMaxPriors)


def scan_channel_priors(graph, x, out=None):
    """channel_priors on the device (gnnd_v24_scan_priors): the distinct first variable inputs
    of the codewords of x [B*N] (fp64) -- the element the decoder keys a codeword's table on --
    ascending, as (priors fp64 [64], status int32 [2]) device tensors: priors[:count] the
    values, zeros after them, status = [count, 0]; more than 64 distinct values: zeros and
    status = [0, 1].  NaN inputs are skipped.  No host copy and no synchronisation; `out` = an
    earlier result's pair to write into."""
    _require_gpu(x)
    if x.dtype != torch.float64:
        raise TypeError(f'channel-prior tables are fp64 only, got {x.dtype}')
    x = x.contiguous()
    if x.numel() % graph.N:
        raise ValueError(f'x has {x.numel()} rows, not a multiple of N={graph.N}')
    if out is None:
        out = (torch.empty(MAX_PRIORS, dtype=torch.float64, device=x.device),
               torch.empty(2, dtype=torch.int32, device=x.device))
    priors, status = out
    if (priors.dtype != torch.float64 or priors.numel() != MAX_PRIORS or not priors.is_contiguous()
            or status.dtype != torch.int32 or status.numel() != 2 or not status.is_contiguous()):
        raise ValueError('out must be (contiguous fp64 [64], contiguous int32 [2])')
    _require_gpu(priors, status)
    _lib.call('gnnd_v24_scan_priors', graph.handle, dtype_code(x.dtype), _ptr(x),
              x.numel() // graph.N, _ptr(priors), _ptr(status), current_stream(x.device))
    return priors, status


def prepare_weights_auto(graph, flat, x, out=None, scratch=None):
    """prepare_weights('v24', flat, priors=channel_priors(graph, x)) with no host round trip:
    the batch's priors are found on the device (scan_channel_priors) and the tables built from
    that device list (gnnd_prepare_weights_priors_dev), all on the current stream.  The count is
    not known to the host, so the result has prepared_count('v24', float64, priors=64) elements
    (the tables of the priors found, then the readout table, the rest unused); with more than 64
    distinct priors it carries no tables.  `out` (that many fp64 elements) and `scratch` (a
    scan_channel_priors pair) are reused when given.  Returns the prepared tensor."""
    _require_gpu(flat, x)
    flat = flat.contiguous()
    if flat.dtype != torch.float64:
        raise TypeError(f'channel-prior tables are fp64 only, got {flat.dtype} weights')
    n = weights_count('v24')
    if flat.numel() != n:
        raise ValueError(f'v24: expected {n} packed weights, got {flat.numel()}')
    cap = prepared_count('v24', torch.float64, priors=MAX_PRIORS)
    if out is None:
        out = torch.empty(cap, dtype=torch.float64, device=flat.device)
    elif out.dtype != torch.float64 or out.numel() < cap or not out.is_contiguous():
        raise ValueError(f'out must be a contiguous fp64 tensor of at least {cap} elements')
    _require_gpu(out)
    priors, status = scan_channel_priors(graph, x, out=scratch)
    _lib.call('gnnd_prepare_weights_priors_dev', _lib.VARIANT['v24'], dtype_code(flat.dtype),
              _ptr(flat), _ptr(out), out.numel(), _ptr(priors), _ptr(status),
              current_stream(flat.device))
    return out


def v24_var_mlp_table(prepared_weights, u, xv=None):
    """gnnd_v24_var_mlp_table: decoder_v2_4's variable-side MLP through the channel-prior tables
    at fp64 points (u, x_v) -> (y, hit) with y = tanh(ggc1.mlp(u, x_v) / 2), the check step's
    pre-op of the MLP output that the tables hold; xv None: the readout MLP's table at u,
    y = mlp(u).  y is NaN where hit is False."""
    _require_gpu(prepared_weights, u)
    u = u.to(torch.float64).contiguous()
    if xv is not None:
        xv = xv.to(torch.float64).contiguous()
        if u.shape != xv.shape:
            raise ValueError('u and x need the same shape')
    y = torch.full_like(u, float('nan'))
    hit = torch.zeros(u.shape, dtype=torch.int32, device=u.device)
    _lib.call('gnnd_v24_var_mlp_table', _ptr(prepared_weights), _ptr(u),
              _ptr(xv) if xv is not None else None, _ptr(y), _ptr(hit), u.numel(),
              current_stream(u.device))
    return y, hit.bool()


def decode_out_rows(graph, model, B, iters=1):
    """Rows of gnnd_decode's output: B*V, 2*B*N for decoder_v3_0's two-output readout,
    iters*B*V for decoder_v2_2's per-iteration readout list."""
    if model == 'v30':
        return 2 * B * graph.N
    return iters * B * graph.V if model == 'v22' else B * graph.V


def decode(graph: TannerGraph, model, x, iters, prepared_weights=None, out=None):
    """Fused T-iteration decode: x [B*N(,1)] -> P(bit=1) [B*V, 1] (v30: [2*B*N, 1], the
    two readout tensors of quantum/decoder_v3_0.py:287-288 stacked; v22: [T*B*V, 1], the
    per-iteration readouts of quantum/decoder_v2_2.py:341-347 stacked).  Traced code
    (torch.compile / FX) gets the registered ops gnnd::decode / gnnd::decode_out."""
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.decode(graph.gid, model, x, int(iters), prepared_weights)
        torch.ops.gnnd.decode_out(graph.gid, model, x, int(iters), prepared_weights, out)
        return out
    _require_gpu(x, prepared_weights)
    x = x.contiguous()
    if x.numel() % graph.N:
        raise ValueError(f'x has {x.numel()} rows, not a multiple of N={graph.N}')
    B = x.numel() // graph.N
    wdt = torch.float32 if x.dtype == torch.bfloat16 else x.dtype   # bf16 storage, fp32 math
    nw = prepared_count(model, wdt, graph, iters)
    # (fp64 decoder_v2_4 prepared with channel-prior tables: more)
    if nw and (prepared_weights is None or prepared_weights.numel() < nw or
               (prepared_weights.numel() != nw and not (model == 'v24' and wdt == torch.float64))):
        raise ValueError(f'{model}: needs {nw} prepared weights (prepare_weights)')
    if prepared_weights is not None and prepared_weights.dtype != wdt:
        raise TypeError(f'{x.dtype} inputs need {wdt} prepared weights')
    rows = decode_out_rows(graph, model, B, int(iters))
    if out is None:
        out = torch.empty(rows, 1, dtype=x.dtype, device=x.device)
    elif out.numel() != rows or not out.is_contiguous() or out.dtype != x.dtype:
        raise ValueError(f'out must be a contiguous {x.dtype} tensor of {rows} values')
    _decode_impl(graph, model, x, iters, prepared_weights, out)
    return out


def _decode_impl(graph, model, x, iters, prepared_weights, out):
    """gnnd::decode / gnnd::decode_out implementation (gnndecode.library)."""
    _lib.call('gnnd_decode', graph.handle, _lib.VARIANT[model], dtype_code(x.dtype),
              _ptr(prepared_weights), _ptr(x), _ptr(out), x.numel() // graph.N, int(iters),
              current_stream(x.device))


def decode_plan(graph, model, dtype):
    """{'cw', 'lds', 'kernel', 'items_per_lane'} of the fused decoder's launch plan."""
    plan = (ctypes.c_int32 * 5)()
    _lib.call('gnnd_decode_plan', graph.handle, _lib.VARIANT[model], dtype_code(dtype), plan)
    return {'cw': plan[0], 'lds': plan[1],
            'kernel': 'decode_resident_kernel' if plan[2] else 'decode_kernel',
            'items_per_lane': plan[3], 'var_group': plan[4]}


def decode_tile(graph, model, dtype):
    cw, lds = ctypes.c_int32(), ctypes.c_int32()
    _lib.call('gnnd_decode_tile', graph.handle, _lib.VARIANT[model], dtype_code(dtype),
              ctypes.byref(cw), ctypes.byref(lds))
    return cw.value, lds.value


# ---------------------------------------------------------------------------------------
# fused training step (decoder_v2_4): forward with tape + one-launch reverse pass
# ---------------------------------------------------------------------------------------
def train_forward(graph, model, x, prepared_weights, iters):
    """gnnd_train_fwd: the fused decode plus the training tape (models v24, v30; nbp, v22 fp64).
    Returns (out, tape)."""
    _require_gpu(x, prepared_weights)
    x = x.contiguous()
    B = x.numel() // graph.N
    dt = dtype_code(x.dtype)
    # (decoder_v2_4 reads its prepared layout -- fp64: with the check-MLP table; the other
    # models' training forwards read the plain weights at its head)
    nw = (prepared_count(model, x.dtype, graph, iters) if model == 'v24'
          else weights_count(model, graph, iters))
    if nw and (prepared_weights is None or prepared_weights.numel() < nw):
        raise ValueError(f'{model}: needs {nw} prepared weights (prepare_weights)')
    nb = ctypes.c_int64()
    _lib.call('gnnd_train_tape_bytes', graph.handle, _lib.VARIANT[model], dt, B, int(iters),
              ctypes.byref(nb))
    tape = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=x.device)
    # v30: the two readout tensors [2][B*N]; v22: every layer's readout [T][B*V] (gnnd_decode's
    # layouts)
    nout = 2 * B * graph.N if model == 'v30' else iters * B * graph.V if model == 'v22' else B * graph.V
    out = torch.empty(nout, 1, dtype=x.dtype, device=x.device)
    _lib.call('gnnd_train_fwd', graph.handle, _lib.VARIANT[model], dt, _ptr(prepared_weights),
              _ptr(x), _ptr(out), _ptr(tape), B, int(iters), current_stream(x.device))
    return out, tape


def train_forward_loss(graph, model, x, prepared_weights, iters, y, logical_mask, n_logical,
                       logical_only):
    """gnnd_train_fwd_loss: train_forward plus decoder_v2_4's syndrome loss in the forward's
    epilogue.  Returns (out, tape, d loss / d out, per-codeword-and-component losses), or None
    when the plan does not take it (fp32 V24 unit-split small batches only): then
    train_backward_loss_partial computes the same loss in the reverse pass."""
    _require_gpu(x, prepared_weights)
    x = x.contiguous()
    B = x.numel() // graph.N
    dt = dtype_code(x.dtype)
    nb = ctypes.c_int64()
    _lib.call('gnnd_train_tape_bytes', graph.handle, _lib.VARIANT[model], dt, B, int(iters),
              ctypes.byref(nb))
    nl = ctypes.c_int64()
    _lib.call('gnnd_train_loss_count', graph.handle, B, ctypes.byref(nl))
    tape = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=x.device)
    out = torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device)
    gout = torch.empty_like(out)
    loss_b = torch.empty(max(nl.value, 1), dtype=x.dtype, device=x.device)[:nl.value]
    y = y.to(x.dtype).contiguous()
    ok = _lib.call_or_unsupported(
        'gnnd_train_fwd_loss', graph.handle, _lib.VARIANT[model], dt, _ptr(prepared_weights),
        _ptr(x), _ptr(out), _ptr(tape), _ptr(y), _ptr(logical_mask), int(n_logical),
        int(bool(logical_only)), _ptr(gout), _ptr(loss_b), B, int(iters), current_stream(x.device))
    return (out, tape, gout, loss_b) if ok else None


def train_backward(graph, model, plain_weights, x, out, grad_out, tape, iters):
    """gnnd_train_bwd: d loss / d (plain packed weights) from d loss / d out."""
    B = x.numel() // graph.N
    dt = dtype_code(x.dtype)
    nb = ctypes.c_int64()
    _lib.call('gnnd_train_workspace_bytes', graph.handle, _lib.VARIANT[model], dt, B, int(iters),
              ctypes.byref(nb))
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=x.device)
    gw = torch.empty_like(plain_weights)
    grad_out = grad_out.contiguous()
    _lib.call('gnnd_train_bwd', graph.handle, _lib.VARIANT[model], dt, _ptr(plain_weights), _ptr(x),
              _ptr(out), _ptr(grad_out), _ptr(tape), _ptr(gw), _ptr(ws), nb.value, B, int(iters),
              current_stream(x.device))
    return gw


def train_backward_partial(graph, model, plain_weights, x, out, grad_out, tape, iters, ws=None):
    """gnnd_train_bwd_partial: the reverse pass leaving its per-workgroup gradient rows in a
    workspace.  Returns (workspace, rows); reduce with train_update."""
    B = x.numel() // graph.N
    dt = dtype_code(x.dtype)
    nr = ctypes.c_int64()
    _lib.call('gnnd_train_bwd_rows', graph.handle, _lib.VARIANT[model], dt, B, ctypes.byref(nr))
    nb = ctypes.c_int64()
    _lib.call('gnnd_train_workspace_bytes', graph.handle, _lib.VARIANT[model], dt, B, int(iters),
              ctypes.byref(nb))
    if ws is None or ws.numel() < nb.value:
        ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=x.device)
    grad_out = grad_out.contiguous()
    _lib.call('gnnd_train_bwd_partial', graph.handle, _lib.VARIANT[model], dt, _ptr(plain_weights),
              _ptr(x), _ptr(out), _ptr(grad_out), _ptr(tape), _ptr(ws), nb.value, B, int(iters),
              current_stream(x.device))
    return ws, int(nr.value)


def train_backward_loss_partial(graph, model, plain_weights, x, out, y, logical_mask, n_logical,
                                logical_only, tape, iters, ws=None):
    """gnnd_train_bwd_loss_partial: the reverse pass with the syndrome loss fused in (no
    d loss / d out tensor).  Returns (workspace, rows, per-codeword-and-component losses), or
    None when the graph's tables plus the loss arrays exceed the workgroup's LDS (nothing
    launched: use the syndrome-loss kernel and train_backward_partial instead)."""
    B = x.numel() // graph.N
    dt = dtype_code(x.dtype)
    nr = ctypes.c_int64()
    _lib.call('gnnd_train_bwd_rows', graph.handle, _lib.VARIANT[model], dt, B, ctypes.byref(nr))
    nb = ctypes.c_int64()
    _lib.call('gnnd_train_workspace_bytes', graph.handle, _lib.VARIANT[model], dt, B, int(iters),
              ctypes.byref(nb))
    nl = ctypes.c_int64()
    _lib.call('gnnd_train_loss_count', graph.handle, B, ctypes.byref(nl))
    if ws is None or ws.numel() < nb.value:
        ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=x.device)
    loss_b = torch.empty(max(nl.value, 1), dtype=x.dtype, device=x.device)[:nl.value]
    y = y.to(x.dtype).contiguous()
    ok = _lib.call_or_unsupported(
        'gnnd_train_bwd_loss_partial', graph.handle, _lib.VARIANT[model], dt,
        _ptr(plain_weights), _ptr(x), _ptr(out), _ptr(y), _ptr(logical_mask), int(n_logical),
        int(bool(logical_only)), _ptr(tape), _ptr(loss_b), _ptr(ws), nb.value, B, int(iters),
        current_stream(x.device))
    return (ws, int(nr.value), loss_b) if ok else None


def train_update(model, dtype, rows=None, n_rows=0, grad=None, loss_b=None, loss=None,
                 param=None, exp_avg=None, exp_avg_sq=None, step=None, sync=None, lr=3e-4,
                 betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, prepared=None, device=None):
    """gnnd_train_update: reduce the reverse pass's rows (and the per-codeword losses) and/or
    apply Adam + the kernel-layout weight copy, in one launch (see include/gnnd.h)."""
    dev = device or (param.device if param is not None else grad.device)
    _lib.call('gnnd_train_update', _lib.VARIANT[model], dtype_code(dtype), _ptr(rows), int(n_rows),
              _ptr(grad), _ptr(loss_b), 0 if loss_b is None else loss_b.numel(), _ptr(loss),
              _ptr(param), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(step), _ptr(sync), float(lr),
              float(betas[0]), float(betas[1]), float(eps), float(weight_decay), _ptr(prepared),
              current_stream(dev))


class FusedTrainFn(torch.autograd.Function):
    """out = decode(weights, x) with a one-launch HIP backward to the packed weights."""

    @staticmethod
    def forward(ctx, flat_w, x, graph, model, iters):
        w = flat_w.detach().to(x.dtype).contiguous()
        out, tape = train_forward(graph, model, x, prepare_weights(model, w), iters)
        ctx.save_for_backward(w, x, out, tape)
        ctx.args = (graph, model, iters, flat_w.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        w, x, out, tape = ctx.saved_tensors
        graph, model, iters, wdt = ctx.args
        gw = train_backward(graph, model, w, x, out, grad_out.to(x.dtype), tape, iters)
        return gw.to(wdt), None, None, None, None


# ---------------------------------------------------------------------------------------
# training objective: syndrome loss + gradient in one launch (gnnd_syndrome_loss)
# ---------------------------------------------------------------------------------------
def syndrome_loss(graph, logical_rows, logical_only, pred, y):
    """(per-codeword losses [B], d loss / d pred [B*V, 1]) of quantum/decoder_v2_4.py:297-317
    (logical_only: quantum/QGNNI.py:255-290).  logical_rows: int32 [n_l, V] on the device."""
    _require_gpu(pred, y)
    V = graph.V
    pred = pred.contiguous()
    y = y.to(pred.dtype).contiguous()
    B = pred.numel() // V
    if pred.numel() != B * V or y.numel() != pred.numel():
        raise ValueError(f'pred/y must hold B*V values (V = {V})')
    loss_b = torch.empty(B, dtype=pred.dtype, device=pred.device)
    dpred = torch.empty_like(pred)
    lg = logical_rows.contiguous()
    _lib.call('gnnd_syndrome_loss', graph.handle, _ptr(lg), int(lg.size(0)), int(bool(logical_only)),
              dtype_code(pred.dtype), _ptr(pred), _ptr(y), _ptr(loss_b), _ptr(dpred), B,
              current_stream(pred.device))
    return loss_b, dpred


def v24_check_mlp_table(graph, w, u):
    """decoder_v2_4's check-side MLP evaluated through the fp64 decoder's table
    (gnnd_v24_check_mlp_table): (y [n] fp64, valid) where valid says whether the decoder uses
    the table for these weights (y undefined when not).  w: packed fp64 V24 weights (1283,
    prepared here) or prepared ones; u: fp64 inputs within [-(max_dc - 1), max_dc - 1]."""
    _require_gpu(w, u)
    w = w.to(torch.float64).contiguous()
    if w.numel() == weights_count('v24'):
        w = prepare_weights('v24', w)
    u = u.to(torch.float64).contiguous().reshape(-1)
    y = torch.empty_like(u)
    ok = torch.zeros(1, dtype=torch.int32, device=u.device)
    _lib.call('gnnd_v24_check_mlp_table', graph.handle, _ptr(w), _ptr(u), _ptr(y), u.numel(),
              _ptr(ok), current_stream(u.device))
    return y, bool(ok.item())


def decision_errors(graph, logical_rows, pred, y):
    """(bit errors, frame errors, residual-syndrome failures, logical failures) of hard
    decisions pred > 0.5 against y, one HIP launch (gnnd_decision_errors); int64 tensor [4]
    on the device (no host sync).  logical_rows: int32 [n_l, V] or None (classical)."""
    _require_gpu(pred, y)
    V = graph.V
    pred = pred.contiguous()
    y = y.to(pred.dtype).contiguous()
    B = pred.numel() // V
    if pred.numel() != B * V or y.numel() != pred.numel():
        raise ValueError(f'pred/y must hold B*V values (V = {V})')
    counts = torch.empty(4, dtype=torch.int64, device=pred.device)
    if logical_rows is None:
        lg, nl = None, 0
    else:
        lg = logical_rows.to(device=pred.device, dtype=torch.int32).contiguous()
        nl = int(lg.size(0))
    _lib.call('gnnd_decision_errors', graph.handle, _ptr(lg), nl,
              dtype_code(pred.dtype), _ptr(pred), _ptr(y), _ptr(counts), B,
              current_stream(pred.device))
    return counts


# ---------------------------------------------------------------------------------------
# OSD-0 post-processing (gnnd_osd0): syndrome-satisfying estimates from soft outputs
# ---------------------------------------------------------------------------------------
def osd0(graph, x, pred, base='zero', out=None):
    """Order-0 ordered-statistics post-processing of a decoder's soft output, one HIP launch
    (gnnd_osd0): x [B*N(,1)] the decoder input (its check rows carry the syndrome), pred
    [B*V(,1)] P(bit = 1) -> (ehat, status).  ehat has pred's shape and dtype and holds exactly
    0.0 / 1.0: it satisfies the syndrome wherever status [B] (int32) is 0 and is the base vector
    where it is 1 (syndrome outside the column space of H^T).  base 'zero': solve from the zero
    vector with the columns ordered by pred (the usual quantum form); 'hard': solve for a
    correction of the hard decision pred > 0.5 with the least reliable columns first (the
    classical form).  No host sync; `out` = (ehat, status) tensors to write into."""
    if base not in _lib.OSD_BASE:
        raise ValueError(f"base must be 'zero' or 'hard', got {base!r}")
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.osd0(graph.gid, x, pred, base)
        torch.ops.gnnd.osd0_out(graph.gid, x, pred, base, out[0], out[1])
        return out
    _require_gpu(x, pred)
    if x.dtype != pred.dtype:
        raise TypeError(f'x ({x.dtype}) and pred ({pred.dtype}) must share a dtype')
    if pred.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'osd0 supports float32/float64, got {pred.dtype}')
    x = x.contiguous()
    pred = pred.contiguous()
    B = pred.numel() // graph.V
    if pred.numel() != B * graph.V or x.numel() != B * graph.N:
        raise ValueError(f'pred must hold B*V and x B*N values (V = {graph.V}, N = {graph.N})')
    if out is None:
        out = (torch.empty_like(pred), torch.empty(B, dtype=torch.int32, device=pred.device))
    ehat, status = out
    _require_gpu(ehat, status)
    if (ehat.dtype != pred.dtype or ehat.numel() != pred.numel() or not ehat.is_contiguous()
            or status.dtype != torch.int32 or status.numel() != B or not status.is_contiguous()):
        raise ValueError(f'out must be (contiguous {pred.dtype} [{B * graph.V}], contiguous int32 [{B}])')
    _osd0_impl(graph, x, pred, base, ehat, status)
    return ehat, status


def _osd0_impl(graph, x, pred, base, ehat, status):
    """gnnd::osd0 / gnnd::osd0_out implementation (gnndecode.library)."""
    _lib.call('gnnd_osd0', graph.handle, dtype_code(pred.dtype), _ptr(x), _ptr(pred),
              _lib.OSD_BASE[base], _ptr(ehat), _ptr(status), pred.numel() // graph.V,
              current_stream(pred.device))


def osd0_host(H, x, pred, base='zero'):
    """The host mirror of osd0 (gnnd_osd0_host): numpy in, numpy out, no device.  H [V, C],
    x [B*N], pred [B*V] float32 or float64 -> (ehat like pred, status int32 [B])."""
    import numpy as np
    from .graph import edge_list
    if base not in _lib.OSD_BASE:
        raise ValueError(f"base must be 'zero' or 'hard', got {base!r}")
    H = np.asarray(H)
    V, C = H.shape
    pred = np.ascontiguousarray(pred)
    if pred.dtype not in (np.float32, np.float64):
        raise TypeError(f'osd0_host supports float32/float64, got {pred.dtype}')
    x = np.ascontiguousarray(x, dtype=pred.dtype)
    B = pred.size // V
    if pred.size != B * V or x.size != B * (V + C):
        raise ValueError(f'pred must hold B*V and x B*N values (V = {V}, N = {V + C})')
    var, chk = edge_list(H)
    ehat = np.empty_like(pred)
    status = np.empty(B, np.int32)
    P64 = ctypes.POINTER(ctypes.c_int64)
    _lib.call('gnnd_osd0_host', var.ctypes.data_as(P64), chk.ctypes.data_as(P64), var.size, V, C,
              _lib.F32 if pred.dtype == np.float32 else _lib.F64, x.ctypes.data, pred.ctypes.data,
              _lib.OSD_BASE[base], ehat.ctypes.data, status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
              B)
    return ehat, status


# ---------------------------------------------------------------------------------------
# higher-order OSD post-processing (gnnd_osd): the lightest of the combination-sweep or
# exhaustive candidates on top of OSD-0
# ---------------------------------------------------------------------------------------
def _osd_check_method(base, method, order):
    if base not in _lib.OSD_BASE:
        raise ValueError(f"base must be 'zero' or 'hard', got {base!r}")
    if method not in _lib.OSD_METHOD:
        raise ValueError(f"method must be 'osd0', 'cs' or 'e', got {method!r}")
    limit = {'osd0': 2 ** 31 - 1, 'cs': 64, 'e': 12}[method]
    if not isinstance(order, int) or not 0 <= order <= limit:
        raise ValueError(f'order must be an integer in [0, {limit}] for method {method!r}, got {order!r}')


def osd(graph, x, pred, base='zero', method='cs', order=10, out=None):
    """Ordered-statistics post-processing of order > 0, one HIP launch (gnnd_osd): as osd0, then
    among a fixed list of further syndrome-satisfying candidates over the free (non-pivot)
    columns the one of least weight, ties to the lowest candidate index (include/gnnd.h).
    method 'osd0': the OSD-0 solution alone; 'cs' (combination sweep): every single free column,
    then the pairs of the first min(order, F) of them, order <= 64; 'e' (exhaustive): the
    2^min(order, F) subsets of the first free columns, order <= 12.  -> (ehat, status, choice):
    ehat and status as osd0, choice [B] int32 the chosen candidate's index (0: the OSD-0
    solution, and where status is 1).  No host sync; `out` = (ehat, status, choice) tensors to
    write into, or (ehat, status) to skip the choice (returned as None)."""
    _osd_check_method(base, method, order)
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.osd(graph.gid, x, pred, base, method, order)
        if len(out) != 3 or out[2] is None:
            raise ValueError('traced osd needs out = (ehat, status, choice)')
        torch.ops.gnnd.osd_out(graph.gid, x, pred, base, method, order, out[0], out[1], out[2])
        return out
    _require_gpu(x, pred)
    if x.dtype != pred.dtype:
        raise TypeError(f'x ({x.dtype}) and pred ({pred.dtype}) must share a dtype')
    if pred.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'osd supports float32/float64, got {pred.dtype}')
    x = x.contiguous()
    pred = pred.contiguous()
    B = pred.numel() // graph.V
    if pred.numel() != B * graph.V or x.numel() != B * graph.N:
        raise ValueError(f'pred must hold B*V and x B*N values (V = {graph.V}, N = {graph.N})')
    if out is None:
        out = (torch.empty_like(pred), torch.empty(B, dtype=torch.int32, device=pred.device),
               torch.empty(B, dtype=torch.int32, device=pred.device))
    if len(out) not in (2, 3):
        raise ValueError('out must be (ehat, status) or (ehat, status, choice)')
    ehat, status = out[0], out[1]
    choice = out[2] if len(out) == 3 else None
    _require_gpu(ehat, status)
    if (ehat.dtype != pred.dtype or ehat.numel() != pred.numel() or not ehat.is_contiguous()
            or status.dtype != torch.int32 or status.numel() != B or not status.is_contiguous()):
        raise ValueError(f'out must be (contiguous {pred.dtype} [{B * graph.V}], contiguous int32 [{B}], ...)')
    if choice is not None:
        _require_gpu(choice)
        if choice.dtype != torch.int32 or choice.numel() != B or not choice.is_contiguous():
            raise ValueError(f'choice must be contiguous int32 [{B}]')
    _osd_impl(graph, x, pred, base, method, order, ehat, status, choice)
    return ehat, status, choice


def _osd_impl(graph, x, pred, base, method, order, ehat, status, choice):
    """gnnd::osd / gnnd::osd_out implementation (gnndecode.library)."""
    _lib.call('gnnd_osd', graph.handle, dtype_code(pred.dtype), _ptr(x), _ptr(pred),
              _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order, _ptr(ehat), _ptr(status),
              None if choice is None else _ptr(choice), pred.numel() // graph.V,
              current_stream(pred.device))


def osd_host(H, x, pred, base='zero', method='cs', order=10):
    """The host mirror of osd (gnnd_osd_host): numpy in, numpy out, no device.  H [V, C], x [B*N],
    pred [B*V] float32 or float64 -> (ehat like pred, status int32 [B], choice int32 [B])."""
    import numpy as np
    from .graph import edge_list
    _osd_check_method(base, method, order)
    H = np.asarray(H)
    V, C = H.shape
    pred = np.ascontiguousarray(pred)
    if pred.dtype not in (np.float32, np.float64):
        raise TypeError(f'osd_host supports float32/float64, got {pred.dtype}')
    x = np.ascontiguousarray(x, dtype=pred.dtype)
    B = pred.size // V
    if pred.size != B * V or x.size != B * (V + C):
        raise ValueError(f'pred must hold B*V and x B*N values (V = {V}, N = {V + C})')
    var, chk = edge_list(H)
    ehat = np.empty_like(pred)
    status = np.empty(B, np.int32)
    choice = np.empty(B, np.int32)
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    _lib.call('gnnd_osd_host', var.ctypes.data_as(P64), chk.ctypes.data_as(P64), var.size, V, C,
              _lib.F32 if pred.dtype == np.float32 else _lib.F64, x.ctypes.data, pred.ctypes.data,
              _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order, ehat.ctypes.data,
              status.ctypes.data_as(P32), choice.ctypes.data_as(P32), B)
    return ehat, status, choice


# ---------------------------------------------------------------------------------------
# min-sum BP with the syndrome-converged early stop (gnnd_minsum)
# ---------------------------------------------------------------------------------------
def _minsum_check_params(iters, alpha, beta):
    if not isinstance(iters, int) or isinstance(iters, bool) or not 1 <= iters <= 2 ** 31 - 1:
        raise ValueError(f'iters must be an integer >= 1, got {iters!r}')
    alpha, beta = float(alpha), float(beta)
    if not 0.0 < alpha <= 1.0:
        raise ValueError(f'alpha must be in (0, 1], got {alpha!r}')
    if not 0.0 <= beta < float('inf'):
        raise ValueError(f'beta must be finite and >= 0, got {beta!r}')
    return alpha, beta


def _schedule_suffix(schedule):
    """'' for the flooding schedule, '_layered' for the layered one: the suffix of the C entry
    points and of the gnnd:: torch ops."""
    if schedule == 'flooding':
        return ''
    if schedule == 'layered':
        return '_layered'
    raise ValueError(f"schedule must be 'flooding' or 'layered', got {schedule!r}")


def minsum(graph, x, iters, alpha=0.75, beta=0.0, early_stop=True, out=None, schedule='flooding'):
    """Normalized / offset min-sum BP, one HIP launch (gnnd_minsum on the flooding schedule,
    gnnd_minsum_layered with schedule='layered': the checks visited layer by layer, each seeing
    the posteriors the layers before it just updated; both defined in include/gnnd.h): x [B*N(,1)] the decoder input (priors at the variable rows, the
    syndrome at the check rows as for osd0) -> (pred, llr, iters_used, status).  Check messages
    are max(alpha * min|q| - beta, 0) with the sign product; with early_stop a codeword stops at
    the first iteration whose hard decision satisfies its syndrome.  pred [B*V, 1] is
    P(bit = 1) = 1 / (1 + exp(llr)), the tensor osd and decision_errors take; llr [B*V, 1] the
    posterior LLRs of the last executed iteration; iters_used [B] int32 the iterations executed;
    status [B] int32 0 where that hard decision satisfies the syndrome, else 1.  llr, iters_used
    and status are bit-reproducible (the host mirror minsum_host gives the same bits).  No host
    sync; `out` = (pred, llr, iters_used, status) tensors to write into, each but pred may be
    None to skip it (returned as None)."""
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    early_stop = bool(early_stop)
    suffix = _schedule_suffix(schedule)
    if torch.compiler.is_compiling():
        if out is None:
            return getattr(torch.ops.gnnd, 'minsum' + suffix)(graph.gid, x, iters, alpha, beta,
                                                              early_stop)
        if len(out) != 4 or any(o is None for o in out):
            raise ValueError('traced minsum needs out = (pred, llr, iters_used, status)')
        getattr(torch.ops.gnnd, 'minsum' + suffix + '_out')(graph.gid, x, iters, alpha, beta,
                                                            early_stop, *out)
        return out
    _require_gpu(x)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'minsum supports float32/float64, got {x.dtype}')
    x = x.contiguous()
    B = x.numel() // graph.N
    if x.numel() != B * graph.N:
        raise ValueError(f'x must hold B*N values (N = {graph.N})')
    if out is None:
        out = (torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device),
               torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device),
               torch.empty(B, dtype=torch.int32, device=x.device),
               torch.empty(B, dtype=torch.int32, device=x.device))
    if len(out) != 4 or out[0] is None:
        raise ValueError('out must be (pred, llr, iters_used, status); only pred is required')
    _require_gpu(*out)
    for t in out[:2]:
        if t is not None and (t.dtype != x.dtype or t.numel() != B * graph.V
                              or not t.is_contiguous()):
            raise ValueError(f'pred / llr must be contiguous {x.dtype} [{B * graph.V}]')
    for t in out[2:]:
        if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError(f'iters_used / status must be contiguous int32 [{B}]')
    _minsum_impl(graph, x, iters, alpha, beta, early_stop, *out, schedule=schedule)
    return tuple(out)


def _minsum_impl(graph, x, iters, alpha, beta, early_stop, pred, llr, iters_used, status,
                 schedule='flooding'):
    """gnnd::minsum[_layered] / gnnd::minsum[_layered]_out implementation (gnndecode.library)."""
    _lib.call('gnnd_minsum' + _schedule_suffix(schedule), graph.handle, dtype_code(x.dtype), _ptr(x), alpha, beta, iters,
              int(early_stop), _ptr(pred), _ptr(llr), _ptr(iters_used), _ptr(status),
              x.numel() // graph.N, current_stream(x.device))


def minsum_host(H, x, iters, alpha=0.75, beta=0.0, early_stop=True, schedule='flooding'):
    """The host mirror of minsum (gnnd_minsum_host, gnnd_minsum_layered_host with
    schedule='layered'): numpy in, numpy out, no device.  H [V, C], x [B*N] float32 or float64
    -> (pred, llr like x's dtype [B*V], iters_used, status int32 [B])."""
    import numpy as np
    from .graph import edge_list
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    suffix = _schedule_suffix(schedule)
    H = np.asarray(H)
    V, C = H.shape
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError(f'minsum_host supports float32/float64, got {x.dtype}')
    B = x.size // (V + C)
    if x.size != B * (V + C):
        raise ValueError(f'x must hold B*N values (N = {V + C})')
    var, chk = edge_list(H)
    pred = np.empty(B * V, x.dtype)
    llr = np.empty(B * V, x.dtype)
    iters_used = np.empty(B, np.int32)
    status = np.empty(B, np.int32)
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    _lib.call(f'gnnd_minsum{suffix}_host', var.ctypes.data_as(P64), chk.ctypes.data_as(P64), var.size, V, C,
              _lib.F32 if x.dtype == np.float32 else _lib.F64, x.ctypes.data, alpha, beta, iters,
              int(bool(early_stop)), pred.ctypes.data, llr.ctypes.data,
              iters_used.ctypes.data_as(P32), status.ctypes.data_as(P32), B)
    return pred, llr, iters_used, status


def minsum_layered_plan(graph, dtype):
    """The layered kernel's plan for `dtype` (gnnd_minsum_layered_plan) -> dict(layers,
    largest_layer, lanes_per_codeword, codewords_per_workgroup)."""
    plan = (ctypes.c_int32 * 4)()
    _lib.call('gnnd_minsum_layered_plan', graph.handle, dtype_code(dtype), plan)
    return dict(zip(('layers', 'largest_layer', 'lanes_per_codeword', 'codewords_per_workgroup'),
                    (int(p) for p in plan)))


def layers_host(H):
    """The greedy layers of H [V, C] on the host (gnnd_graph_layers_host) -> layer_of_check
    int32 [C]."""
    import numpy as np
    V, C, var, chk, vp, cp = _host_graph(H)
    n = ctypes.c_int32()
    layer = np.empty(C, np.int32)
    _lib.call('gnnd_graph_layers_host', vp, cp, var.size, V, C, ctypes.byref(n),
              layer.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert C == 0 or int(layer.max()) + 1 == n.value
    return layer


# ---------------------------------------------------------------------------------------
# relay min-sum BP: memory-strength legs that keep the lightest solution (gnnd_relay)
# ---------------------------------------------------------------------------------------
def _relay_check_params(iters0, iters_leg, stop_after, alpha, beta, legs):
    if iters_leg is None:
        iters_leg = iters0
    for name, val in (('iters0', iters0), ('iters_leg', iters_leg), ('stop_after', stop_after)):
        if not isinstance(val, int) or isinstance(val, bool) or not 1 <= val <= 2 ** 31 - 1:
            raise ValueError(f'{name} must be an integer >= 1, got {val!r}')
    if legs < 1:
        raise ValueError('gammas must hold at least one leg')
    if iters0 + (legs - 1) * iters_leg > 2 ** 31 - 1:
        raise ValueError('iters0 + (legs - 1) * iters_leg must fit an int32')
    alpha, beta = _minsum_check_params(1, alpha, beta)
    return iters_leg, alpha, beta


def relay_gammas(V, legs, gamma0=0.125, center=0.21, width=0.9, seed=0, dtype=torch.float64,
                 device=None):
    """The usual relay memory strengths, [legs, V] in `dtype`: row 0 is `gamma0` on every variable,
    the later rows are numpy.random.default_rng(seed).uniform(center - width / 2, center + width /
    2, (legs - 1, V)) (disordered, partly negative), drawn in float64 and cast to `dtype`."""
    import numpy as np
    if not isinstance(legs, int) or isinstance(legs, bool) or legs < 1:
        raise ValueError(f'legs must be an integer >= 1, got {legs!r}')
    g = np.full((legs, V), float(gamma0), np.float64)
    g[1:] = np.random.default_rng(seed).uniform(center - width / 2, center + width / 2,
                                                (legs - 1, V))
    return torch.from_numpy(g).to(dtype=dtype, device=device)


def relay(graph, x, gammas, iters0, iters_leg=None, stop_after=1, alpha=0.75, beta=0.0, out=None):
    """Relay min-sum BP, one HIP launch (gnnd_relay, defined in include/gnnd.h): min-sum with the
    per-variable memory strengths gammas [legs, V] (relay_gammas makes the usual table), one row
    per leg; leg 0 runs at most iters0 iterations, every later leg iters_leg (default iters0), each
    from the posteriors of the leg before; a leg ends at its first hard decision that satisfies the
    syndrome, the call after stop_after such solutions, and the lightest solution is kept.
    x [B*N(,1)] as for minsum -> (ehat, llr, iters_used, status, leg, nsol): ehat [B*V, 1] exactly
    0.0 / 1.0 and llr [B*V, 1] of the kept solution (of the last iteration where there is none),
    iters_used [B] int32 all iterations executed, status [B] int32 0 where a solution was found
    (ehat then satisfies the syndrome), leg [B] int32 the leg of the kept solution or -1, nsol [B]
    int32 the solutions collected.  Every output is bit-reproducible (relay_host gives the same
    bits).  No host sync; `out` = the six tensors to write into, each but ehat may be None to skip
    it (returned as None)."""
    if gammas.dim() != 2 or gammas.shape[1] != graph.V:
        raise ValueError(f'gammas must be [legs, V] (V = {graph.V})')
    legs = gammas.shape[0]
    iters_leg, alpha, beta = _relay_check_params(iters0, iters_leg, stop_after, alpha, beta, legs)
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.relay(graph.gid, x, gammas, iters0, iters_leg, stop_after, alpha,
                                        beta)
        if len(out) != 6 or any(o is None for o in out):
            raise ValueError('traced relay needs out = (ehat, llr, iters_used, status, leg, nsol)')
        torch.ops.gnnd.relay_out(graph.gid, x, gammas, iters0, iters_leg, stop_after, alpha, beta,
                                 *out)
        return out
    _require_gpu(x, gammas)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'relay supports float32/float64, got {x.dtype}')
    if gammas.dtype != x.dtype:
        raise TypeError(f'gammas must have the dtype of x ({x.dtype}), got {gammas.dtype}')
    x = x.contiguous()
    gammas = gammas.contiguous()
    B = x.numel() // graph.N
    if x.numel() != B * graph.N:
        raise ValueError(f'x must hold B*N values (N = {graph.N})')
    if out is None:
        out = ((torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device),
                torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device))
               + tuple(torch.empty(B, dtype=torch.int32, device=x.device) for _ in range(4)))
    if len(out) != 6 or out[0] is None:
        raise ValueError('out must be (ehat, llr, iters_used, status, leg, nsol); only ehat is '
                         'required')
    _require_gpu(*out)
    for t in out[:2]:
        if t is not None and (t.dtype != x.dtype or t.numel() != B * graph.V
                              or not t.is_contiguous()):
            raise ValueError(f'ehat / llr must be contiguous {x.dtype} [{B * graph.V}]')
    for t in out[2:]:
        if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError(f'iters_used / status / leg / nsol must be contiguous int32 [{B}]')
    _relay_impl(graph, x, gammas, iters0, iters_leg, stop_after, alpha, beta, *out)
    return tuple(out)


def _relay_impl(graph, x, gammas, iters0, iters_leg, stop_after, alpha, beta, ehat, llr, iters_used,
                status, leg, nsol):
    """gnnd::relay / gnnd::relay_out implementation (gnndecode.library)."""
    _lib.call('gnnd_relay', graph.handle, dtype_code(x.dtype), _ptr(x), _ptr(gammas),
              gammas.shape[0], iters0, iters_leg, stop_after, alpha, beta, _ptr(ehat), _ptr(llr),
              _ptr(iters_used), _ptr(status), _ptr(leg), _ptr(nsol), x.numel() // graph.N,
              current_stream(x.device))


def relay_host(H, x, gammas, iters0, iters_leg=None, stop_after=1, alpha=0.75, beta=0.0):
    """The host mirror of relay (gnnd_relay_host): numpy in, numpy out, no device.  H [V, C],
    x [B*N] float32 or float64, gammas [legs, V] (cast to x's dtype) -> (ehat, llr like x's dtype
    [B*V], iters_used, status, leg, nsol int32 [B])."""
    import numpy as np
    from .graph import edge_list
    H = np.asarray(H)
    V, C = H.shape
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError(f'relay_host supports float32/float64, got {x.dtype}')
    gammas = np.ascontiguousarray(gammas, x.dtype)
    if gammas.ndim != 2 or gammas.shape[1] != V:
        raise ValueError(f'gammas must be [legs, V] (V = {V})')
    legs = gammas.shape[0]
    iters_leg, alpha, beta = _relay_check_params(iters0, iters_leg, stop_after, alpha, beta, legs)
    B = x.size // (V + C)
    if x.size != B * (V + C):
        raise ValueError(f'x must hold B*N values (N = {V + C})')
    var, chk = edge_list(H)
    ehat = np.empty(B * V, x.dtype)
    llr = np.empty(B * V, x.dtype)
    ints = [np.empty(B, np.int32) for _ in range(4)]
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    _lib.call('gnnd_relay_host', var.ctypes.data_as(P64), chk.ctypes.data_as(P64), var.size, V, C,
              _lib.F32 if x.dtype == np.float32 else _lib.F64, x.ctypes.data, gammas.ctypes.data,
              legs, iters0, iters_leg, stop_after, alpha, beta, ehat.ctypes.data, llr.ctypes.data,
              *(a.ctypes.data_as(P32) for a in ints), B)
    return (ehat, llr) + tuple(ints)


# ---------------------------------------------------------------------------------------
# relay with a soft output (gnnd_relay_soft) and the one-call relay+OSD decoder (gnnd_relay_osd)
# ---------------------------------------------------------------------------------------
def _relay_check_soft(soft):
    if soft not in _lib.RELAY_SOFT:
        raise ValueError(f"soft must be 'last' or 'mean', got {soft!r}")


def _relay_device_inputs(name, graph, x, gammas):
    """The checks ops.relay makes on its device inputs -> (x, gammas) contiguous, B."""
    _require_gpu(x, gammas)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'{name} supports float32/float64, got {x.dtype}')
    if gammas.dtype != x.dtype:
        raise TypeError(f'gammas must have the dtype of x ({x.dtype}), got {gammas.dtype}')
    x = x.contiguous()
    gammas = gammas.contiguous()
    B = x.numel() // graph.N
    if x.numel() != B * graph.N:
        raise ValueError(f'x must hold B*N values (N = {graph.N})')
    return x, gammas, B


def relay_soft(graph, x, gammas, iters0, iters_leg=None, stop_after=1, alpha=0.75, beta=0.0,
               soft='last', out=None):
    """relay with a soft output, one HIP launch (gnnd_relay_soft): everything ops.relay returns,
    bit for bit, plus a soft LLR per variable and its probability, the input osd_gated needs.  For
    a solved codeword the soft LLR is the kept solution's llr; for an unsolved one it is the last
    iteration's llr (soft='last') or the mean of the posteriors over every iteration of every leg
    (soft='mean').  -> (pred, soft, ehat, llr, iters_used, status, leg, nsol): pred [B*V, 1] =
    1 / (1 + exp(soft)), soft [B*V, 1], the rest as for relay.  soft is bit-reproducible, pred in
    float64 too (relay_soft_host gives the same bits).  `out` = the eight tensors to write into;
    each but pred and ehat may be None to skip it (returned as None)."""
    if gammas.dim() != 2 or gammas.shape[1] != graph.V:
        raise ValueError(f'gammas must be [legs, V] (V = {graph.V})')
    legs = gammas.shape[0]
    iters_leg, alpha, beta = _relay_check_params(iters0, iters_leg, stop_after, alpha, beta, legs)
    _relay_check_soft(soft)
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.relay_soft(graph.gid, x, gammas, iters0, iters_leg, stop_after,
                                             alpha, beta, soft)
        if len(out) != 8 or any(o is None for o in out):
            raise ValueError('traced relay_soft needs all eight out tensors')
        torch.ops.gnnd.relay_soft_out(graph.gid, x, gammas, iters0, iters_leg, stop_after, alpha,
                                      beta, soft, *out)
        return out
    x, gammas, B = _relay_device_inputs('relay_soft', graph, x, gammas)
    if out is None:
        out = (tuple(torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device) for _ in range(4))
               + tuple(torch.empty(B, dtype=torch.int32, device=x.device) for _ in range(4)))
    if len(out) != 8 or out[0] is None or out[2] is None:
        raise ValueError('out must be (pred, soft, ehat, llr, iters_used, status, leg, nsol); only '
                         'pred and ehat are required')
    _require_gpu(*out)
    for t in out[:4]:
        if t is not None and (t.dtype != x.dtype or t.numel() != B * graph.V
                              or not t.is_contiguous()):
            raise ValueError(f'pred / soft / ehat / llr must be contiguous {x.dtype} '
                             f'[{B * graph.V}]')
    for t in out[4:]:
        if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError(f'iters_used / status / leg / nsol must be contiguous int32 [{B}]')
    _relay_soft_impl(graph, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft, *out)
    return tuple(out)


def _relay_soft_impl(graph, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft, pred,
                     soft_out, ehat, llr, iters_used, status, leg, nsol):
    """gnnd::relay_soft / gnnd::relay_soft_out implementation (gnndecode.library)."""
    _lib.call('gnnd_relay_soft', graph.handle, dtype_code(x.dtype), _ptr(x), _ptr(gammas),
              gammas.shape[0], iters0, iters_leg, stop_after, alpha, beta, _lib.RELAY_SOFT[soft],
              _ptr(pred), _ptr(soft_out), _ptr(ehat), _ptr(llr), _ptr(iters_used), _ptr(status),
              _ptr(leg), _ptr(nsol), x.numel() // graph.N, current_stream(x.device))


def relay_osd(graph, x, gammas, iters0, iters_leg=None, stop_after=1, alpha=0.75, beta=0.0,
              soft='last', base='zero', method='cs', order=10, out=None, work=None):
    """The relay+OSD decoder in one call (gnnd_relay_osd): relay_soft, then osd_gated with the relay
    status as the gate and the relay llr as the pass-through decision, three launches on the
    current stream, no host sync.  -> (ehat, status, choice, pred, llr, iters_used, relay_status,
    leg, nsol): where relay_status is 0 ehat is relay's kept solution, which satisfies the
    syndrome, and choice is -1; elsewhere ehat / status / choice are osd's on the soft output
    `soft` selects.  Everything but a float32 pred is bit-reproducible (relay_osd_host gives the
    same bits).  `out`: the nine tensors to write into; choice, iters_used, leg and nsol may be
    None to skip them; `work` as for osd_gated."""
    if gammas.dim() != 2 or gammas.shape[1] != graph.V:
        raise ValueError(f'gammas must be [legs, V] (V = {graph.V})')
    legs = gammas.shape[0]
    iters_leg, alpha, beta = _relay_check_params(iters0, iters_leg, stop_after, alpha, beta, legs)
    _relay_check_soft(soft)
    _osd_check_method(base, method, order)
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.relay_osd(graph.gid, x, gammas, iters0, iters_leg, stop_after,
                                            alpha, beta, soft, base, method, order)
        if len(out) != 9 or any(o is None for o in out):
            raise ValueError('traced relay_osd needs all nine out tensors')
        torch.ops.gnnd.relay_osd_out(graph.gid, x, gammas, iters0, iters_leg, stop_after, alpha,
                                     beta, soft, base, method, order, *out)
        return out
    x, gammas, B = _relay_device_inputs('relay_osd', graph, x, gammas)
    if out is None:
        def real():
            return torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device)

        def ints():
            return torch.empty(B, dtype=torch.int32, device=x.device)
        out = (real(), ints(), ints(), real(), real(), ints(), ints(), ints(), ints())
    if len(out) != 9:
        raise ValueError('out must be (ehat, status, choice, pred, llr, iters_used, relay_status, '
                         'leg, nsol)')
    ehat, status, choice, pred, llr, iters_used, relay_status, leg, nsol = out
    if any(t is None for t in (ehat, status, pred, llr, relay_status)):
        raise ValueError('only choice, iters_used, leg and nsol may be None in out')
    _require_gpu(*out)
    for t in (ehat, pred, llr):
        if t.dtype != x.dtype or t.numel() != B * graph.V or not t.is_contiguous():
            raise ValueError(f'ehat / pred / llr must be contiguous {x.dtype} [{B * graph.V}]')
    for t in (status, choice, iters_used, relay_status, leg, nsol):
        if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError('status / choice / iters_used / relay_status / leg / nsol must be '
                             f'contiguous int32 [{B}]')
    _relay_osd_impl(graph, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft, base,
                    method, order, *out, work=work)
    return tuple(out)


def _relay_osd_impl(graph, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft, base,
                    method, order, ehat, status, choice, pred, llr, iters_used, relay_status, leg,
                    nsol, work=None):
    """gnnd::relay_osd / gnnd::relay_osd_out implementation (gnndecode.library)."""
    B = x.numel() // graph.N
    work, nbytes = _gated_work(work, B, x.device)
    _lib.call('gnnd_relay_osd', graph.handle, dtype_code(x.dtype), _ptr(x), _ptr(gammas),
              gammas.shape[0], iters0, iters_leg, stop_after, alpha, beta, _lib.RELAY_SOFT[soft],
              _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order, _ptr(pred), _ptr(llr),
              _ptr(iters_used), _ptr(relay_status), _ptr(leg), _ptr(nsol), _ptr(ehat),
              _ptr(status), _ptr(choice), _ptr(work), nbytes, B, current_stream(x.device))


def _relay_host_inputs(name, H, x, gammas):
    """The checks ops.relay_host makes -> (V, C, var, chk, x, gammas, B)."""
    import numpy as np
    from .graph import edge_list
    H = np.asarray(H)
    V, C = H.shape
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError(f'{name} supports float32/float64, got {x.dtype}')
    gammas = np.ascontiguousarray(gammas, x.dtype)
    if gammas.ndim != 2 or gammas.shape[1] != V:
        raise ValueError(f'gammas must be [legs, V] (V = {V})')
    B = x.size // (V + C)
    if x.size != B * (V + C):
        raise ValueError(f'x must hold B*N values (N = {V + C})')
    var, chk = edge_list(H)
    return V, C, var, chk, x, gammas, B


def relay_soft_host(H, x, gammas, iters0, iters_leg=None, stop_after=1, alpha=0.75, beta=0.0,
                    soft='last'):
    """The host mirror of relay_soft (gnnd_relay_soft_host): numpy in, numpy out, no device.
    -> (pred, soft, ehat, llr like x's dtype [B*V], iters_used, status, leg, nsol int32 [B])."""
    import numpy as np
    V, C, var, chk, x, gammas, B = _relay_host_inputs('relay_soft_host', H, x, gammas)
    legs = gammas.shape[0]
    iters_leg, alpha, beta = _relay_check_params(iters0, iters_leg, stop_after, alpha, beta, legs)
    _relay_check_soft(soft)
    real = [np.empty(B * V, x.dtype) for _ in range(4)]
    ints = [np.empty(B, np.int32) for _ in range(4)]
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    _lib.call('gnnd_relay_soft_host', var.ctypes.data_as(P64), chk.ctypes.data_as(P64), var.size,
              V, C, _lib.F32 if x.dtype == np.float32 else _lib.F64, x.ctypes.data,
              gammas.ctypes.data, legs, iters0, iters_leg, stop_after, alpha, beta,
              _lib.RELAY_SOFT[soft], *(a.ctypes.data for a in real),
              *(a.ctypes.data_as(P32) for a in ints), B)
    return tuple(real) + tuple(ints)


def relay_osd_host(H, x, gammas, iters0, iters_leg=None, stop_after=1, alpha=0.75, beta=0.0,
                   soft='last', base='zero', method='cs', order=10):
    """The host mirror of relay_osd (gnnd_relay_osd_host): numpy in, numpy out, no device.
    -> (ehat, status, choice, pred, llr, iters_used, relay_status, leg, nsol)."""
    import numpy as np
    V, C, var, chk, x, gammas, B = _relay_host_inputs('relay_osd_host', H, x, gammas)
    legs = gammas.shape[0]
    iters_leg, alpha, beta = _relay_check_params(iters0, iters_leg, stop_after, alpha, beta, legs)
    _relay_check_soft(soft)
    _osd_check_method(base, method, order)
    ehat, pred, llr = (np.empty(B * V, x.dtype) for _ in range(3))
    status, choice, iters_used, relay_status, leg, nsol = (np.empty(B, np.int32) for _ in range(6))
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    _lib.call('gnnd_relay_osd_host', var.ctypes.data_as(P64), chk.ctypes.data_as(P64), var.size, V,
              C, _lib.F32 if x.dtype == np.float32 else _lib.F64, x.ctypes.data, gammas.ctypes.data,
              legs, iters0, iters_leg, stop_after, alpha, beta, _lib.RELAY_SOFT[soft],
              _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order, pred.ctypes.data,
              llr.ctypes.data, iters_used.ctypes.data_as(P32), relay_status.ctypes.data_as(P32),
              leg.ctypes.data_as(P32), nsol.ctypes.data_as(P32), ehat.ctypes.data,
              status.ctypes.data_as(P32), choice.ctypes.data_as(P32), B)
    return ehat, status, choice, pred, llr, iters_used, relay_status, leg, nsol


# ---------------------------------------------------------------------------------------
# min-sum BP with guided decimation: freeze bits between BP rounds (gnnd_bpgd)
# ---------------------------------------------------------------------------------------
def _bpgd_check_params(iters0, iters_round, rounds, per_round, pick, clamp, alpha, beta):
    for name, val, lo in (('iters0', iters0, 1), ('iters_round', iters_round, 1),
                          ('rounds', rounds, 0), ('per_round', per_round, 1)):
        if not isinstance(val, int) or isinstance(val, bool) or not lo <= val <= 2 ** 31 - 1:
            raise ValueError(f'{name} must be an integer >= {lo}, got {val!r}')
    if iters0 + rounds * iters_round > 2 ** 31 - 1:
        raise ValueError('iters0 + rounds * iters_round must fit an int32')
    if pick not in _lib.BPGD_PICK:
        raise ValueError(f"pick must be 'least' or 'most', got {pick!r}")
    clamp = float(clamp)
    if not 0.0 < clamp < float('inf'):
        raise ValueError(f'clamp must be finite and > 0, got {clamp!r}')
    alpha, beta = _minsum_check_params(1, alpha, beta)
    return clamp, alpha, beta


def bpgd(graph, x, iters0, iters_round, rounds, per_round=1, pick='least', clamp=25.0, alpha=0.75,
         beta=0.0, out=None):
    """Min-sum BP with guided decimation, one HIP launch (gnnd_bpgd, defined in include/gnnd.h):
    iters0 min-sum iterations, then up to `rounds` rounds that freeze the prior of `per_round`
    undecimated variables at +-clamp (the sign of their current posterior) and run iters_round
    more iterations from the same messages; pick='least' freezes the least reliable variables
    (smallest |llr|, the rule that breaks the ties of a degenerate code), pick='most' the most
    reliable ones.  A codeword stops at its first hard decision that satisfies the syndrome.
    x [B*N(,1)] as for minsum -> (ehat, llr, pred, iters_used, status, ndec): ehat [B*V, 1] exactly
    0.0 / 1.0 and llr [B*V, 1] of the last executed iteration, pred [B*V, 1] = 1 / (1 + exp(llr)),
    iters_used [B] int32, status [B] int32 0 where ehat satisfies the syndrome, ndec [B] int32 the
    variables frozen.  Everything but a float32 pred is bit-reproducible (bpgd_host gives the same
    bits); pred, status and llr are what osd_gated takes.  No host sync; `out` = the six tensors to
    write into, each but ehat may be None to skip it (returned as None)."""
    clamp, alpha, beta = _bpgd_check_params(iters0, iters_round, rounds, per_round, pick, clamp,
                                            alpha, beta)
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.bpgd(graph.gid, x, iters0, iters_round, rounds, per_round, pick,
                                       clamp, alpha, beta)
        if len(out) != 6 or any(o is None for o in out):
            raise ValueError('traced bpgd needs out = (ehat, llr, pred, iters_used, status, ndec)')
        torch.ops.gnnd.bpgd_out(graph.gid, x, iters0, iters_round, rounds, per_round, pick, clamp,
                                alpha, beta, *out)
        return out
    _require_gpu(x)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'bpgd supports float32/float64, got {x.dtype}')
    x = x.contiguous()
    B = x.numel() // graph.N
    if x.numel() != B * graph.N:
        raise ValueError(f'x must hold B*N values (N = {graph.N})')
    if out is None:
        out = (tuple(torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device) for _ in range(3))
               + tuple(torch.empty(B, dtype=torch.int32, device=x.device) for _ in range(3)))
    if len(out) != 6 or out[0] is None:
        raise ValueError('out must be (ehat, llr, pred, iters_used, status, ndec); only ehat is '
                         'required')
    _require_gpu(*out)
    for t in out[:3]:
        if t is not None and (t.dtype != x.dtype or t.numel() != B * graph.V
                              or not t.is_contiguous()):
            raise ValueError(f'ehat / llr / pred must be contiguous {x.dtype} [{B * graph.V}]')
    for t in out[3:]:
        if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError(f'iters_used / status / ndec must be contiguous int32 [{B}]')
    _bpgd_impl(graph, x, iters0, iters_round, rounds, per_round, pick, clamp, alpha, beta, *out)
    return tuple(out)


def _bpgd_impl(graph, x, iters0, iters_round, rounds, per_round, pick, clamp, alpha, beta, ehat,
               llr, pred, iters_used, status, ndec):
    """gnnd::bpgd / gnnd::bpgd_out implementation (gnndecode.library)."""
    _lib.call('gnnd_bpgd', graph.handle, dtype_code(x.dtype), _ptr(x), alpha, beta, iters0,
              iters_round, rounds, per_round, _lib.BPGD_PICK[pick], clamp, _ptr(ehat), _ptr(llr),
              _ptr(pred), _ptr(iters_used), _ptr(status), _ptr(ndec), x.numel() // graph.N,
              current_stream(x.device))


def bpgd_host(H, x, iters0, iters_round, rounds, per_round=1, pick='least', clamp=25.0, alpha=0.75,
              beta=0.0):
    """The host mirror of bpgd (gnnd_bpgd_host): numpy in, numpy out, no device.  H [V, C], x [B*N]
    float32 or float64 -> (ehat, llr, pred like x's dtype [B*V], iters_used, status, ndec int32
    [B])."""
    import numpy as np
    from .graph import edge_list
    clamp, alpha, beta = _bpgd_check_params(iters0, iters_round, rounds, per_round, pick, clamp,
                                            alpha, beta)
    H = np.asarray(H)
    V, C = H.shape
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError(f'bpgd_host supports float32/float64, got {x.dtype}')
    B = x.size // (V + C)
    if x.size != B * (V + C):
        raise ValueError(f'x must hold B*N values (N = {V + C})')
    var, chk = edge_list(H)
    real = [np.empty(B * V, x.dtype) for _ in range(3)]
    ints = [np.empty(B, np.int32) for _ in range(3)]
    P64, P32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    _lib.call('gnnd_bpgd_host', var.ctypes.data_as(P64), chk.ctypes.data_as(P64), var.size, V, C,
              _lib.F32 if x.dtype == np.float32 else _lib.F64, x.ctypes.data, alpha, beta, iters0,
              iters_round, rounds, per_round, _lib.BPGD_PICK[pick], clamp,
              *(a.ctypes.data for a in real), *(a.ctypes.data_as(P32) for a in ints), B)
    return tuple(real) + tuple(ints)


# ---------------------------------------------------------------------------------------
# union-find decoding of a matchable code: grow, merge, peel (gnnd_uf)
# ---------------------------------------------------------------------------------------
def uf(graph, x, gate=None, out=None):
    """The union-find decoder, one HIP launch (gnnd_uf, defined in include/gnnd.h): clusters grow
    around the defects of the syndrome in x by half-edges, merge, and a spanning forest of each is
    peeled.  `graph` must be matchable (every variable of degree 1 or 2, toric_code(L) is); only
    the signs of x's check rows are read.  x [B*N(,1)] as for minsum -> (ehat, rounds, status,
    nfull): ehat [B*V, 1] exactly 0.0 / 1.0, which always satisfies the syndrome; rounds [B] int32
    the growth rounds; status [B] int32, 0 for a decoded codeword; nfull [B] int32 the fully grown
    edges.  gate [B] int32 (for instance the status of bpgd, relay or minsum): codewords whose gate
    is 0 are skipped and none of their outputs written, so
        ops.uf(g, x, gate=status, out=(ehat, None, status, None))
    finishes exactly the codewords another decoder left unsolved.  Bit-reproducible (uf_host gives
    the same bits).  No host sync; `out` = the four tensors to write into, each but ehat may be
    None to skip it (returned as None)."""
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.uf(graph.gid, x, gate)
        if len(out) != 4 or any(o is None for o in out):
            raise ValueError('traced uf needs out = (ehat, rounds, status, nfull)')
        torch.ops.gnnd.uf_out(graph.gid, x, gate, *out)
        return out
    _require_gpu(x, gate)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'uf supports float32/float64, got {x.dtype}')
    x = x.contiguous()
    B = x.numel() // graph.N
    if x.numel() != B * graph.N:
        raise ValueError(f'x must hold B*N values (N = {graph.N})')
    if gate is not None:
        if gate.dtype != torch.int32:
            raise TypeError(f'gate must be int32, got {gate.dtype}')
        gate = gate.contiguous()
        if gate.numel() != B:
            raise ValueError(f'gate must hold B = {B} values')
    if out is None:
        out = ((torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device),)
               + tuple(torch.empty(B, dtype=torch.int32, device=x.device) for _ in range(3)))
    if len(out) != 4 or out[0] is None:
        raise ValueError('out must be (ehat, rounds, status, nfull); only ehat is required')
    _require_gpu(*out)
    if out[0].dtype != x.dtype or out[0].numel() != B * graph.V or not out[0].is_contiguous():
        raise ValueError(f'ehat must be contiguous {x.dtype} [{B * graph.V}]')
    for t in out[1:]:
        if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError(f'rounds / status / nfull must be contiguous int32 [{B}]')
    _uf_impl(graph, x, gate, *out)
    return tuple(out)


def _uf_impl(graph, x, gate, ehat, rounds, status, nfull):
    """gnnd::uf / gnnd::uf_out implementation (gnndecode.library)."""
    _lib.call('gnnd_uf', graph.handle, dtype_code(x.dtype), _ptr(x), _ptr(gate), _ptr(ehat),
              _ptr(rounds), _ptr(status), _ptr(nfull), x.numel() // graph.N,
              current_stream(x.device))


def uf_host(H, x, gate=None):
    """The host mirror of uf (gnnd_uf_host): numpy in, numpy out, no device.  H [V, C], x [B*N]
    float32 or float64, gate [B] int32 or None -> (ehat like x's dtype [B*V], rounds, status, nfull
    int32 [B]).  The rows a gate skips are returned as zeros."""
    import numpy as np
    V, C, var, chk, vp, cp = _host_graph(H)
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError(f'uf_host supports float32/float64, got {x.dtype}')
    B = x.size // (V + C)
    if x.size != B * (V + C):
        raise ValueError(f'x must hold B*N values (N = {V + C})')
    P32 = ctypes.POINTER(ctypes.c_int32)
    if gate is not None:
        gate = np.ascontiguousarray(gate, dtype=np.int32)
        if gate.size != B:
            raise ValueError(f'gate must hold B = {B} values')
    ehat = np.zeros(B * V, x.dtype)
    ints = [np.zeros(B, np.int32) for _ in range(3)]
    _lib.call('gnnd_uf_host', vp, cp, var.size, V, C,
              _lib.F32 if x.dtype == np.float32 else _lib.F64, x.ctypes.data,
              None if gate is None else gate.ctypes.data_as(P32), ehat.ctypes.data,
              *(a.ctypes.data_as(P32) for a in ints), B)
    return (ehat,) + tuple(ints)


def matching_host(H):
    """The decoding graph of H [V, C] on the host (gnnd_graph_matching_host) -> (N, endpoints
    int32 [V, 2]), as TannerGraph.matching gives it."""
    import numpy as np
    V, C, var, chk, vp, cp = _host_graph(H)
    n = ctypes.c_int32()
    ends = np.empty((V, 2), np.int32)
    _lib.call('gnnd_graph_matching_host', vp, cp, var.size, V, C, ctypes.byref(n),
              ends.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return int(n.value), ends


# ---------------------------------------------------------------------------------------
# weighted union-find (gnnd_ufw) and the one-call belief-find decoder (gnnd_belief_find)
# ---------------------------------------------------------------------------------------
UFW_MAX_WEIGHT = 1024     # kGnndUfwMaxWeight


def _ufw_check_params(scale, wmax):
    scale = float(scale)
    if not 0.0 <= scale < float('inf'):
        raise ValueError(f'scale must be finite and >= 0, got {scale!r}')
    if not isinstance(wmax, int) or isinstance(wmax, bool) or not 1 <= wmax <= UFW_MAX_WEIGHT:
        raise ValueError(f'wmax must be an integer in [1, {UFW_MAX_WEIGHT}], got {wmax!r}')
    return scale


def ufw(graph, x, llr=None, scale=2.0, wmax=32, gate=None, passthrough=False, out=None):
    """Weighted union-find, one HIP launch (gnnd_ufw, defined in include/gnnd.h): uf with the
    length of edge v its quantised reliability, w = clamp(1 + trunc(r_v * scale), 1, wmax) with
    r_v = llr [B*V(,1)] if given (the posteriors of minsum, relay_soft or bpgd: "belief-find"),
    else the priors in x; a negative, zero or NaN reliability gives 1.  Clusters grow fast through
    bits believed flipped and slowly through reliable ones.  -> (ehat, rounds, status, nfull,
    events): as uf, rounds in unit half-steps, events [B] int32 the growth events (the jumps from
    one filled edge to the next).  scale = 0 or wmax = 1 gives uf's bits.  gate [B] int32 as for
    uf: codewords whose gate is 0 are skipped and none of their outputs written, so
        ops.ufw(g, x, llr=llr, gate=status, out=(ehat, None, status, None, None))
    finishes the codewords relay_soft or bpgd left unsolved, on the posteriors they stopped with.
    passthrough=True (needs gate and llr) instead writes ehat = (llr < 0) and zero counters for
    them.  Bit-reproducible (ufw_host gives the same bits).  The defaults scale = 2.0, wmax = 32
    are not tuned: nobody has measured them against others beyond the grid of
    tools/ufw_bench.py.  No host sync; `out` = the five tensors to write into, each but ehat may
    be None to skip it (returned as None)."""
    scale = _ufw_check_params(scale, wmax)
    passthrough = bool(passthrough)
    if passthrough and (gate is None or llr is None):
        raise ValueError('passthrough needs gate and llr')
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.ufw(graph.gid, x, llr, scale, wmax, gate, passthrough)
        if len(out) != 5 or any(o is None for o in out):
            raise ValueError('traced ufw needs out = (ehat, rounds, status, nfull, events)')
        torch.ops.gnnd.ufw_out(graph.gid, x, llr, scale, wmax, gate, passthrough, *out)
        return out
    _require_gpu(x, llr, gate)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'ufw supports float32/float64, got {x.dtype}')
    x = x.contiguous()
    B = x.numel() // graph.N
    if x.numel() != B * graph.N:
        raise ValueError(f'x must hold B*N values (N = {graph.N})')
    if llr is not None:
        if llr.dtype != x.dtype:
            raise TypeError(f'x ({x.dtype}) and llr ({llr.dtype}) must share a dtype')
        llr = llr.contiguous()
        if llr.numel() != B * graph.V:
            raise ValueError(f'llr must hold B*V values (V = {graph.V})')
    if gate is not None:
        if gate.dtype != torch.int32:
            raise TypeError(f'gate must be int32, got {gate.dtype}')
        gate = gate.contiguous()
        if gate.numel() != B:
            raise ValueError(f'gate must hold B = {B} values')
    if out is None:
        out = ((torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device),)
               + tuple(torch.empty(B, dtype=torch.int32, device=x.device) for _ in range(4)))
    if len(out) != 5 or out[0] is None:
        raise ValueError('out must be (ehat, rounds, status, nfull, events); only ehat is required')
    _require_gpu(*out)
    if out[0].dtype != x.dtype or out[0].numel() != B * graph.V or not out[0].is_contiguous():
        raise ValueError(f'ehat must be contiguous {x.dtype} [{B * graph.V}]')
    for t in out[1:]:
        if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError(f'rounds / status / nfull / events must be contiguous int32 [{B}]')
    _ufw_impl(graph, x, llr, scale, wmax, gate, passthrough, *out)
    return tuple(out)


def _ufw_impl(graph, x, llr, scale, wmax, gate, passthrough, ehat, rounds, status, nfull, events):
    """gnnd::ufw / gnnd::ufw_out implementation (gnndecode.library)."""
    _lib.call('gnnd_ufw', graph.handle, dtype_code(x.dtype), _ptr(x), _ptr(llr), scale, wmax,
              _ptr(gate), int(passthrough), _ptr(ehat), _ptr(rounds), _ptr(status), _ptr(nfull),
              _ptr(events), x.numel() // graph.N, current_stream(x.device))


def ufw_host(H, x, llr=None, scale=2.0, wmax=32, gate=None, passthrough=False):
    """The host mirror of ufw (gnnd_ufw_host): numpy in, numpy out, no device.  H [V, C], x [B*N]
    float32 or float64, llr [B*V] or None, gate [B] int32 or None -> (ehat like x's dtype [B*V],
    rounds, status, nfull, events int32 [B]).  The rows a gate skips are returned as zeros."""
    import numpy as np
    scale = _ufw_check_params(scale, wmax)
    if passthrough and (gate is None or llr is None):
        raise ValueError('passthrough needs gate and llr')
    V, C, var, chk, vp, cp = _host_graph(H)
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError(f'ufw_host supports float32/float64, got {x.dtype}')
    B = x.size // (V + C)
    if x.size != B * (V + C):
        raise ValueError(f'x must hold B*N values (N = {V + C})')
    if llr is not None:
        llr = np.ascontiguousarray(llr, dtype=x.dtype)
        if llr.size != B * V:
            raise ValueError(f'llr must hold B*V values (V = {V})')
    P32 = ctypes.POINTER(ctypes.c_int32)
    if gate is not None:
        gate = np.ascontiguousarray(gate, dtype=np.int32)
        if gate.size != B:
            raise ValueError(f'gate must hold B = {B} values')
    ehat = np.zeros(B * V, x.dtype)
    ints = [np.zeros(B, np.int32) for _ in range(4)]
    _lib.call('gnnd_ufw_host', vp, cp, var.size, V, C,
              _lib.F32 if x.dtype == np.float32 else _lib.F64, x.ctypes.data,
              None if llr is None else llr.ctypes.data, scale, wmax,
              None if gate is None else gate.ctypes.data_as(P32), int(bool(passthrough)),
              ehat.ctypes.data, *(a.ctypes.data_as(P32) for a in ints), B)
    return (ehat,) + tuple(ints)


def belief_find(graph, x, iters, alpha=0.75, beta=0.0, early_stop=True, scale=2.0, wmax=32,
                out=None):
    """Belief-find in one call (gnnd_belief_find): minsum, then ufw on the min-sum posteriors with
    the min-sum status as the gate and passthrough on, two launches on the current stream, no
    workspace, no host sync.  `graph` must be matchable.  -> (ehat, status, iters_used, bp_status,
    pred, llr, rounds, nfull, events): where bp_status is 0, ehat is min-sum's hard decision,
    which satisfies the syndrome, and rounds / nfull / events are 0; elsewhere ehat / status /
    rounds / nfull / events are ufw's.  Like bposd it always returns a syndrome-satisfying
    estimate (on a graph whose components all have a virtual vertex, toric_code(L) is one), with
    no elimination.  Everything but pred is bit-reproducible (belief_find_host gives the same
    bits).  The defaults scale = 2.0, wmax = 32 are not tuned (see ufw).  `out`: the nine tensors
    to write into; status, iters_used, rounds, nfull and events may be None to skip them."""
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    early_stop = bool(early_stop)
    scale = _ufw_check_params(scale, wmax)
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.belief_find(graph.gid, x, iters, alpha, beta, early_stop, scale,
                                              wmax)
        if len(out) != 9 or any(o is None for o in out):
            raise ValueError('traced belief_find needs all nine out tensors')
        torch.ops.gnnd.belief_find_out(graph.gid, x, iters, alpha, beta, early_stop, scale, wmax,
                                       *out)
        return out
    _require_gpu(x)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'belief_find supports float32/float64, got {x.dtype}')
    x = x.contiguous()
    B = x.numel() // graph.N
    if x.numel() != B * graph.N:
        raise ValueError(f'x must hold B*N values (N = {graph.N})')
    if out is None:
        def real():
            return torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device)

        def ints():
            return torch.empty(B, dtype=torch.int32, device=x.device)
        out = (real(), ints(), ints(), ints(), real(), real(), ints(), ints(), ints())
    if len(out) != 9:
        raise ValueError('out must be (ehat, status, iters_used, bp_status, pred, llr, rounds, '
                         'nfull, events)')
    ehat, status, iters_used, bp_status, pred, llr, rounds, nfull, events = out
    if any(t is None for t in (ehat, bp_status, pred, llr)):
        raise ValueError('ehat, bp_status, pred and llr are required in out')
    _require_gpu(*out)
    for t in (ehat, pred, llr):
        if t.dtype != x.dtype or t.numel() != B * graph.V or not t.is_contiguous():
            raise ValueError(f'ehat / pred / llr must be contiguous {x.dtype} [{B * graph.V}]')
    for t in (status, iters_used, bp_status, rounds, nfull, events):
        if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError('status / iters_used / bp_status / rounds / nfull / events must be '
                             f'contiguous int32 [{B}]')
    _belief_find_impl(graph, x, iters, alpha, beta, early_stop, scale, wmax, *out)
    return tuple(out)


def _belief_find_impl(graph, x, iters, alpha, beta, early_stop, scale, wmax, ehat, status,
                      iters_used, bp_status, pred, llr, rounds, nfull, events):
    """gnnd::belief_find / gnnd::belief_find_out implementation (gnndecode.library)."""
    _lib.call('gnnd_belief_find', graph.handle, dtype_code(x.dtype), _ptr(x), alpha, beta, iters,
              int(early_stop), scale, wmax, _ptr(pred), _ptr(llr), _ptr(iters_used),
              _ptr(bp_status), _ptr(ehat), _ptr(status), _ptr(rounds), _ptr(nfull), _ptr(events),
              x.numel() // graph.N, current_stream(x.device))


def belief_find_host(H, x, iters, alpha=0.75, beta=0.0, early_stop=True, scale=2.0, wmax=32):
    """The host mirror of belief_find (gnnd_belief_find_host): numpy in, numpy out, no device.
    -> (ehat, status, iters_used, bp_status, pred, llr, rounds, nfull, events)."""
    import numpy as np
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    scale = _ufw_check_params(scale, wmax)
    V, C, var, chk, vp, cp = _host_graph(H)
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError(f'belief_find_host supports float32/float64, got {x.dtype}')
    B = x.size // (V + C)
    if x.size != B * (V + C):
        raise ValueError(f'x must hold B*N values (N = {V + C})')
    ehat, pred, llr = (np.empty(B * V, x.dtype) for _ in range(3))
    status, iters_used, bp_status, rounds, nfull, events = (np.empty(B, np.int32)
                                                            for _ in range(6))
    P32 = ctypes.POINTER(ctypes.c_int32)
    _lib.call('gnnd_belief_find_host', vp, cp, var.size, V, C,
              _lib.F32 if x.dtype == np.float32 else _lib.F64, x.ctypes.data, alpha, beta, iters,
              int(bool(early_stop)), scale, wmax, pred.ctypes.data, llr.ctypes.data,
              iters_used.ctypes.data_as(P32), bp_status.ctypes.data_as(P32), ehat.ctypes.data,
              status.ctypes.data_as(P32), rounds.ctypes.data_as(P32), nfull.ctypes.data_as(P32),
              events.ctypes.data_as(P32), B)
    return ehat, status, iters_used, bp_status, pred, llr, rounds, nfull, events


# ---------------------------------------------------------------------------------------
# gated OSD (gnnd_osd_gated) and the one-call BP+OSD decoder (gnnd_bposd)
# ---------------------------------------------------------------------------------------
def osd_gated_workspace(B):
    """Bytes of scratch gnnd_osd_gated / gnnd_bposd need for a batch of B codewords."""
    n = ctypes.c_int64()
    _lib.call('gnnd_osd_gated_workspace', B, ctypes.byref(n))
    return n.value


def _gated_work(work, B, device):
    need = osd_gated_workspace(B)
    if work is None:
        return torch.empty(need, dtype=torch.uint8, device=device), need
    _require_gpu(work)
    have = work.numel() * work.element_size()
    if have < need or not work.is_contiguous() or work.data_ptr() % 4:
        raise ValueError(f'work must be a contiguous 4-byte aligned tensor of >= {need} bytes')
    return work, have


def _check_ehat_status_choice(out, dtype, B, V):
    """(ehat, status[, choice]) of the OSD calls -> (ehat, status, choice or None)."""
    if len(out) not in (2, 3):
        raise ValueError('out must be (ehat, status) or (ehat, status, choice)')
    ehat, status = out[0], out[1]
    choice = out[2] if len(out) == 3 else None
    _require_gpu(ehat, status, choice)
    if (ehat.dtype != dtype or ehat.numel() != B * V or not ehat.is_contiguous()
            or status.dtype != torch.int32 or status.numel() != B or not status.is_contiguous()):
        raise ValueError(f'out must be (contiguous {dtype} [{B * V}], contiguous int32 [{B}], ...)')
    if choice is not None and (choice.dtype != torch.int32 or choice.numel() != B
                               or not choice.is_contiguous()):
        raise ValueError(f'choice must be contiguous int32 [{B}]')
    return ehat, status, choice


def osd_gated(graph, x, pred, gate, base='zero', method='cs', order=10, llr=None, out=None,
              work=None):
    """osd on the codewords a gate selects (gnnd_osd_gated): gate [B] int32, for instance minsum's
    status.  Where gate != 0, ehat / status / choice are bit for bit osd's; where gate == 0 the
    codeword passes through: ehat is the hard decision (llr < 0 if llr [B*V(,1)] is given, else
    pred > 0.5) as 0.0 / 1.0, status 0, choice -1, its syndrome not re-checked.  Give llr with a
    min-sum gate: pred rounds to exactly 0.5 for a tiny |llr| and then loses the decision the
    status was computed from.  Two launches (a compaction of the gate on the device, then osd's
    kernel over the gated list), no host sync.  -> (ehat, status, choice); `out` as for osd;
    `work`: a scratch tensor of osd_gated_workspace(B) bytes, allocated with torch.empty when
    None."""
    _osd_check_method(base, method, order)
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.osd_gated(graph.gid, x, pred, gate, base, method, order, llr)
        if len(out) != 3 or out[2] is None:
            raise ValueError('traced osd_gated needs out = (ehat, status, choice)')
        torch.ops.gnnd.osd_gated_out(graph.gid, x, pred, gate, base, method, order, llr, *out)
        return out
    _require_gpu(x, pred, gate, llr)
    if x.dtype != pred.dtype or (llr is not None and llr.dtype != pred.dtype):
        raise TypeError(f'x ({x.dtype}), pred ({pred.dtype}) and llr must share a dtype')
    if pred.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'osd_gated supports float32/float64, got {pred.dtype}')
    if gate.dtype != torch.int32:
        raise TypeError(f'gate must be int32, got {gate.dtype}')
    x = x.contiguous()
    pred = pred.contiguous()
    gate = gate.contiguous()
    B = pred.numel() // graph.V
    if pred.numel() != B * graph.V or x.numel() != B * graph.N or gate.numel() != B:
        raise ValueError(f'pred must hold B*V, x B*N and gate B values (V = {graph.V}, '
                         f'N = {graph.N})')
    if llr is not None:
        llr = llr.contiguous()
        if llr.numel() != pred.numel():
            raise ValueError('llr must hold B*V values')
    if out is None:
        out = (torch.empty_like(pred), torch.empty(B, dtype=torch.int32, device=pred.device),
               torch.empty(B, dtype=torch.int32, device=pred.device))
    ehat, status, choice = _check_ehat_status_choice(out, pred.dtype, B, graph.V)
    _osd_gated_impl(graph, x, pred, gate, base, method, order, llr, ehat, status, choice, work)
    return ehat, status, choice


def _osd_gated_impl(graph, x, pred, gate, base, method, order, llr, ehat, status, choice,
                    work=None):
    """gnnd::osd_gated / gnnd::osd_gated_out implementation (gnndecode.library)."""
    B = pred.numel() // graph.V
    work, nbytes = _gated_work(work, B, pred.device)
    _lib.call('gnnd_osd_gated', graph.handle, dtype_code(pred.dtype), _ptr(x), _ptr(pred),
              _ptr(llr), _ptr(gate), _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order,
              _ptr(ehat), _ptr(status), _ptr(choice), _ptr(work), nbytes, B,
              current_stream(pred.device))


def bposd(graph, x, iters, alpha=0.75, beta=0.0, early_stop=True, base='zero', method='cs',
          order=10, out=None, work=None, schedule='flooding'):
    """The BP+OSD decoder in one call (gnnd_bposd): minsum, then osd_gated with the min-sum status
    as the gate and the min-sum llr as the pass-through decision, three launches on the current
    stream, no host sync.  -> (ehat, status, choice, iters_used, bp_status, pred, llr): where
    bp_status is 0 ehat is min-sum's hard decision, which satisfies the syndrome, and choice is
    -1; elsewhere ehat / status / choice are osd's.  Everything but pred is bit-reproducible
    (bposd_host gives the same bits).  `out`: the seven tensors to write into, choice and
    iters_used may be None to skip them; `work` as for osd_gated.  schedule='layered' runs the
    min-sum stage on the layered schedule (gnnd_bposd_layered, mirror bposd_host(...,
    schedule='layered')); the OSD stage is the same."""
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    early_stop = bool(early_stop)
    _osd_check_method(base, method, order)
    suffix = _schedule_suffix(schedule)
    if torch.compiler.is_compiling():
        if out is None:
            return getattr(torch.ops.gnnd, 'bposd' + suffix)(graph.gid, x, iters, alpha, beta,
                                                             early_stop, base, method, order)
        if len(out) != 7 or any(o is None for o in out):
            raise ValueError('traced bposd needs all seven out tensors')
        getattr(torch.ops.gnnd, 'bposd' + suffix + '_out')(graph.gid, x, iters, alpha, beta,
                                                           early_stop, base, method, order, *out)
        return out
    _require_gpu(x)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'bposd supports float32/float64, got {x.dtype}')
    x = x.contiguous()
    B = x.numel() // graph.N
    if x.numel() != B * graph.N:
        raise ValueError(f'x must hold B*N values (N = {graph.N})')
    if out is None:
        def real():
            return torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device)

        def ints():
            return torch.empty(B, dtype=torch.int32, device=x.device)
        out = (real(), ints(), ints(), ints(), ints(), real(), real())
    if len(out) != 7:
        raise ValueError('out must be (ehat, status, choice, iters_used, bp_status, pred, llr)')
    ehat, status, choice, iters_used, bp_status, pred, llr = out
    if any(t is None for t in (ehat, status, bp_status, pred, llr)):
        raise ValueError('only choice and iters_used may be None in out')
    _require_gpu(*out)
    for t in (ehat, pred, llr):
        if t.dtype != x.dtype or t.numel() != B * graph.V or not t.is_contiguous():
            raise ValueError(f'ehat / pred / llr must be contiguous {x.dtype} [{B * graph.V}]')
    for t in (status, choice, iters_used, bp_status):
        if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError(f'status / choice / iters_used / bp_status must be contiguous int32 [{B}]')
    _bposd_impl(graph, x, iters, alpha, beta, early_stop, base, method, order, ehat, status, choice,
                iters_used, bp_status, pred, llr, work, schedule)
    return tuple(out)


def _bposd_impl(graph, x, iters, alpha, beta, early_stop, base, method, order, ehat, status, choice,
                iters_used, bp_status, pred, llr, work=None, schedule='flooding'):
    """gnnd::bposd[_layered] / gnnd::bposd[_layered]_out implementation (gnndecode.library)."""
    B = x.numel() // graph.N
    work, nbytes = _gated_work(work, B, x.device)
    _lib.call('gnnd_bposd' + _schedule_suffix(schedule), graph.handle, dtype_code(x.dtype), _ptr(x), alpha, beta, iters,
              int(early_stop), _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order, _ptr(pred),
              _ptr(llr), _ptr(iters_used), _ptr(bp_status), _ptr(ehat), _ptr(status), _ptr(choice),
              _ptr(work), nbytes, B, current_stream(x.device))


def _host_graph(H):
    import numpy as np
    from .graph import edge_list
    H = np.asarray(H)
    var, chk = edge_list(H)
    P64 = ctypes.POINTER(ctypes.c_int64)
    return H.shape[0], H.shape[1], var, chk, var.ctypes.data_as(P64), chk.ctypes.data_as(P64)


def osd_gated_host(H, x, pred, gate, base='zero', method='cs', order=10, llr=None):
    """The host mirror of osd_gated (gnnd_osd_gated_host): numpy in, numpy out, no device.
    -> (ehat like pred, status int32 [B], choice int32 [B])."""
    import numpy as np
    _osd_check_method(base, method, order)
    V, C, var, chk, vp, cp = _host_graph(H)
    pred = np.ascontiguousarray(pred)
    if pred.dtype not in (np.float32, np.float64):
        raise TypeError(f'osd_gated_host supports float32/float64, got {pred.dtype}')
    x = np.ascontiguousarray(x, dtype=pred.dtype)
    gate = np.ascontiguousarray(gate, dtype=np.int32)
    B = pred.size // V
    if pred.size != B * V or x.size != B * (V + C) or gate.size != B:
        raise ValueError(f'pred must hold B*V, x B*N and gate B values (V = {V}, N = {V + C})')
    if llr is not None:
        llr = np.ascontiguousarray(llr, dtype=pred.dtype)
        if llr.size != pred.size:
            raise ValueError('llr must hold B*V values')
    ehat = np.empty_like(pred)
    status = np.empty(B, np.int32)
    choice = np.empty(B, np.int32)
    P32 = ctypes.POINTER(ctypes.c_int32)
    _lib.call('gnnd_osd_gated_host', vp, cp, var.size, V, C,
              _lib.F32 if pred.dtype == np.float32 else _lib.F64, x.ctypes.data, pred.ctypes.data,
              None if llr is None else llr.ctypes.data, gate.ctypes.data_as(P32),
              _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order, ehat.ctypes.data,
              status.ctypes.data_as(P32), choice.ctypes.data_as(P32), B)
    return ehat, status, choice


def bposd_host(H, x, iters, alpha=0.75, beta=0.0, early_stop=True, base='zero', method='cs',
               order=10, schedule='flooding'):
    """The host mirror of bposd (gnnd_bposd_host, gnnd_bposd_layered_host with
    schedule='layered'): numpy in, numpy out, no device.  -> (ehat, status, choice, iters_used,
    bp_status, pred, llr)."""
    import numpy as np
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    suffix = _schedule_suffix(schedule)
    _osd_check_method(base, method, order)
    V, C, var, chk, vp, cp = _host_graph(H)
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError(f'bposd_host supports float32/float64, got {x.dtype}')
    B = x.size // (V + C)
    if x.size != B * (V + C):
        raise ValueError(f'x must hold B*N values (N = {V + C})')
    ehat, pred, llr = (np.empty(B * V, x.dtype) for _ in range(3))
    status, choice, iters_used, bp_status = (np.empty(B, np.int32) for _ in range(4))
    P32 = ctypes.POINTER(ctypes.c_int32)
    _lib.call(f'gnnd_bposd{suffix}_host', vp, cp, var.size, V, C,
              _lib.F32 if x.dtype == np.float32 else _lib.F64, x.ctypes.data, alpha, beta, iters,
              int(bool(early_stop)), _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order,
              pred.ctypes.data, llr.ctypes.data, iters_used.ctypes.data_as(P32),
              bp_status.ctypes.data_as(P32), ehat.ctypes.data, status.ctypes.data_as(P32),
              choice.ctypes.data_as(P32), B)
    return ehat, status, choice, iters_used, bp_status, pred, llr


# ---------------------------------------------------------------------------------------
# localized-statistics decoding (gnnd_lsd, gnnd_lsd_gated) and the one-call BP+LSD decoder
# (gnnd_bplsd)
# ---------------------------------------------------------------------------------------
def _lsd_check_params(base, bits_per_step):
    if base not in _lib.OSD_BASE:
        raise ValueError(f"base must be 'zero' or 'hard', got {base!r}")
    if (not isinstance(bits_per_step, int) or isinstance(bits_per_step, bool)
            or not 0 <= bits_per_step <= 2 ** 31 - 1):
        raise ValueError(f'bits_per_step must be an integer in [0, 2^31 - 1], got {bits_per_step!r}')


def _lsd_inputs(name, graph, x, pred, gate=None, llr=None, gated=False):
    """The checks osd_gated makes of its inputs -> (x, pred, gate, llr, B), contiguous."""
    _require_gpu(x, pred, gate, llr)
    if x.dtype != pred.dtype or (llr is not None and llr.dtype != pred.dtype):
        raise TypeError(f'x ({x.dtype}), pred ({pred.dtype}) and llr must share a dtype')
    if pred.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'{name} supports float32/float64, got {pred.dtype}')
    x = x.contiguous()
    pred = pred.contiguous()
    B = pred.numel() // graph.V
    if pred.numel() != B * graph.V or x.numel() != B * graph.N:
        raise ValueError(f'pred must hold B*V and x B*N values (V = {graph.V}, N = {graph.N})')
    if gated:
        if gate.dtype != torch.int32:
            raise TypeError(f'gate must be int32, got {gate.dtype}')
        gate = gate.contiguous()
        if gate.numel() != B:
            raise ValueError('gate must hold B values')
    if llr is not None:
        llr = llr.contiguous()
        if llr.numel() != pred.numel():
            raise ValueError('llr must hold B*V values')
    return x, pred, gate, llr, B


def _lsd_outs(out, pred, B, V):
    """(ehat, status, rounds, nclus, ncols) of the LSD calls; the four int outputs may be None."""
    dtype = pred.dtype
    if out is None:
        out = (torch.empty_like(pred),) + tuple(
            torch.empty(B, dtype=torch.int32, device=pred.device) for _ in range(4))
    if len(out) != 5:
        raise ValueError('out must be (ehat, status, rounds, nclus, ncols)')
    if out[0] is None:
        raise ValueError('ehat is required in out')
    _require_gpu(*out)
    if out[0].dtype != dtype or out[0].numel() != B * V or not out[0].is_contiguous():
        raise ValueError(f'ehat must be contiguous {dtype} [{B * V}]')
    for t in out[1:]:
        if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError(f'status / rounds / nclus / ncols must be contiguous int32 [{B}]')
    return tuple(out)


def lsd(graph, x, pred, base='zero', bits_per_step=1, out=None):
    """Localized-statistics decoding of a decoder's soft output, one HIP launch (gnnd_lsd):
    clusters grow around the unsatisfied checks, on any Tanner graph, and every round solves them
    by osd0's elimination restricted to the cluster columns.  x, pred and base as for osd0.
    bits_per_step = k > 0: every unsolved cluster takes its k most likely boundary variables per
    round (1, the default, is the published LSD-0 rule); 0: its whole boundary.  -> (ehat, status,
    rounds, nclus, ncols): status [B] is osd0's on every input, and where it is 0 ehat satisfies
    the syndrome and is osd0's solution for the column order "cluster variables first"; rounds
    [B] the growth rounds, nclus [B] the clusters and ncols [B] the cluster variables at the end.
    All outputs are bit-reproducible in both dtypes (lsd_host gives the same bits).  No host
    sync; `out`: the five tensors to write into, all but ehat may be None to skip them."""
    _lsd_check_params(base, bits_per_step)
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.lsd(graph.gid, x, pred, base, bits_per_step)
        if len(out) != 5 or any(o is None for o in out):
            raise ValueError('traced lsd needs all five out tensors')
        torch.ops.gnnd.lsd_out(graph.gid, x, pred, base, bits_per_step, *out)
        return out
    x, pred, _, _, B = _lsd_inputs('lsd', graph, x, pred)
    out = _lsd_outs(out, pred, B, graph.V)
    _lsd_impl(graph, x, pred, base, bits_per_step, *out)
    return out


def _lsd_impl(graph, x, pred, base, bits_per_step, ehat, status, rounds, nclus, ncols):
    """gnnd::lsd / gnnd::lsd_out implementation (gnndecode.library)."""
    _lib.call('gnnd_lsd', graph.handle, dtype_code(pred.dtype), _ptr(x), _ptr(pred),
              _lib.OSD_BASE[base], bits_per_step, _ptr(ehat), _ptr(status), _ptr(rounds),
              _ptr(nclus), _ptr(ncols), pred.numel() // graph.V, current_stream(pred.device))


def lsd_gated(graph, x, pred, gate, base='zero', bits_per_step=1, llr=None, out=None, work=None):
    """lsd on the codewords a gate selects (gnnd_lsd_gated): gate, llr, the pass-through rule, the
    two launches and `work` as for osd_gated.  Where gate != 0 the five outputs are bit for bit
    lsd's; a pass-through codeword gets its hard decision and status = rounds = nclus = ncols =
    0.  -> (ehat, status, rounds, nclus, ncols); `out` as for lsd."""
    _lsd_check_params(base, bits_per_step)
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.lsd_gated(graph.gid, x, pred, gate, base, bits_per_step, llr)
        if len(out) != 5 or any(o is None for o in out):
            raise ValueError('traced lsd_gated needs all five out tensors')
        torch.ops.gnnd.lsd_gated_out(graph.gid, x, pred, gate, base, bits_per_step, llr, *out)
        return out
    x, pred, gate, llr, B = _lsd_inputs('lsd_gated', graph, x, pred, gate, llr, gated=True)
    out = _lsd_outs(out, pred, B, graph.V)
    _lsd_gated_impl(graph, x, pred, gate, base, bits_per_step, llr, *out, work=work)
    return out


def _lsd_gated_impl(graph, x, pred, gate, base, bits_per_step, llr, ehat, status, rounds, nclus,
                    ncols, work=None):
    """gnnd::lsd_gated / gnnd::lsd_gated_out implementation (gnndecode.library)."""
    B = pred.numel() // graph.V
    work, nbytes = _gated_work(work, B, pred.device)
    _lib.call('gnnd_lsd_gated', graph.handle, dtype_code(pred.dtype), _ptr(x), _ptr(pred),
              _ptr(llr), _ptr(gate), _lib.OSD_BASE[base], bits_per_step, _ptr(ehat), _ptr(status),
              _ptr(rounds), _ptr(nclus), _ptr(ncols), _ptr(work), nbytes, B,
              current_stream(pred.device))


def bplsd(graph, x, iters, alpha=0.75, beta=0.0, early_stop=True, base='zero', bits_per_step=1,
          out=None, work=None):
    """The BP+LSD decoder in one call (gnnd_bplsd): minsum (flooding schedule), then lsd_gated with
    the min-sum status as the gate and the min-sum llr as the pass-through decision, three
    launches on the current stream, no host sync.  -> (ehat, status, rounds, nclus, ncols,
    iters_used, bp_status, pred, llr): where bp_status is 0 ehat is min-sum's hard decision and
    every output bposd shares is bposd's; elsewhere ehat / status / rounds / nclus / ncols are
    lsd's.  Everything but pred is bit-reproducible (bplsd_host gives the same bits).  `out`: the
    nine tensors to write into, status, rounds, nclus, ncols and iters_used may be None to skip
    them; `work` as for osd_gated."""
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    early_stop = bool(early_stop)
    _lsd_check_params(base, bits_per_step)
    if torch.compiler.is_compiling():
        if out is None:
            return torch.ops.gnnd.bplsd(graph.gid, x, iters, alpha, beta, early_stop, base,
                                        bits_per_step)
        if len(out) != 9 or any(o is None for o in out):
            raise ValueError('traced bplsd needs all nine out tensors')
        torch.ops.gnnd.bplsd_out(graph.gid, x, iters, alpha, beta, early_stop, base, bits_per_step,
                                 *out)
        return out
    _require_gpu(x)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'bplsd supports float32/float64, got {x.dtype}')
    x = x.contiguous()
    B = x.numel() // graph.N
    if x.numel() != B * graph.N:
        raise ValueError(f'x must hold B*N values (N = {graph.N})')
    if out is None:
        def real():
            return torch.empty(B * graph.V, 1, dtype=x.dtype, device=x.device)

        def ints():
            return torch.empty(B, dtype=torch.int32, device=x.device)
        out = (real(), ints(), ints(), ints(), ints(), ints(), ints(), real(), real())
    if len(out) != 9:
        raise ValueError('out must be (ehat, status, rounds, nclus, ncols, iters_used, bp_status, '
                         'pred, llr)')
    ehat, status, rounds, nclus, ncols, iters_used, bp_status, pred, llr = out
    if any(t is None for t in (ehat, bp_status, pred, llr)):
        raise ValueError('ehat, bp_status, pred and llr are required in out')
    _require_gpu(*out)
    for t in (ehat, pred, llr):
        if t.dtype != x.dtype or t.numel() != B * graph.V or not t.is_contiguous():
            raise ValueError(f'ehat / pred / llr must be contiguous {x.dtype} [{B * graph.V}]')
    for t in (status, rounds, nclus, ncols, iters_used, bp_status):
        if t is not None and (t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError('status / rounds / nclus / ncols / iters_used / bp_status must be '
                             f'contiguous int32 [{B}]')
    _bplsd_impl(graph, x, iters, alpha, beta, early_stop, base, bits_per_step, *out, work=work)
    return tuple(out)


def _bplsd_impl(graph, x, iters, alpha, beta, early_stop, base, bits_per_step, ehat, status,
                rounds, nclus, ncols, iters_used, bp_status, pred, llr, work=None):
    """gnnd::bplsd / gnnd::bplsd_out implementation (gnndecode.library)."""
    B = x.numel() // graph.N
    work, nbytes = _gated_work(work, B, x.device)
    _lib.call('gnnd_bplsd', graph.handle, dtype_code(x.dtype), _ptr(x), alpha, beta, iters,
              int(early_stop), _lib.OSD_BASE[base], bits_per_step, _ptr(pred), _ptr(llr),
              _ptr(iters_used), _ptr(bp_status), _ptr(ehat), _ptr(status), _ptr(rounds),
              _ptr(nclus), _ptr(ncols), _ptr(work), nbytes, B, current_stream(x.device))


def _lsd_host_inputs(name, H, x, pred, gate=None, llr=None, gated=False):
    import numpy as np
    V, C, var, chk, vp, cp = _host_graph(H)
    pred = np.ascontiguousarray(pred)
    if pred.dtype not in (np.float32, np.float64):
        raise TypeError(f'{name} supports float32/float64, got {pred.dtype}')
    x = np.ascontiguousarray(x, dtype=pred.dtype)
    B = pred.size // V
    if pred.size != B * V or x.size != B * (V + C):
        raise ValueError(f'pred must hold B*V and x B*N values (V = {V}, N = {V + C})')
    if gated:
        gate = np.ascontiguousarray(gate, dtype=np.int32)
        if gate.size != B:
            raise ValueError('gate must hold B values')
    if llr is not None:
        llr = np.ascontiguousarray(llr, dtype=pred.dtype)
        if llr.size != pred.size:
            raise ValueError('llr must hold B*V values')
    return V, C, var, vp, cp, x, pred, gate, llr, B


def lsd_host(H, x, pred, base='zero', bits_per_step=1):
    """The host mirror of lsd (gnnd_lsd_host): numpy in, numpy out, no device.  H [V, C], x [B*N],
    pred [B*V] float32 or float64 -> (ehat like pred, status, rounds, nclus, ncols int32 [B])."""
    import numpy as np
    _lsd_check_params(base, bits_per_step)
    V, C, var, vp, cp, x, pred, _, _, B = _lsd_host_inputs('lsd_host', H, x, pred)
    ehat = np.empty_like(pred)
    ints = tuple(np.empty(B, np.int32) for _ in range(4))
    P32 = ctypes.POINTER(ctypes.c_int32)
    _lib.call('gnnd_lsd_host', vp, cp, var.size, V, C,
              _lib.F32 if pred.dtype == np.float32 else _lib.F64, x.ctypes.data, pred.ctypes.data,
              _lib.OSD_BASE[base], bits_per_step, ehat.ctypes.data,
              *(a.ctypes.data_as(P32) for a in ints), B)
    return (ehat,) + ints


def lsd_gated_host(H, x, pred, gate, base='zero', bits_per_step=1, llr=None):
    """The host mirror of lsd_gated (gnnd_lsd_gated_host): numpy in, numpy out, no device.
    -> (ehat like pred, status, rounds, nclus, ncols int32 [B])."""
    import numpy as np
    _lsd_check_params(base, bits_per_step)
    V, C, var, vp, cp, x, pred, gate, llr, B = _lsd_host_inputs('lsd_gated_host', H, x, pred, gate,
                                                                llr, gated=True)
    ehat = np.empty_like(pred)
    ints = tuple(np.empty(B, np.int32) for _ in range(4))
    P32 = ctypes.POINTER(ctypes.c_int32)
    _lib.call('gnnd_lsd_gated_host', vp, cp, var.size, V, C,
              _lib.F32 if pred.dtype == np.float32 else _lib.F64, x.ctypes.data, pred.ctypes.data,
              None if llr is None else llr.ctypes.data, gate.ctypes.data_as(P32),
              _lib.OSD_BASE[base], bits_per_step, ehat.ctypes.data,
              *(a.ctypes.data_as(P32) for a in ints), B)
    return (ehat,) + ints


def bplsd_host(H, x, iters, alpha=0.75, beta=0.0, early_stop=True, base='zero', bits_per_step=1):
    """The host mirror of bplsd (gnnd_bplsd_host): numpy in, numpy out, no device.  -> (ehat,
    status, rounds, nclus, ncols, iters_used, bp_status, pred, llr)."""
    import numpy as np
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    _lsd_check_params(base, bits_per_step)
    V, C, var, chk, vp, cp = _host_graph(H)
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError(f'bplsd_host supports float32/float64, got {x.dtype}')
    B = x.size // (V + C)
    if x.size != B * (V + C):
        raise ValueError(f'x must hold B*N values (N = {V + C})')
    ehat, pred, llr = (np.empty(B * V, x.dtype) for _ in range(3))
    status, rounds, nclus, ncols, iters_used, bp_status = (np.empty(B, np.int32) for _ in range(6))
    P32 = ctypes.POINTER(ctypes.c_int32)
    _lib.call('gnnd_bplsd_host', vp, cp, var.size, V, C,
              _lib.F32 if x.dtype == np.float32 else _lib.F64, x.ctypes.data, alpha, beta, iters,
              int(bool(early_stop)), _lib.OSD_BASE[base], bits_per_step, pred.ctypes.data,
              llr.ctypes.data, iters_used.ctypes.data_as(P32), bp_status.ctypes.data_as(P32),
              ehat.ctypes.data, status.ctypes.data_as(P32), rounds.ctypes.data_as(P32),
              nclus.ctypes.data_as(P32), ncols.ctypes.data_as(P32), B)
    return ehat, status, rounds, nclus, ncols, iters_used, bp_status, pred, llr


class SyndromeLossFn(torch.autograd.Function):
    """Batch-summed syndrome loss; backward scales the kernel's d loss / d pred."""

    @staticmethod
    def forward(ctx, pred, y, graph, logical_rows, logical_only):
        loss_b, dpred = syndrome_loss(graph, logical_rows, logical_only, pred, y)
        ctx.save_for_backward(dpred)
        return loss_b.sum()

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None, None


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8,
              weight_decay=0.0):
    """In-place torch.optim.Adam update of one flat parameter buffer (gnnd_adam_step);
    `step` is a float64 device scalar tensor incremented by the call."""
    _require_gpu(param, grad, exp_avg, exp_avg_sq, step)
    for t in (grad, exp_avg, exp_avg_sq):
        if t.dtype != param.dtype or t.numel() != param.numel() or not t.is_contiguous():
            raise ValueError('adam_step: buffers must match the parameter (dtype, size, contiguous)')
    if step.dtype != torch.float64 or step.numel() != 1:
        raise ValueError('adam_step: step must be a float64 scalar tensor')
    _lib.call('gnnd_adam_step', dtype_code(param.dtype), _ptr(param), _ptr(grad), _ptr(exp_avg),
              _ptr(exp_avg_sq), _ptr(step), param.numel(), float(lr), float(betas[0]),
              float(betas[1]), float(eps), float(weight_decay), current_stream(param.device))


# ---------------------------------------------------------------------------------------
# input synthesis (gnnd_sample_*)
# ---------------------------------------------------------------------------------------
def _doubles(vals):
    vals = [float(v) for v in vals]
    return (ctypes.c_double * len(vals))(*vals), len(vals)


def sample_toric(graph, B, ps, seed=0, offset=0, dtype=torch.float64, device=None):
    """gen_syn inputs on the device (gnnd_sample_toric): x [B*N, 1], y [B*V, 1]."""
    device = device or graph.device
    x = torch.empty(B * graph.N, 1, dtype=dtype, device=device)
    y = torch.empty(B * graph.V, 1, dtype=dtype, device=device)
    _require_gpu(x)
    arr, n = _doubles(ps)
    _lib.call('gnnd_sample_toric', graph.handle, dtype_code(dtype), arr, n, int(seed) & (2**64 - 1),
              int(offset), _ptr(x), _ptr(y), int(B), current_stream(x.device))
    return x, y


def pack_generator_columns(G):
    """Generator [k, V] (0/1) -> [V, ceil(k/32)] uint32 column bit masks (int32 storage)."""
    import numpy as np
    G = np.asarray(G, dtype=np.uint8)
    k, V = G.shape
    kw = (k + 31) // 32
    cols = np.zeros((V, kw), dtype=np.uint64)
    for i in range(k):
        cols[:, i // 32] |= G[i].astype(np.uint64) << np.uint64(i % 32)
    return torch.from_numpy(cols.astype(np.uint32).view(np.int32)), k


def sample_awgn(graph, B, snrs, gen_cols=None, k=0, codeword_bit=1, seed=0, offset=0,
                dtype=torch.float32, device=None):
    """Gen_Data inputs on the device (gnnd_sample_awgn): x [B*N, 1], labels [B*V, 1].
    gen_cols: device int32 [V, ceil(k/32)] from pack_generator_columns (random codewords),
    or None for the constant word `codeword_bit`."""
    device = device or graph.device
    x = torch.empty(B * graph.N, 1, dtype=dtype, device=device)
    y = torch.empty(B * graph.V, 1, dtype=dtype, device=device)
    _require_gpu(x)
    arr, n = _doubles(snrs)
    if gen_cols is not None:
        if gen_cols.dtype != torch.int32 or not gen_cols.is_cuda or gen_cols.size(0) != graph.V:
            raise ValueError('gen_cols must be a device int32 [V, ceil(k/32)] tensor')
        gen_cols = gen_cols.contiguous()
    _lib.call('gnnd_sample_awgn', graph.handle, dtype_code(dtype), arr, n, _ptr(gen_cols), int(k),
              int(codeword_bit), int(seed) & (2**64 - 1), int(offset), _ptr(x), _ptr(y), int(B),
              current_stream(x.device))
    return x, y


def philox4x32_10(counter, key):
    """Host mirror of the device generator (known-answer tests)."""
    c = (ctypes.c_uint32 * 4)(*[int(v) & 0xffffffff for v in counter])
    kk = (ctypes.c_uint32 * 2)(*[int(v) & 0xffffffff for v in key])
    out = (ctypes.c_uint32 * 4)()
    _lib.get().gnnd_philox4x32_10(c, kk, out)
    return list(out)
