"""The post-processing and BP decoders over the C ABI (gnndecode.ops re-exports every name here).

Each decoder's tensor interface is declared once (a `Decoder` next to its wrapper).  The shared
helpers read that declaration: `_check_inputs` (device and host), `_outputs`, `_traced` and
`_host_args`; gnndecode.library generates the gnnd:: torch ops from DECODERS.  A decoder keeps
only its docstring, its scalar-parameter check, its `_X_impl` with the one C call (the C argument
order differs from the Python return order) and the matching call of its host mirror.
"""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .graph import current_stream, dtype_code, edge_list


def _ptr(t):
    """The address of t for a void* argument of the C ABI (None: NULL), as the plain integer
    ctypes converts itself: building a c_void_p per argument cost more than the input checks."""
    return None if t is None else t.data_ptr()


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('gnndecode runs on the GPU only (HIP/gfx950); got a CPU tensor')


# ---------------------------------------------------------------------------------------
# the declaration of a decoder's tensor interface, and the helpers that read it
# ---------------------------------------------------------------------------------------
class Out(NamedTuple):
    name: str               # in the returned tuple and in `out`
    kind: str               # 'real': [B*V, 1] in the input dtype; 'int': int32 [B]
    optional: bool          # may be None in `out` (then skipped and returned as None)
    arg: str                # its argument name in the gnnd::X_out schema


class Decoder(NamedTuple):
    name: str               # ops.X, ops.X_host, ops._X_impl, gnnd::X and gnnd::X_out
    args: str               # the gnnd::X schema after graph_id: tensors and scalars in call order
    tensors: tuple          # ((name, optional), ...): the tensors of `args`.  The name fixes the
                            # form: x [B*N], pred / llr [B*V] and gammas [legs, V] in one
                            # float32/float64 dtype, gate int32 [B]
    outs: tuple             # the Outs, in the order returned
    batch: str              # the input that defines B: 'x' by N, or 'pred' by V
    ref: int                # its index in `tensors`
    zeros: bool             # gnnd::X and X_host return zeros where nothing is written (a gate's
                            # skipped rows); the eager call with out=None allocates with empty
    short_out: bool         # `out` may leave its last (optional) entry off: osd's (ehat, status)
    layered: bool           # gnnd::X_layered[_out] too: the same declaration, schedule='layered'


def _real(name, optional=False, arg=None):
    return Out(name, 'real', optional, arg or name)


def _int(name, optional=False):
    return Out(name, 'int', optional, name)


def _decoder(name, args, outs, batch='x', zeros=False, short_out=False, layered=False):
    tensors = tuple((a.split()[1], a.startswith('Tensor?')) for a in args.split(', ')
                    if a.startswith('Tensor'))
    ref = [t[0] for t in tensors].index(batch)
    return Decoder(name, args, tensors, tuple(outs), batch, ref, zeros, short_out, layered)


_REAL = ((torch.float32, torch.float64), (np.float32, np.float64))    # [host]
_I32 = (torch.int32, np.int32)
_P32 = ctypes.POINTER(ctypes.c_int32)


def _check_inputs(d, V, N, tensors, host=False):
    """The tensor inputs of decoder `d`, given in declared order -> (the same, contiguous, B).
    Device tensors (host=False) must be on the GPU and already have the declared dtypes; the
    numpy inputs of a host mirror are cast to them.  Checks the device, then every dtype, then
    every size."""
    ref = tensors[d.ref]
    if host:
        ref = np.ascontiguousarray(ref)
    else:
        for t in tensors:
            if t is not None and not t.is_cuda:
                _require_gpu(t)
    dtype = ref.dtype
    if dtype not in _REAL[host]:
        raise TypeError(f'{d.name}: {d.batch} must be float32 or float64, got {dtype}')
    i32, res, i = _I32[host], list(tensors), 0
    for name, optional in d.tensors:
        t = res[i]
        if t is None:
            if not optional:
                raise TypeError(f'{d.name}: {name} is required')
        elif host:
            res[i] = np.ascontiguousarray(t, dtype=i32 if name == 'gate' else dtype)
        elif t.dtype != (i32 if name == 'gate' else dtype):
            raise TypeError(f'{d.name}: {name} must be {i32 if name == "gate" else dtype} '
                            f'({d.batch} is {dtype}), got {t.dtype}')
        i += 1
    B = (res[d.ref].size if host else ref.numel()) // (N if d.batch == 'x' else V)
    i = 0
    for name, _ in d.tensors:
        t = res[i]
        if t is not None:
            if name != 'gammas':                    # (gammas [legs, V]: the decoder's own check)
                need = B * N if name == 'x' else B if name == 'gate' else B * V
                if (t.size if host else t.numel()) != need:
                    raise ValueError(f'{d.name}: {name} must hold {need} values (B = {B}, V = '
                                     f'{V}, N = {N}), has {t.size if host else t.numel()}')
            if not host:
                res[i] = t.contiguous()
        i += 1
    return res, B


def _new_outputs(d, ref, B, V, new=torch.empty):
    """Fresh outputs of `d` for the contiguous input `ref` that defines B: a real output has
    pred's shape where pred defines B, else [B*V, 1]."""
    shape = ref.shape if d.batch == 'pred' else (B * V, 1)
    return tuple(new(shape, dtype=ref.dtype, device=ref.device) if o.kind == 'real'
                 else new(B, dtype=torch.int32, device=ref.device) for o in d.outs)


def _out_form(d):
    return '(' + ', '.join(o.name + ('?' if o.optional else '') for o in d.outs) + ')'


def _outputs(d, out, ref, B, V):
    """`out` of an eager call -> the tuple of d's outputs: allocated (torch.empty) when None,
    else checked entry by entry: length, required entries, device, dtype, size, contiguity."""
    if out is None:
        return _new_outputs(d, ref, B, V)
    if len(out) != len(d.outs):
        if not (d.short_out and len(out) == len(d.outs) - 1):
            raise ValueError(f'{d.name}: out must be {_out_form(d)}, got {len(out)} entries')
        out = tuple(out) + (None,)
    dtype, nreal = ref.dtype, B * V
    for o, t in zip(d.outs, out):
        if t is None:
            if not o.optional:
                raise ValueError(f'{d.name}: {o.name} is required in out = {_out_form(d)}')
        elif not (t.is_cuda and t.is_contiguous()
                  and (t.dtype == dtype and t.numel() == nreal if o.kind == 'real'
                       else t.dtype == torch.int32 and t.numel() == B)):
            _require_gpu(t)
            want = f'{dtype} [{nreal}]' if o.kind == 'real' else f'int32 [{B}]'
            raise ValueError(f'{d.name}: out entry {o.name} must be contiguous {want}')
    return tuple(out)


def _traced(d, suffix, graph, args, out):
    """The traced (torch.compile / FX) form of a call: the registered op gnnd::X when `out` is
    None, else gnnd::X_out, which needs every entry of `out`."""
    if out is None:
        return getattr(torch.ops.gnnd, d.name + suffix)(graph.gid, *args)
    if len(out) != len(d.outs) or any(o is None for o in out):
        raise ValueError(f'traced {d.name} needs every entry of out = {_out_form(d)}')
    getattr(torch.ops.gnnd, d.name + suffix + '_out')(graph.gid, *args, *out)
    return out


def _host_graph(H):
    H = np.asarray(H)
    var, chk = edge_list(H)
    P64 = ctypes.POINTER(ctypes.c_int64)
    return H.shape[0], H.shape[1], var, chk, var.ctypes.data_as(P64), chk.ctypes.data_as(P64)


def _host_ptr(a):
    """The C pointer of a host array (it keeps the array alive): int32* or void*."""
    if a is None:
        return None
    return a.ctypes.data_as(_P32 if a.dtype == np.int32 else ctypes.c_void_p)


def _host_args(d, H, *tensors):
    """What a host mirror of `d` hands to its C entry point, for H [V, C] and d's tensor inputs
    -> (graph, ins, B, outs, out_ptrs): graph = (var*, chk*, E, V, C, dtype code), the leading C
    arguments; ins the pointers of the checked inputs (None for an absent one); outs the fresh
    numpy outputs in the order returned (zeros where d says so) and out_ptrs their pointers."""
    V, C, var, chk, vp, cp = _host_graph(H)
    ins, B = _check_inputs(d, V, V + C, tensors, host=True)
    ref = ins[d.ref]
    new = np.zeros if d.zeros else np.empty
    shape = ref.shape if d.batch == 'pred' else B * V
    outs = tuple(new(shape, ref.dtype) if o.kind == 'real' else new(B, np.int32) for o in d.outs)
    code = _lib.F32 if ref.dtype == np.float32 else _lib.F64
    return ((vp, cp, var.size, V, C, code), tuple(map(_host_ptr, ins)), B, outs,
            tuple(map(_host_ptr, outs)))


# ---------------------------------------------------------------------------------------
# OSD-0 post-processing (gnnd_osd0): syndrome-satisfying estimates from soft outputs
# ---------------------------------------------------------------------------------------
_OSD0 = _decoder('osd0', 'Tensor x, Tensor pred, str base', (_real('ehat'), _int('status')),
                 batch='pred')


def _osd_check_base(base):
    if base not in _lib.OSD_BASE:
        raise ValueError(f"base must be 'zero' or 'hard', got {base!r}")


def osd0(graph, x, pred, base='zero', out=None):
    """Order-0 ordered-statistics post-processing of a decoder's soft output, one HIP launch
    (gnnd_osd0): x [B*N(,1)] the decoder input (its check rows carry the syndrome), pred
    [B*V(,1)] P(bit = 1) -> (ehat, status).  ehat has pred's shape and dtype and holds exactly
    0.0 / 1.0: it satisfies the syndrome wherever status [B] (int32) is 0 and is the base vector
    where it is 1 (syndrome outside the column space of H^T).  base 'zero': solve from the zero
    vector with the columns ordered by pred (the usual quantum form); 'hard': solve for a
    correction of the hard decision pred > 0.5 with the least reliable columns first (the
    classical form).  No host sync; `out` = (ehat, status) tensors to write into."""
    _osd_check_base(base)
    if torch.compiler.is_compiling():
        return _traced(_OSD0, '', graph, (x, pred, base), out)
    (x, pred), B = _check_inputs(_OSD0, graph.V, graph.N, (x, pred))
    out = _outputs(_OSD0, out, pred, B, graph.V)
    _osd0_impl(graph, x, pred, base, *out)
    return out


def _osd0_impl(graph, x, pred, base, ehat, status):
    """gnnd::osd0 / gnnd::osd0_out implementation (gnndecode.library)."""
    _lib.call('gnnd_osd0', graph.handle, dtype_code(pred.dtype), _ptr(x), _ptr(pred),
              _lib.OSD_BASE[base], _ptr(ehat), _ptr(status), pred.numel() // graph.V,
              current_stream(pred.device))


def osd0_host(H, x, pred, base='zero'):
    """The host mirror of osd0 (gnnd_osd0_host): numpy in, numpy out, no device.  H [V, C],
    x [B*N], pred [B*V] float32 or float64 -> (ehat like pred, status int32 [B])."""
    _osd_check_base(base)
    g, (x, pred), B, outs, (ehat, status) = _host_args(_OSD0, H, x, pred)
    _lib.call('gnnd_osd0_host', *g, x, pred, _lib.OSD_BASE[base], ehat, status, B)
    return outs


# ---------------------------------------------------------------------------------------
# higher-order OSD post-processing (gnnd_osd): the lightest of the combination-sweep or
# exhaustive candidates on top of OSD-0
# ---------------------------------------------------------------------------------------
_OSD = _decoder('osd', 'Tensor x, Tensor pred, str base, str method, SymInt order',
                (_real('ehat'), _int('status'), _int('choice', True)), batch='pred',
                short_out=True)


def _osd_check_method(base, method, order):
    _osd_check_base(base)
    if method not in _lib.OSD_METHOD:
        raise ValueError(f"method must be 'osd0', 'cs' or 'e', got {method!r}")
    limit = {'osd0': 2 ** 31 - 1, 'cs': 64, 'e': 12}[method]
    if not isinstance(order, int) or not 0 <= order <= limit:
        raise ValueError(f'order must be an integer in [0, {limit}] for method {method!r}, '
                         f'got {order!r}')


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
        return _traced(_OSD, '', graph, (x, pred, base, method, order), out)
    (x, pred), B = _check_inputs(_OSD, graph.V, graph.N, (x, pred))
    out = _outputs(_OSD, out, pred, B, graph.V)
    _osd_impl(graph, x, pred, base, method, order, *out)
    return out


def _osd_impl(graph, x, pred, base, method, order, ehat, status, choice):
    """gnnd::osd / gnnd::osd_out implementation (gnndecode.library)."""
    _lib.call('gnnd_osd', graph.handle, dtype_code(pred.dtype), _ptr(x), _ptr(pred),
              _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order, _ptr(ehat), _ptr(status),
              _ptr(choice), pred.numel() // graph.V, current_stream(pred.device))


def osd_host(H, x, pred, base='zero', method='cs', order=10):
    """The host mirror of osd (gnnd_osd_host): numpy in, numpy out, no device.  H [V, C], x [B*N],
    pred [B*V] float32 or float64 -> (ehat like pred, status int32 [B], choice int32 [B])."""
    _osd_check_method(base, method, order)
    g, (x, pred), B, outs, (ehat, status, choice) = _host_args(_OSD, H, x, pred)
    _lib.call('gnnd_osd_host', *g, x, pred, _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order,
              ehat, status, choice, B)
    return outs


# ---------------------------------------------------------------------------------------
# min-sum BP with the syndrome-converged early stop (gnnd_minsum)
# ---------------------------------------------------------------------------------------
_MINSUM_ARGS = 'Tensor x, SymInt iters, float alpha, float beta, bool early_stop'
_MINSUM = _decoder('minsum', _MINSUM_ARGS,
                   (_real('pred'), _real('llr', True), _int('iters_used', True),
                    _int('status', True)), layered=True)


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
    the posteriors the layers before it just updated; both defined in include/gnnd.h):
    x [B*N(,1)] the decoder input (priors at the variable rows, the syndrome at the check rows
    as for osd0) -> (pred, llr, iters_used, status).  Check messages
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
        return _traced(_MINSUM, suffix, graph, (x, iters, alpha, beta, early_stop), out)
    (x,), B = _check_inputs(_MINSUM, graph.V, graph.N, (x,))
    out = _outputs(_MINSUM, out, x, B, graph.V)
    _minsum_impl(graph, x, iters, alpha, beta, early_stop, *out, schedule=schedule)
    return out


def _minsum_impl(graph, x, iters, alpha, beta, early_stop, pred, llr, iters_used, status,
                 schedule='flooding'):
    """gnnd::minsum[_layered] / gnnd::minsum[_layered]_out implementation (gnndecode.library)."""
    _lib.call('gnnd_minsum' + _schedule_suffix(schedule), graph.handle, dtype_code(x.dtype),
              _ptr(x), alpha, beta, iters, int(early_stop), _ptr(pred), _ptr(llr),
              _ptr(iters_used), _ptr(status), x.numel() // graph.N, current_stream(x.device))


def minsum_host(H, x, iters, alpha=0.75, beta=0.0, early_stop=True, schedule='flooding'):
    """The host mirror of minsum (gnnd_minsum_host, gnnd_minsum_layered_host with
    schedule='layered'): numpy in, numpy out, no device.  H [V, C], x [B*N] float32 or float64
    -> (pred, llr like x's dtype [B*V], iters_used, status int32 [B])."""
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    suffix = _schedule_suffix(schedule)
    g, (x,), B, outs, (pred, llr, iters_used, status) = _host_args(_MINSUM, H, x)
    _lib.call(f'gnnd_minsum{suffix}_host', *g, x, alpha, beta, iters, int(bool(early_stop)), pred,
              llr, iters_used, status, B)
    return outs


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
    V, C, var, chk, vp, cp = _host_graph(H)
    n = ctypes.c_int32()
    layer = np.empty(C, np.int32)
    _lib.call('gnnd_graph_layers_host', vp, cp, var.size, V, C, ctypes.byref(n),
              layer.ctypes.data_as(_P32))
    assert C == 0 or int(layer.max()) + 1 == n.value
    return layer


# ---------------------------------------------------------------------------------------
# relay min-sum BP: memory-strength legs that keep the lightest solution (gnnd_relay)
# ---------------------------------------------------------------------------------------
_RELAY_ARGS = ('Tensor x, Tensor gammas, SymInt iters0, SymInt iters_leg, SymInt stop_after, '
               'float alpha, float beta')
_RELAY = _decoder('relay', _RELAY_ARGS,
                  (_real('ehat'), _real('llr', True), _int('iters_used', True),
                   _int('status', True), _int('leg', True), _int('nsol', True)))


def _relay_check_params(V, gammas, iters0, iters_leg, stop_after, alpha, beta):
    """-> (legs, iters_leg, alpha, beta) of gammas [legs, V] (a tensor or an array)."""
    if gammas.ndim != 2 or gammas.shape[1] != V:
        raise ValueError(f'gammas must be [legs, V] (V = {V})')
    legs = gammas.shape[0]
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
    return legs, iters_leg, alpha, beta


def relay_gammas(V, legs, gamma0=0.125, center=0.21, width=0.9, seed=0, dtype=torch.float64,
                 device=None):
    """The usual relay memory strengths, [legs, V] in `dtype`: row 0 is `gamma0` on every variable,
    the later rows are numpy.random.default_rng(seed).uniform(center - width / 2, center + width /
    2, (legs - 1, V)) (disordered, partly negative), drawn in float64 and cast to `dtype`."""
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
    _, iters_leg, alpha, beta = _relay_check_params(graph.V, gammas, iters0, iters_leg,
                                                    stop_after, alpha, beta)
    if torch.compiler.is_compiling():
        return _traced(_RELAY, '', graph,
                       (x, gammas, iters0, iters_leg, stop_after, alpha, beta), out)
    (x, gammas), B = _check_inputs(_RELAY, graph.V, graph.N, (x, gammas))
    out = _outputs(_RELAY, out, x, B, graph.V)
    _relay_impl(graph, x, gammas, iters0, iters_leg, stop_after, alpha, beta, *out)
    return out


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
    legs, iters_leg, alpha, beta = _relay_check_params(np.shape(H)[0], np.asarray(gammas), iters0,
                                                       iters_leg, stop_after, alpha, beta)
    g, (x, gammas), B, outs, (ehat, llr, iters_used, status, leg, nsol) = _host_args(
        _RELAY, H, x, gammas)
    _lib.call('gnnd_relay_host', *g, x, gammas, legs, iters0, iters_leg, stop_after, alpha, beta,
              ehat, llr, iters_used, status, leg, nsol, B)
    return outs


# ---------------------------------------------------------------------------------------
# relay with a soft output (gnnd_relay_soft) and the one-call relay+OSD decoder (gnnd_relay_osd)
# ---------------------------------------------------------------------------------------
_RELAY_SOFT = _decoder('relay_soft', _RELAY_ARGS + ', str soft',
                       (_real('pred'), _real('soft', True, 'soft_out'), _real('ehat'),
                        _real('llr', True), _int('iters_used', True), _int('status', True),
                        _int('leg', True), _int('nsol', True)))
_RELAY_OSD = _decoder('relay_osd',
                      _RELAY_ARGS + ', str soft, str base, str method, SymInt order',
                      (_real('ehat'), _int('status'), _int('choice', True), _real('pred'),
                       _real('llr'), _int('iters_used', True), _int('relay_status'),
                       _int('leg', True), _int('nsol', True)))


def _relay_check_soft(soft):
    if soft not in _lib.RELAY_SOFT:
        raise ValueError(f"soft must be 'last' or 'mean', got {soft!r}")


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
    _, iters_leg, alpha, beta = _relay_check_params(graph.V, gammas, iters0, iters_leg,
                                                    stop_after, alpha, beta)
    _relay_check_soft(soft)
    if torch.compiler.is_compiling():
        return _traced(_RELAY_SOFT, '', graph,
                       (x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft), out)
    (x, gammas), B = _check_inputs(_RELAY_SOFT, graph.V, graph.N, (x, gammas))
    out = _outputs(_RELAY_SOFT, out, x, B, graph.V)
    _relay_soft_impl(graph, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft, *out)
    return out


def _relay_soft_impl(graph, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft, pred,
                     soft_out, ehat, llr, iters_used, status, leg, nsol):
    """gnnd::relay_soft / gnnd::relay_soft_out implementation (gnndecode.library)."""
    _lib.call('gnnd_relay_soft', graph.handle, dtype_code(x.dtype), _ptr(x), _ptr(gammas),
              gammas.shape[0], iters0, iters_leg, stop_after, alpha, beta, _lib.RELAY_SOFT[soft],
              _ptr(pred), _ptr(soft_out), _ptr(ehat), _ptr(llr), _ptr(iters_used), _ptr(status),
              _ptr(leg), _ptr(nsol), x.numel() // graph.N, current_stream(x.device))


def relay_soft_host(H, x, gammas, iters0, iters_leg=None, stop_after=1, alpha=0.75, beta=0.0,
                    soft='last'):
    """The host mirror of relay_soft (gnnd_relay_soft_host): numpy in, numpy out, no device.
    -> (pred, soft, ehat, llr like x's dtype [B*V], iters_used, status, leg, nsol int32 [B])."""
    legs, iters_leg, alpha, beta = _relay_check_params(np.shape(H)[0], np.asarray(gammas), iters0,
                                                       iters_leg, stop_after, alpha, beta)
    _relay_check_soft(soft)
    g, (x, gammas), B, outs, out_ptrs = _host_args(_RELAY_SOFT, H, x, gammas)
    _lib.call('gnnd_relay_soft_host', *g, x, gammas, legs, iters0, iters_leg, stop_after, alpha,
              beta, _lib.RELAY_SOFT[soft], *out_ptrs, B)
    return outs


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
    _, iters_leg, alpha, beta = _relay_check_params(graph.V, gammas, iters0, iters_leg,
                                                    stop_after, alpha, beta)
    _relay_check_soft(soft)
    _osd_check_method(base, method, order)
    if torch.compiler.is_compiling():
        return _traced(_RELAY_OSD, '', graph, (x, gammas, iters0, iters_leg, stop_after, alpha,
                                               beta, soft, base, method, order), out)
    (x, gammas), B = _check_inputs(_RELAY_OSD, graph.V, graph.N, (x, gammas))
    out = _outputs(_RELAY_OSD, out, x, B, graph.V)
    _relay_osd_impl(graph, x, gammas, iters0, iters_leg, stop_after, alpha, beta, soft, base,
                    method, order, *out, work=work)
    return out


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


def relay_osd_host(H, x, gammas, iters0, iters_leg=None, stop_after=1, alpha=0.75, beta=0.0,
                   soft='last', base='zero', method='cs', order=10):
    """The host mirror of relay_osd (gnnd_relay_osd_host): numpy in, numpy out, no device.
    -> (ehat, status, choice, pred, llr, iters_used, relay_status, leg, nsol)."""
    legs, iters_leg, alpha, beta = _relay_check_params(np.shape(H)[0], np.asarray(gammas), iters0,
                                                       iters_leg, stop_after, alpha, beta)
    _relay_check_soft(soft)
    _osd_check_method(base, method, order)
    g, (x, gammas), B, outs, out_ptrs = _host_args(_RELAY_OSD, H, x, gammas)
    ehat, status, choice, pred, llr, iters_used, relay_status, leg, nsol = out_ptrs
    _lib.call('gnnd_relay_osd_host', *g, x, gammas, legs, iters0, iters_leg, stop_after, alpha,
              beta, _lib.RELAY_SOFT[soft], _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order,
              pred, llr, iters_used, relay_status, leg, nsol, ehat, status, choice, B)
    return outs


# ---------------------------------------------------------------------------------------
# min-sum BP with guided decimation: freeze bits between BP rounds (gnnd_bpgd)
# ---------------------------------------------------------------------------------------
_BPGD = _decoder('bpgd', 'Tensor x, SymInt iters0, SymInt iters_round, SymInt rounds, '
                 'SymInt per_round, str pick, float clamp, float alpha, float beta',
                 (_real('ehat'), _real('llr', True), _real('pred', True), _int('iters_used', True),
                  _int('status', True), _int('ndec', True)))


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
        return _traced(_BPGD, '', graph, (x, iters0, iters_round, rounds, per_round, pick, clamp,
                                          alpha, beta), out)
    (x,), B = _check_inputs(_BPGD, graph.V, graph.N, (x,))
    out = _outputs(_BPGD, out, x, B, graph.V)
    _bpgd_impl(graph, x, iters0, iters_round, rounds, per_round, pick, clamp, alpha, beta, *out)
    return out


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
    clamp, alpha, beta = _bpgd_check_params(iters0, iters_round, rounds, per_round, pick, clamp,
                                            alpha, beta)
    g, (x,), B, outs, out_ptrs = _host_args(_BPGD, H, x)
    _lib.call('gnnd_bpgd_host', *g, x, alpha, beta, iters0, iters_round, rounds, per_round,
              _lib.BPGD_PICK[pick], clamp, *out_ptrs, B)
    return outs


# ---------------------------------------------------------------------------------------
# union-find decoding of a matchable code: grow, merge, peel (gnnd_uf)
# ---------------------------------------------------------------------------------------
_UF = _decoder('uf', 'Tensor x, Tensor? gate',
               (_real('ehat'), _int('rounds', True), _int('status', True), _int('nfull', True)),
               zeros=True)


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
        return _traced(_UF, '', graph, (x, gate), out)
    (x, gate), B = _check_inputs(_UF, graph.V, graph.N, (x, gate))
    out = _outputs(_UF, out, x, B, graph.V)
    _uf_impl(graph, x, gate, *out)
    return out


def _uf_impl(graph, x, gate, ehat, rounds, status, nfull):
    """gnnd::uf / gnnd::uf_out implementation (gnndecode.library)."""
    _lib.call('gnnd_uf', graph.handle, dtype_code(x.dtype), _ptr(x), _ptr(gate), _ptr(ehat),
              _ptr(rounds), _ptr(status), _ptr(nfull), x.numel() // graph.N,
              current_stream(x.device))


def uf_host(H, x, gate=None):
    """The host mirror of uf (gnnd_uf_host): numpy in, numpy out, no device.  H [V, C], x [B*N]
    float32 or float64, gate [B] int32 or None -> (ehat like x's dtype [B*V], rounds, status, nfull
    int32 [B]).  The rows a gate skips are returned as zeros."""
    g, (x, gate), B, outs, out_ptrs = _host_args(_UF, H, x, gate)
    _lib.call('gnnd_uf_host', *g, x, gate, *out_ptrs, B)
    return outs


def matching_host(H):
    """The decoding graph of H [V, C] on the host (gnnd_graph_matching_host) -> (N, endpoints
    int32 [V, 2]), as TannerGraph.matching gives it."""
    V, C, var, chk, vp, cp = _host_graph(H)
    n = ctypes.c_int32()
    ends = np.empty((V, 2), np.int32)
    _lib.call('gnnd_graph_matching_host', vp, cp, var.size, V, C, ctypes.byref(n),
              ends.ctypes.data_as(_P32))
    return int(n.value), ends


# ---------------------------------------------------------------------------------------
# weighted union-find (gnnd_ufw) and the one-call belief-find decoder (gnnd_belief_find)
# ---------------------------------------------------------------------------------------
UFW_MAX_WEIGHT = 1024     # kGnndUfwMaxWeight

_UFW = _decoder('ufw', 'Tensor x, Tensor? llr, float scale, SymInt wmax, Tensor? gate, '
                'bool passthrough',
                (_real('ehat'), _int('rounds', True), _int('status', True), _int('nfull', True),
                 _int('events', True)), zeros=True)
_BELIEF_FIND = _decoder('belief_find', _MINSUM_ARGS + ', float scale, SymInt wmax',
                        (_real('ehat'), _int('status', True), _int('iters_used', True),
                         _int('bp_status'), _real('pred'), _real('llr'), _int('rounds', True),
                         _int('nfull', True), _int('events', True)))


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
        return _traced(_UFW, '', graph, (x, llr, scale, wmax, gate, passthrough), out)
    (x, llr, gate), B = _check_inputs(_UFW, graph.V, graph.N, (x, llr, gate))
    out = _outputs(_UFW, out, x, B, graph.V)
    _ufw_impl(graph, x, llr, scale, wmax, gate, passthrough, *out)
    return out


def _ufw_impl(graph, x, llr, scale, wmax, gate, passthrough, ehat, rounds, status, nfull, events):
    """gnnd::ufw / gnnd::ufw_out implementation (gnndecode.library)."""
    _lib.call('gnnd_ufw', graph.handle, dtype_code(x.dtype), _ptr(x), _ptr(llr), scale, wmax,
              _ptr(gate), int(passthrough), _ptr(ehat), _ptr(rounds), _ptr(status), _ptr(nfull),
              _ptr(events), x.numel() // graph.N, current_stream(x.device))


def ufw_host(H, x, llr=None, scale=2.0, wmax=32, gate=None, passthrough=False):
    """The host mirror of ufw (gnnd_ufw_host): numpy in, numpy out, no device.  H [V, C], x [B*N]
    float32 or float64, llr [B*V] or None, gate [B] int32 or None -> (ehat like x's dtype [B*V],
    rounds, status, nfull, events int32 [B]).  The rows a gate skips are returned as zeros."""
    scale = _ufw_check_params(scale, wmax)
    if passthrough and (gate is None or llr is None):
        raise ValueError('passthrough needs gate and llr')
    g, (x, llr, gate), B, outs, out_ptrs = _host_args(_UFW, H, x, llr, gate)
    _lib.call('gnnd_ufw_host', *g, x, llr, scale, wmax, gate, int(bool(passthrough)), *out_ptrs, B)
    return outs


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
        return _traced(_BELIEF_FIND, '', graph,
                       (x, iters, alpha, beta, early_stop, scale, wmax), out)
    (x,), B = _check_inputs(_BELIEF_FIND, graph.V, graph.N, (x,))
    out = _outputs(_BELIEF_FIND, out, x, B, graph.V)
    _belief_find_impl(graph, x, iters, alpha, beta, early_stop, scale, wmax, *out)
    return out


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
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    scale = _ufw_check_params(scale, wmax)
    g, (x,), B, outs, out_ptrs = _host_args(_BELIEF_FIND, H, x)
    ehat, status, iters_used, bp_status, pred, llr, rounds, nfull, events = out_ptrs
    _lib.call('gnnd_belief_find_host', *g, x, alpha, beta, iters, int(bool(early_stop)), scale,
              wmax, pred, llr, iters_used, bp_status, ehat, status, rounds, nfull, events, B)
    return outs


# ---------------------------------------------------------------------------------------
# gated OSD (gnnd_osd_gated) and the one-call BP+OSD decoder (gnnd_bposd)
# ---------------------------------------------------------------------------------------
_OSD_GATED = _decoder('osd_gated', 'Tensor x, Tensor pred, Tensor gate, str base, str method, '
                      'SymInt order, Tensor? llr',
                      (_real('ehat'), _int('status'), _int('choice', True)), batch='pred',
                      short_out=True)
_BPOSD = _decoder('bposd', _MINSUM_ARGS + ', str base, str method, SymInt order',
                  (_real('ehat'), _int('status'), _int('choice', True), _int('iters_used', True),
                   _int('bp_status'), _real('pred'), _real('llr')), layered=True)


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
        return _traced(_OSD_GATED, '', graph, (x, pred, gate, base, method, order, llr), out)
    (x, pred, gate, llr), B = _check_inputs(_OSD_GATED, graph.V, graph.N, (x, pred, gate, llr))
    out = _outputs(_OSD_GATED, out, pred, B, graph.V)
    _osd_gated_impl(graph, x, pred, gate, base, method, order, llr, *out, work=work)
    return out


def _osd_gated_impl(graph, x, pred, gate, base, method, order, llr, ehat, status, choice,
                    work=None):
    """gnnd::osd_gated / gnnd::osd_gated_out implementation (gnndecode.library)."""
    B = pred.numel() // graph.V
    work, nbytes = _gated_work(work, B, pred.device)
    _lib.call('gnnd_osd_gated', graph.handle, dtype_code(pred.dtype), _ptr(x), _ptr(pred),
              _ptr(llr), _ptr(gate), _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order,
              _ptr(ehat), _ptr(status), _ptr(choice), _ptr(work), nbytes, B,
              current_stream(pred.device))


def osd_gated_host(H, x, pred, gate, base='zero', method='cs', order=10, llr=None):
    """The host mirror of osd_gated (gnnd_osd_gated_host): numpy in, numpy out, no device.
    -> (ehat like pred, status int32 [B], choice int32 [B])."""
    _osd_check_method(base, method, order)
    g, (x, pred, gate, llr), B, outs, out_ptrs = _host_args(_OSD_GATED, H, x, pred, gate, llr)
    _lib.call('gnnd_osd_gated_host', *g, x, pred, llr, gate, _lib.OSD_BASE[base],
              _lib.OSD_METHOD[method], order, *out_ptrs, B)
    return outs


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
        return _traced(_BPOSD, suffix, graph,
                       (x, iters, alpha, beta, early_stop, base, method, order), out)
    (x,), B = _check_inputs(_BPOSD, graph.V, graph.N, (x,))
    out = _outputs(_BPOSD, out, x, B, graph.V)
    _bposd_impl(graph, x, iters, alpha, beta, early_stop, base, method, order, *out, work=work,
                schedule=schedule)
    return out


def _bposd_impl(graph, x, iters, alpha, beta, early_stop, base, method, order, ehat, status, choice,
                iters_used, bp_status, pred, llr, work=None, schedule='flooding'):
    """gnnd::bposd[_layered] / gnnd::bposd[_layered]_out implementation (gnndecode.library)."""
    B = x.numel() // graph.N
    work, nbytes = _gated_work(work, B, x.device)
    _lib.call('gnnd_bposd' + _schedule_suffix(schedule), graph.handle, dtype_code(x.dtype),
              _ptr(x), alpha, beta, iters, int(early_stop), _lib.OSD_BASE[base],
              _lib.OSD_METHOD[method], order, _ptr(pred), _ptr(llr), _ptr(iters_used),
              _ptr(bp_status), _ptr(ehat), _ptr(status), _ptr(choice), _ptr(work), nbytes, B,
              current_stream(x.device))


def bposd_host(H, x, iters, alpha=0.75, beta=0.0, early_stop=True, base='zero', method='cs',
               order=10, schedule='flooding'):
    """The host mirror of bposd (gnnd_bposd_host, gnnd_bposd_layered_host with
    schedule='layered'): numpy in, numpy out, no device.  -> (ehat, status, choice, iters_used,
    bp_status, pred, llr)."""
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    suffix = _schedule_suffix(schedule)
    _osd_check_method(base, method, order)
    g, (x,), B, outs, out_ptrs = _host_args(_BPOSD, H, x)
    ehat, status, choice, iters_used, bp_status, pred, llr = out_ptrs
    _lib.call(f'gnnd_bposd{suffix}_host', *g, x, alpha, beta, iters, int(bool(early_stop)),
              _lib.OSD_BASE[base], _lib.OSD_METHOD[method], order, pred, llr, iters_used,
              bp_status, ehat, status, choice, B)
    return outs


# ---------------------------------------------------------------------------------------
# localized-statistics decoding (gnnd_lsd, gnnd_lsd_gated) and the one-call BP+LSD decoder
# (gnnd_bplsd)
# ---------------------------------------------------------------------------------------
_LSD_OUTS = (_real('ehat'), _int('status', True), _int('rounds', True), _int('nclus', True),
             _int('ncols', True))
_LSD = _decoder('lsd', 'Tensor x, Tensor pred, str base, SymInt bits_per_step', _LSD_OUTS,
                batch='pred')
_LSD_GATED = _decoder('lsd_gated', 'Tensor x, Tensor pred, Tensor gate, str base, '
                      'SymInt bits_per_step, Tensor? llr', _LSD_OUTS, batch='pred')
_BPLSD = _decoder('bplsd', _MINSUM_ARGS + ', str base, SymInt bits_per_step',
                  _LSD_OUTS + (_int('iters_used', True), _int('bp_status'), _real('pred'),
                               _real('llr')))


def _lsd_check_params(base, bits_per_step):
    _osd_check_base(base)
    if (not isinstance(bits_per_step, int) or isinstance(bits_per_step, bool)
            or not 0 <= bits_per_step <= 2 ** 31 - 1):
        raise ValueError('bits_per_step must be an integer in [0, 2^31 - 1], got '
                         f'{bits_per_step!r}')


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
        return _traced(_LSD, '', graph, (x, pred, base, bits_per_step), out)
    (x, pred), B = _check_inputs(_LSD, graph.V, graph.N, (x, pred))
    out = _outputs(_LSD, out, pred, B, graph.V)
    _lsd_impl(graph, x, pred, base, bits_per_step, *out)
    return out


def _lsd_impl(graph, x, pred, base, bits_per_step, ehat, status, rounds, nclus, ncols):
    """gnnd::lsd / gnnd::lsd_out implementation (gnndecode.library)."""
    _lib.call('gnnd_lsd', graph.handle, dtype_code(pred.dtype), _ptr(x), _ptr(pred),
              _lib.OSD_BASE[base], bits_per_step, _ptr(ehat), _ptr(status), _ptr(rounds),
              _ptr(nclus), _ptr(ncols), pred.numel() // graph.V, current_stream(pred.device))


def lsd_host(H, x, pred, base='zero', bits_per_step=1):
    """The host mirror of lsd (gnnd_lsd_host): numpy in, numpy out, no device.  H [V, C], x [B*N],
    pred [B*V] float32 or float64 -> (ehat like pred, status, rounds, nclus, ncols int32 [B])."""
    _lsd_check_params(base, bits_per_step)
    g, (x, pred), B, outs, out_ptrs = _host_args(_LSD, H, x, pred)
    _lib.call('gnnd_lsd_host', *g, x, pred, _lib.OSD_BASE[base], bits_per_step, *out_ptrs, B)
    return outs


def lsd_gated(graph, x, pred, gate, base='zero', bits_per_step=1, llr=None, out=None, work=None):
    """lsd on the codewords a gate selects (gnnd_lsd_gated): gate, llr, the pass-through rule, the
    two launches and `work` as for osd_gated.  Where gate != 0 the five outputs are bit for bit
    lsd's; a pass-through codeword gets its hard decision and status = rounds = nclus = ncols =
    0.  -> (ehat, status, rounds, nclus, ncols); `out` as for lsd."""
    _lsd_check_params(base, bits_per_step)
    if torch.compiler.is_compiling():
        return _traced(_LSD_GATED, '', graph, (x, pred, gate, base, bits_per_step, llr), out)
    (x, pred, gate, llr), B = _check_inputs(_LSD_GATED, graph.V, graph.N, (x, pred, gate, llr))
    out = _outputs(_LSD_GATED, out, pred, B, graph.V)
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


def lsd_gated_host(H, x, pred, gate, base='zero', bits_per_step=1, llr=None):
    """The host mirror of lsd_gated (gnnd_lsd_gated_host): numpy in, numpy out, no device.
    -> (ehat like pred, status, rounds, nclus, ncols int32 [B])."""
    _lsd_check_params(base, bits_per_step)
    g, (x, pred, gate, llr), B, outs, out_ptrs = _host_args(_LSD_GATED, H, x, pred, gate, llr)
    _lib.call('gnnd_lsd_gated_host', *g, x, pred, llr, gate, _lib.OSD_BASE[base], bits_per_step,
              *out_ptrs, B)
    return outs


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
        return _traced(_BPLSD, '', graph,
                       (x, iters, alpha, beta, early_stop, base, bits_per_step), out)
    (x,), B = _check_inputs(_BPLSD, graph.V, graph.N, (x,))
    out = _outputs(_BPLSD, out, x, B, graph.V)
    _bplsd_impl(graph, x, iters, alpha, beta, early_stop, base, bits_per_step, *out, work=work)
    return out


def _bplsd_impl(graph, x, iters, alpha, beta, early_stop, base, bits_per_step, ehat, status,
                rounds, nclus, ncols, iters_used, bp_status, pred, llr, work=None):
    """gnnd::bplsd / gnnd::bplsd_out implementation (gnndecode.library)."""
    B = x.numel() // graph.N
    work, nbytes = _gated_work(work, B, x.device)
    _lib.call('gnnd_bplsd', graph.handle, dtype_code(x.dtype), _ptr(x), alpha, beta, iters,
              int(early_stop), _lib.OSD_BASE[base], bits_per_step, _ptr(pred), _ptr(llr),
              _ptr(iters_used), _ptr(bp_status), _ptr(ehat), _ptr(status), _ptr(rounds),
              _ptr(nclus), _ptr(ncols), _ptr(work), nbytes, B, current_stream(x.device))


def bplsd_host(H, x, iters, alpha=0.75, beta=0.0, early_stop=True, base='zero', bits_per_step=1):
    """The host mirror of bplsd (gnnd_bplsd_host): numpy in, numpy out, no device.  -> (ehat,
    status, rounds, nclus, ncols, iters_used, bp_status, pred, llr)."""
    alpha, beta = _minsum_check_params(iters, alpha, beta)
    _lsd_check_params(base, bits_per_step)
    g, (x,), B, outs, out_ptrs = _host_args(_BPLSD, H, x)
    ehat, status, rounds, nclus, ncols, iters_used, bp_status, pred, llr = out_ptrs
    _lib.call('gnnd_bplsd_host', *g, x, alpha, beta, iters, int(bool(early_stop)),
              _lib.OSD_BASE[base], bits_per_step, pred, llr, iters_used, bp_status, ehat, status,
              rounds, nclus, ncols, B)
    return outs


# every declaration: gnndecode.library registers gnnd::X and gnnd::X_out for each
DECODERS = (_OSD0, _OSD, _MINSUM, _OSD_GATED, _BPOSD, _RELAY, _RELAY_SOFT, _RELAY_OSD, _BPGD, _UF,
            _UFW, _BELIEF_FIND, _LSD, _LSD_GATED, _BPLSD)
