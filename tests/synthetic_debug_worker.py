"""The device side of tests/test_gpu_synthetic_graphs.py: every case of tests/synthetic_codes.py
(min-sum on both schedules, relay, OSD-0 and OSD in both bases, BP+OSD on both schedules, gated OSD
on the tall graph) through the ops, outputs as numpy arrays.  The tests call run() case by case on
the release library.  As a program (a child process with GNND_LIB pointing at libgnnd_debug.so,
test_debug_library_runs_every_case_clean) it runs every case, saves the outputs to the .npz file
named on the command line for the parent to compare with the references, and prints one JSON line
with the debug flags (gnnd_debug_flags synchronises the device and collects every translation
unit's word)."""
import sys

import numpy as np
import torch

from debug_child import report  # first: it puts the package on sys.path
import gnndecode as gd  # noqa: E402
from gnndecode import ops  # noqa: E402
import bposd_cases as bc  # noqa: E402
import minsum_cases as mc  # noqa: E402
import osd_cases as oc  # noqa: E402
import relay_cases as rc  # noqa: E402
import synthetic_codes as sc  # noqa: E402

DEV = 'cuda:0'
DTYPES = ('float32', 'float64')
BASES = ('zero', 'hard')

CASES = ([('minsum', code, B, dt, sch) for code, B in sc.MINSUM_SHAPES for dt in DTYPES
          for sch in ('flooding', 'layered')]
         + [('relay', fam, code, B, dt, pi) for fam, code, B in sc.RELAY_CASES for dt in DTYPES
            for pi in sc.RELAY_PARAMS]
         + [('osd', code, B, dt, base) for code, B in sc.OSD_SHAPES for dt in DTYPES
            for base in BASES]
         + [('bposd', code, B, dt, sch) for code, B in sc.BPOSD_SHAPES for dt in DTYPES
            for sch in ('flooding', 'layered')]
         + [('gated', 'syn_tall', 9, dt) for dt in DTYPES])

_GRAPHS = {}


def graph_of(code):
    if code not in _GRAPHS:
        _GRAPHS[code] = gd.TannerGraph(sc.matrix(code), device=DEV)
    return _GRAPHS[code]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def _np(ts):
    return tuple(t.cpu().numpy().reshape(-1) for t in ts)


def run_minsum(code, B, dtype, schedule):
    """-> (pred, llr, iters_used, status)"""
    alpha, beta, iters, early = mc.PARAMS[0]
    H, x = mc.inputs(code, B, dtype)
    return _np(ops.minsum(graph_of(code), _dev(x).unsqueeze(1), iters, alpha, beta, bool(early),
                          schedule=schedule))


def run_relay(family, code, B, dtype, pi):
    """-> (ehat, llr, iters_used, status, leg, nsol)"""
    params = legs, iters0, iters_leg, S = rc.PARAMS[pi]
    H, x = rc.inputs(family, code, B, dtype)
    g = graph_of(code)
    return _np(ops.relay(g, _dev(x).unsqueeze(1), _dev(rc.gammas(g.V, params, dtype)), iters0,
                         iters_leg, S, rc.ALPHA, rc.BETA))


def run_osd(code, B, dtype, base):
    """-> (ehat, status) of osd0, then (ehat, status, choice) of every method of OSD_METHODS"""
    H, x, p = oc.inputs(code, B, dtype)
    g = graph_of(code)
    xd, pd = _dev(x).unsqueeze(1), _dev(p).unsqueeze(1)
    out = _np(ops.osd0(g, xd, pd, base))
    for method, order in sc.OSD_METHODS:
        out += _np(ops.osd(g, xd, pd, base, method, order))
    return out


def run_bposd(code, B, dtype, schedule):
    """-> (ehat, status, choice, iters_used, bp_status, pred, llr)"""
    alpha, beta, iters, early = bc.bp_params(code)
    H, x = mc.inputs(code, B, dtype)
    return _np(ops.bposd(graph_of(code), _dev(x).unsqueeze(1), iters, alpha, beta, bool(early),
                         'zero', 'cs', 10, schedule=schedule))


def run_gated(code, B, dtype):
    """-> (ehat, status, choice) of ('cs', 10), then of ('e', 8): hard base, alternating gate"""
    H, x, p = oc.inputs(code, B, dtype)
    gate = _dev(bc.gate(code, B, dtype, 'alt'))
    out = ()
    for method, order in (('cs', 10), ('e', 8)):
        out += _np(ops.osd_gated(graph_of(code), _dev(x), _dev(p), gate, 'hard', method, order))
    return out


RUN = {'minsum': run_minsum, 'relay': run_relay, 'osd': run_osd, 'bposd': run_bposd,
       'gated': run_gated}


def run(case):
    return RUN[case[0]](*case[1:])


def key(case, j):
    return '-'.join(str(a) for a in case) + f'-out{j}'


def main():
    arrays = {}
    for case in CASES:
        for j, a in enumerate(run(case)):
            arrays[key(case, j)] = a
    np.savez(sys.argv[1], **arrays)
    report(cases=len(CASES))


if __name__ == '__main__':
    main()
