#!/usr/bin/env python3
"""What the layered schedule costs and decides beside the flooding schedule of the parent commit.
Toric-5, fp64, B = 65 536 (ops.sample_toric over the reference's p list, seed 0), T = 10, alpha
0.75, beta 0, ('cs', 10), zero base:
  ref_minsum       ops.minsum(early_stop=True) of the --ref-pkg build (the parent commit)
  layered_minsum   ops.minsum(early_stop=True, schedule='layered')
  ref_bposd        ops.bposd of the --ref-pkg build
  layered_bposd    ops.bposd(schedule='layered')
LDPC(648,324), fp32, B = 16 384 (ops.sample_awgn, the all-zero codeword, SNR 1 / 2 / 3 / 4 dB,
seed 0), T = 12:
  ref_minsum_ldpc, layered_minsum_ldpc
Each call timed alone (the method of tools/minsum_bench.py: warm-up, device events around each
call, median over the repeats, one child process per row under its own `timeout`; a row that fails
ends the run), with the status-0 count, the histogram of iters_used, the number of gated codewords
and the decision_errors counts of its estimate (pred for the min-sum rows, ehat for bposd).  Ratios
are to the parent's row, never to the code under test.  Without --ref-pkg the yardstick rows come
from this build's flooding schedule.  Writes profiles/minsum_layered_toric5_B65536_f64.json (or
--out).

usage: tools/minsum_layered_bench.py [--ref-pkg DIR] [--batch B] [--ldpc-batch B] [--repeats R]
                                     [--warmup W] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from minsum_bench import PS, timed  # noqa: E402

STEPS = ('ref_minsum', 'layered_minsum', 'ref_bposd', 'layered_bposd', 'ref_minsum_ldpc',
         'layered_minsum_ldpc')
PARENT = {'layered_minsum': 'ref_minsum', 'layered_bposd': 'ref_bposd',
          'layered_minsum_ldpc': 'ref_minsum_ldpc'}
ALPHA, BETA = 0.75, 0.0
OSD = ('zero', 'cs', 10)
LDPC_SNR = (1.0, 2.0, 3.0, 4.0)


def step(name, a):
    sys.path.insert(0, a.ref_pkg or os.path.join(ROOT, 'gnn-decode_amd'))
    import numpy as np
    import torch
    import gnndecode as gd
    from gnndecode import ops
    dev = torch.device('cuda', 0)
    ldpc = name.endswith('_ldpc')
    if ldpc:
        H = gd.codes.get_code('ldpc_648_324')
        g = gd.TannerGraph(H, device=dev)
        lg, B, iters, dt = None, a.ldpc_batch, 12, torch.float32
        x, y = ops.sample_awgn(g, B, LDPC_SNR, codeword_bit=0, seed=0, dtype=dt)
    else:
        H = gd.codes.toric_code(5)
        g = gd.TannerGraph(H, device=dev)
        lg = torch.from_numpy(gd.codes.toric_logicals(H).astype(np.int32)).to(dev)
        B, iters, dt = a.batch, 10, torch.float64
        x, y = ops.sample_toric(g, B, PS, seed=0, dtype=dt)
    # the parent's entry points have no `schedule` keyword
    kw = {'schedule': 'layered'} if name.startswith('layered') else {}

    def real():
        return torch.empty(B * g.V, 1, dtype=dt, device=dev)

    def ints():
        return torch.empty(B, dtype=torch.int32, device=dev)
    res = {'step': name, 'batch': B, 'iters': iters}
    if 'bposd' in name:
        out = (real(), ints(), ints(), ints(), ints(), real(), real())
        work = torch.empty(ops.osd_gated_workspace(B), dtype=torch.uint8, device=dev)
        res.update(timed(lambda: ops.bposd(g, x, iters, ALPHA, BETA, True, *OSD, out=out, work=work,
                                           **kw), a.warmup, a.repeats))
        est, its, bp = out[0], out[3], out[4]
        res['osd_status0'] = int(out[1].eq(0).sum())
    else:
        out = (real(), real(), ints(), ints())
        res.update(timed(lambda: ops.minsum(g, x, iters, ALPHA, BETA, True, out=out, **kw),
                         a.warmup, a.repeats))
        est, its, bp = out[0], out[2], out[3]
    hist = torch.bincount(its.to(torch.int64), minlength=iters + 1).tolist()
    res['iters_histogram'] = {str(i): n for i, n in enumerate(hist) if n}
    res['status0'] = int(bp.eq(0).sum())
    res['gated'] = int(bp.ne(0).sum())
    res['decision_errors'] = ops.decision_errors(g, lg, est, y).tolist()
    print(json.dumps(res), flush=True)


def run_step(name, a, ref_pkg=None):
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__),
           '--step', name, '--batch', str(a.batch), '--ldpc-batch', str(a.ldpc_batch), '--repeats',
           str(a.repeats), '--warmup', str(a.warmup)]
    if ref_pkg:
        cmd += ['--ref-pkg', ref_pkg]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-3000:])
        raise SystemExit(f'step {name} failed (exit {r.returncode}); nothing further started')
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--ldpc-batch', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=180, help='seconds per GPU step')
    ap.add_argument('--ref-pkg', help='built gnn-decode_amd directory of the parent commit: its '
                                      'ops.minsum and ops.bposd are the yardstick')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles',
                                                  'minsum_layered_toric5_B65536_f64.json'))
    ap.add_argument('--step', choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    ref = os.path.abspath(a.ref_pkg) if a.ref_pkg else None
    steps = {name: run_step(name, a, ref if name.startswith('ref_') else None) for name in STEPS}
    ms = {n: steps[n]['ms_median'] for n in STEPS}
    result = {
        'what': f'toric-5 fp64, B = {a.batch} (ops.sample_toric, seed 0, p uniform over {list(PS)}), '
                f'T = 10, and LDPC(648,324) fp32, B = {a.ldpc_batch} (ops.sample_awgn, all-zero '
                f'codeword, SNR {list(LDPC_SNR)} dB, seed 0), T = 12; alpha = {ALPHA}, beta = {BETA}, '
                f'early stop, osd {OSD}: ops.minsum and ops.bposd on the flooding schedule (parent) '
                f'and on the layered schedule; each call alone, device events around each call, '
                f'median of {a.repeats} after {a.warmup} warm-up calls, one process per row; 1x MI355X',
        'reference': ('ops.minsum and ops.bposd of the --ref-pkg build (the parent commit), same '
                      'machine and batch' if ref else "this build's flooding schedule"),
        'ms': ms,
        'ratio_to_parent': {n: ms[n] / ms[p] for n, p in PARENT.items()},
        'status0': {n: steps[n]['status0'] for n in STEPS},
        'gated': {n: steps[n]['gated'] for n in STEPS},
        'iters_histogram': {n: steps[n]['iters_histogram'] for n in STEPS},
        'decision_errors_fields': ['bit errors', 'codewords with a bit error',
                                   'codewords with a residual syndrome',
                                   'codewords with zero residual syndrome and a logical error'],
        'decision_errors': {n: steps[n]['decision_errors'] for n in STEPS},
        'steps': steps,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps({k: result[k] for k in ('ms', 'ratio_to_parent', 'status0', 'gated',
                                             'iters_histogram', 'decision_errors')}))


if __name__ == '__main__':
    main()
