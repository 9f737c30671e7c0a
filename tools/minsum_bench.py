#!/usr/bin/env python3
"""What min-sum BP costs and decides beside the sum-product decode it stands next to: toric-5,
fp64, B = 65 536 (ops.sample_toric over the reference's p list, seed 0), T = 10:
  qbp            ops.decode('qbp', 10), of the --ref-pkg build (the parent commit) when given
  minsum_full    ops.minsum(10, early_stop=False)
  minsum_early   ops.minsum(10, early_stop=True)
  <decode>+osd   ops.osd('cs', 10) on that decode's pred
each call timed alone (warm-up, device events around each call, median over the repeats), with its
decision_errors counts, the histogram of iters_used and the number of codewords with status 0 (for
qbp: the codewords without a residual syndrome; it reports no status and always runs T iterations).
Every GPU step is a child process under its own `timeout`; a step that fails ends the run.
Writes profiles/minsum_toric5_B65536_f64.json (or --out).

usage: tools/minsum_bench.py [--ref-pkg DIR] [--batch B] [--repeats R] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = (0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.1)   # quantum/error_generate.py:252-260
DECODES = ('qbp', 'minsum_full', 'minsum_early')
STEPS = DECODES + tuple(d + '+osd' for d in DECODES)
ITERS = 10
ALPHA, BETA = 0.75, 0.0


def timed(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'ms_median': statistics.median(ms), 'ms_min': min(ms), 'ms_max': max(ms),
            'repeats': repeats, 'warmup': warmup}


def step(name, a):
    sys.path.insert(0, a.ref_pkg or os.path.join(ROOT, 'gnn-decode_amd'))
    import numpy as np
    import torch
    import gnndecode as gd
    from gnndecode import ops
    dev = torch.device('cuda', 0)
    H = gd.codes.toric_code(5)
    g = gd.TannerGraph(H, device=dev)
    lg = torch.from_numpy(gd.codes.toric_logicals(H).astype(np.int32)).to(dev)
    B = a.batch
    x, y = ops.sample_toric(g, B, PS, seed=0, dtype=torch.float64)
    pred = torch.empty(B * g.V, 1, dtype=torch.float64, device=dev)
    decode_name = name.split('+')[0]
    if decode_name == 'qbp':
        ms_out = None

        def decode():
            ops.decode(g, 'qbp', x, ITERS, out=pred)
    else:
        ms_out = (pred, torch.empty_like(pred), torch.empty(B, dtype=torch.int32, device=dev),
                  torch.empty(B, dtype=torch.int32, device=dev))
        early = decode_name == 'minsum_early'

        def decode():
            ops.minsum(g, x, ITERS, ALPHA, BETA, early, out=ms_out)
    decode()
    res = {'step': name}
    if name.endswith('+osd'):
        out = (torch.empty_like(pred), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev))
        res.update(timed(lambda: ops.osd(g, x, pred, 'zero', 'cs', 10, out=out), a.warmup, a.repeats))
        res['decision_errors'] = ops.decision_errors(g, lg, out[0], y).tolist()
        res['status0'] = int(out[1].eq(0).sum())
    else:
        res.update(timed(decode, a.warmup, a.repeats))
        res['decision_errors'] = ops.decision_errors(g, lg, pred, y).tolist()
        if ms_out is None:
            res['iters_histogram'] = {str(ITERS): B}
            res['status0'] = B - res['decision_errors'][2]
        else:
            hist = torch.bincount(ms_out[2].to(torch.int64), minlength=ITERS + 1).tolist()
            res['iters_histogram'] = {str(i): n for i, n in enumerate(hist) if n}
            res['status0'] = int(ms_out[3].eq(0).sum())
    print(json.dumps(res), flush=True)


def run_step(name, a, ref_pkg=None):
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__),
           '--step', name, '--batch', str(a.batch), '--repeats', str(a.repeats), '--warmup',
           str(a.warmup)]
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
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=180, help='seconds per GPU step')
    ap.add_argument('--ref-pkg', help='built gnn-decode_amd directory of the parent commit: its '
                                      "ops.decode('qbp') (and ops.osd behind it) is the yardstick")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'minsum_toric5_B65536_f64.json'))
    ap.add_argument('--step', choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    ref = os.path.abspath(a.ref_pkg) if a.ref_pkg else None
    steps = {name: run_step(name, a, ref if name.startswith('qbp') else None) for name in STEPS}
    qbp = steps['qbp']['ms_median']
    ms = {n: steps[n]['ms_median'] for n in STEPS}
    pipeline = {d: ms[d] + ms[d + '+osd'] for d in DECODES}
    result = {
        'what': f'toric-5 fp64, B = {a.batch} (ops.sample_toric, seed 0, p uniform over {list(PS)}), '
                f"T = {ITERS}: ops.decode('qbp'), ops.minsum(alpha = {ALPHA}, beta = {BETA}) without "
                f"and with early stop, and ops.osd('cs', 10) on each decode's pred; each call alone, "
                f'device events around each call, median of {a.repeats} after {a.warmup} warm-up '
                f'calls, one process per step; 1x MI355X',
        'reference': ("ops.decode('qbp') of the --ref-pkg build (the parent commit), same machine "
                      "and batch" if ref else "this build's ops.decode('qbp')"),
        'qbp_T10_ms': qbp,
        'ms': ms,
        'ratio_to_qbp': {d: ms[d] / qbp for d in DECODES},
        'decode_plus_osd_ms': pipeline,
        'decode_plus_osd_ratio_to_qbp_plus_osd': {d: pipeline[d] / pipeline['qbp'] for d in DECODES},
        'decision_errors_fields': ['bit errors', 'codewords with a bit error',
                                   'codewords with a residual syndrome',
                                   'codewords with zero residual syndrome and a logical error'],
        'decision_errors': {n: steps[n]['decision_errors'] for n in STEPS},
        'iters_histogram': {d: steps[d]['iters_histogram'] for d in DECODES},
        'status0': {n: steps[n]['status0'] for n in STEPS},
        'steps': steps,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps({k: result[k] for k in ('qbp_T10_ms', 'ms', 'ratio_to_qbp', 'decode_plus_osd_ms',
                                             'decision_errors', 'iters_histogram', 'status0')}))


if __name__ == '__main__':
    main()
