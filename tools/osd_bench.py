#!/usr/bin/env python3
"""What OSD-0 post-processing costs beside the decode it follows: toric-5, fp64, B = 65 536
(bench.py config 3's batch: ops.sample_toric over the reference's p list), ops.decode('qbp',
T = 10) and ops.osd0 in both bases, each timed alone (warm-up, device events around each step,
median over the repeats), plus the decision_errors counts before OSD (on pred) and after it (on
ehat).  Every GPU step is a child process under its own `timeout`; a step that fails ends the
run.  Writes profiles/osd0_toric5_B65536_f64.json (or --out).

usage: tools/osd_bench.py [--batch B] [--repeats R] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = (0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.1)   # quantum/error_generate.py:252-260
STEPS = ('decode', 'osd0_zero', 'osd0_hard')
ITERS = 10


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
    sys.path.insert(0, os.path.join(ROOT, 'gnn-decode_amd'))
    import numpy as np
    import torch
    import gnndecode as gd
    from gnndecode import ops
    dev = torch.device('cuda', 0)
    H = gd.codes.toric_code(5)
    g = gd.TannerGraph(H, device=dev)
    lg = torch.from_numpy(gd.codes.toric_logicals(H).astype(np.int32)).to(dev)
    x, y = ops.sample_toric(g, a.batch, PS, seed=0, dtype=torch.float64)
    pred = torch.empty(a.batch * g.V, 1, dtype=torch.float64, device=dev)
    ops.decode(g, 'qbp', x, ITERS, out=pred)
    res = {'step': name}
    if name == 'decode':
        res.update(timed(lambda: ops.decode(g, 'qbp', x, ITERS, out=pred), a.warmup, a.repeats))
        res['decision_errors'] = ops.decision_errors(g, lg, pred, y).tolist()
    else:
        base = name.split('_')[1]
        out = (torch.empty_like(pred), torch.empty(a.batch, dtype=torch.int32, device=dev))
        res.update(timed(lambda: ops.osd0(g, x, pred, base, out=out), a.warmup, a.repeats))
        res['decision_errors'] = ops.decision_errors(g, lg, out[0], y).tolist()
        res['status_nonzero'] = int(out[1].ne(0).sum())
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=180, help='seconds per GPU step')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'osd0_toric5_B65536_f64.json'))
    ap.add_argument('--step', choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    steps = {}
    for name in STEPS:
        r = subprocess.run(['timeout', '-k', '10', str(a.timeout), sys.executable,
                            os.path.abspath(__file__), '--step', name, '--batch', str(a.batch),
                            '--repeats', str(a.repeats), '--warmup', str(a.warmup)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            raise SystemExit(f'step {name} failed (exit {r.returncode}); nothing further started')
        steps[name] = json.loads(r.stdout.strip().splitlines()[-1])
    dec = steps['decode']['ms_median']
    names = ['bit errors', 'codewords with a bit error', 'codewords with a residual syndrome',
             'codewords with zero residual syndrome and a logical error']
    result = {
        'what': f'toric-5 fp64, B = {a.batch} (ops.sample_toric, seed 0, p uniform over '
                f'{list(PS)}): ops.decode qbp T = {ITERS} and ops.osd0 each alone, device events '
                f'around each call, median of {a.repeats} after {a.warmup} warm-up calls, one '
                f'process per step; 1x MI355X',
        'decode_qbp_T10_ms': dec,
        'osd0_ms': {b: steps[f'osd0_{b}']['ms_median'] for b in ('zero', 'hard')},
        'osd0_over_decode': {b: steps[f'osd0_{b}']['ms_median'] / dec for b in ('zero', 'hard')},
        'decision_errors_fields': names,
        'decision_errors_before_osd': steps['decode']['decision_errors'],
        'decision_errors_after_osd': {b: steps[f'osd0_{b}']['decision_errors'] for b in ('zero', 'hard')},
        'osd0_status_nonzero': {b: steps[f'osd0_{b}']['status_nonzero'] for b in ('zero', 'hard')},
        'steps': steps,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps({k: result[k] for k in ('decode_qbp_T10_ms', 'osd0_ms', 'osd0_over_decode',
                                             'decision_errors_before_osd',
                                             'decision_errors_after_osd')}))


if __name__ == '__main__':
    main()
