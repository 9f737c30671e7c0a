#!/usr/bin/env python3
"""What OSD-0 post-processing costs beside the decode it follows: toric-5, fp64, B = 65 536
(bench.py config 3's batch: ops.sample_toric over the reference's p list), ops.decode('qbp',
T = 10) and ops.osd0 in both bases, each timed alone (warm-up, device events around each step,
median over the repeats), plus the decision_errors counts before OSD (on pred) and after it (on
ehat).  Every GPU step is a child process under its own `timeout`; a step that fails ends the
run.  Writes profiles/osd0_toric5_B65536_f64.json (or --out).

--hi measures the higher-order methods instead: ops.osd0, ops.osd('cs', 10) and ops.osd('e', 8),
zero base, on the same batch, each with its decision_errors counts and its time as a ratio to
OSD-0's; --ref-pkg DIR (a built gnn-decode_amd directory of another commit) also times that
build's ops.osd0 on the same machine and batch, and the ratios are taken to it.  Writes
profiles/osd_hi_toric5_B65536_f64.json (or --out).

usage: tools/osd_bench.py [--hi [--ref-pkg DIR]] [--batch B] [--repeats R] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = (0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.1)   # quantum/error_generate.py:252-260
STEPS = ('decode', 'osd0_zero', 'osd0_hard')
HI_STEPS = ('decode', 'osd0_zero', 'osd_osd0_0', 'osd_cs_10', 'osd_e_8')
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
    sys.path.insert(0, a.ref_pkg or os.path.join(ROOT, 'gnn-decode_amd'))
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
    elif name.startswith('osd_'):
        method, order = name[4:].rsplit('_', 1)
        out = (torch.empty_like(pred), torch.empty(a.batch, dtype=torch.int32, device=dev),
               torch.empty(a.batch, dtype=torch.int32, device=dev))
        res.update(timed(lambda: ops.osd(g, x, pred, 'zero', method, int(order), out=out),
                         a.warmup, a.repeats))
        res['decision_errors'] = ops.decision_errors(g, lg, out[0], y).tolist()
        res['status_nonzero'] = int(out[1].ne(0).sum())
        res['estimate_weight'] = int(out[0].sum())
        res['choice_nonzero'] = int(out[2].ne(0).sum())
    else:
        base = name.split('_')[1]
        out = (torch.empty_like(pred), torch.empty(a.batch, dtype=torch.int32, device=dev))
        res.update(timed(lambda: ops.osd0(g, x, pred, base, out=out), a.warmup, a.repeats))
        res['decision_errors'] = ops.decision_errors(g, lg, out[0], y).tolist()
        res['status_nonzero'] = int(out[1].ne(0).sum())
        res['estimate_weight'] = int(out[0].sum())
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


def main_hi(a):
    steps = {name: run_step(name, a) for name in HI_STEPS}
    if a.ref_pkg:
        steps['ref_osd0_zero'] = run_step('osd0_zero', a, os.path.abspath(a.ref_pkg))
    ref = steps['ref_osd0_zero' if a.ref_pkg else 'osd0_zero']['ms_median']
    timed_steps = [n for n in steps if n != 'decode']
    result = {
        'what': f'toric-5 fp64, B = {a.batch} (ops.sample_toric, seed 0, p uniform over '
                f'{list(PS)}), after ops.decode qbp T = {ITERS}, zero base: ops.osd0 and ops.osd '
                f"('osd0', 0), ('cs', 10), ('e', 8), each alone, device events around each call, "
                f'median of {a.repeats} after {a.warmup} warm-up calls, one process per step; 1x '
                f'MI355X',
        'reference': ("ops.osd0 of the --ref-pkg build (the parent commit), same machine and batch"
                      if a.ref_pkg else "this build's ops.osd0"),
        'reference_osd0_ms': ref,
        'decode_qbp_T10_ms': steps['decode']['ms_median'],
        'ms': {n: steps[n]['ms_median'] for n in timed_steps},
        'ratio_to_reference_osd0': {n: steps[n]['ms_median'] / ref for n in timed_steps},
        'candidate_phase_over_elimination': {
            n: (steps[n]['ms_median'] - steps['osd_osd0_0']['ms_median'])
            / steps['osd_osd0_0']['ms_median'] for n in ('osd_cs_10', 'osd_e_8')},
        'decision_errors_fields': ['bit errors', 'codewords with a bit error',
                                   'codewords with a residual syndrome',
                                   'codewords with zero residual syndrome and a logical error'],
        'decision_errors': {n: steps[n]['decision_errors'] for n in steps},
        'estimate_weight': {n: steps[n]['estimate_weight'] for n in timed_steps},
        'steps': steps,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps({k: result[k] for k in ('reference_osd0_ms', 'ms', 'ratio_to_reference_osd0',
                                             'decision_errors', 'estimate_weight')}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=180, help='seconds per GPU step')
    ap.add_argument('--hi', action='store_true', help='the higher-order methods (ops.osd)')
    ap.add_argument('--ref-pkg', help='with --hi: built gnn-decode_amd directory of the reference commit')
    ap.add_argument('--out')
    ap.add_argument('--step', choices=sorted(set(STEPS + HI_STEPS)), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'osd_hi_toric5_B65536_f64.json' if a.hi
                             else 'osd0_toric5_B65536_f64.json')
    if a.hi:
        return main_hi(a)
    steps = {name: run_step(name, a) for name in STEPS}
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
