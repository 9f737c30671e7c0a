#!/usr/bin/env python3
"""What the gated OSD and the one-call BP+OSD decoder cost beside the two separate calls they
replace: toric-5, fp64, B = 65 536 (ops.sample_toric over the reference's p list, seed 0), T = 10,
alpha 0.75, beta 0, ('cs', 10), zero base:
  ref_minsum     ops.minsum(early_stop=True) of the --ref-pkg build (the parent commit)
  ref_osd        ops.osd('cs', 10) of the --ref-pkg build on that pred: every codeword eliminated
  gated_minsum   ops.osd_gated with the min-sum status as the gate (llr given)
  gated_ones     ops.osd_gated with an all-ones gate: against ref_osd, the cost of the compaction
                 and of the indirection
  gated_zeros    ops.osd_gated with an all-zeros gate: the floor (compaction, pass-through, and an
                 elimination grid that leaves at once)
  bposd          ops.bposd
each call timed alone (warm-up, device events around each call, median over the repeats), with the
decision_errors counts of its estimate and the number of gated codewords.  Every GPU step is a
child process under its own `timeout`; a step that fails ends the run.  Without --ref-pkg the
yardstick rows come from this build.  Writes profiles/bposd_toric5_B65536_f64.json (or --out).

usage: tools/bposd_bench.py [--ref-pkg DIR] [--batch B] [--repeats R] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = (0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.1)   # quantum/error_generate.py:252-260
STEPS = ('ref_minsum', 'ref_osd', 'gated_minsum', 'gated_ones', 'gated_zeros', 'bposd')
ITERS = 10
ALPHA, BETA = 0.75, 0.0
OSD = ('zero', 'cs', 10)


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

    def real():
        return torch.empty(B * g.V, 1, dtype=torch.float64, device=dev)

    def ints():
        return torch.empty(B, dtype=torch.int32, device=dev)
    ms_out = (real(), real(), ints(), ints())               # pred, llr, iters_used, status
    ops.minsum(g, x, ITERS, ALPHA, BETA, True, out=ms_out)
    pred, llr, _, bp_status = ms_out
    osd_out = (real(), ints(), ints())
    res = {'step': name}
    if name == 'ref_minsum':
        res.update(timed(lambda: ops.minsum(g, x, ITERS, ALPHA, BETA, True, out=ms_out), a.warmup,
                         a.repeats))
        est, gated = pred, None
    elif name == 'ref_osd':
        res.update(timed(lambda: ops.osd(g, x, pred, *OSD, out=osd_out), a.warmup, a.repeats))
        est, gated = osd_out[0], B
    elif name == 'bposd':
        out = (osd_out[0], osd_out[1], osd_out[2], ints(), ints(), real(), real())
        work = torch.empty(ops.osd_gated_workspace(B), dtype=torch.uint8, device=dev)
        res.update(timed(lambda: ops.bposd(g, x, ITERS, ALPHA, BETA, True, *OSD, out=out, work=work),
                         a.warmup, a.repeats))
        est, gated = out[0], int(out[4].ne(0).sum())
    else:
        gate = {'gated_minsum': bp_status, 'gated_ones': torch.ones_like(bp_status),
                'gated_zeros': torch.zeros_like(bp_status)}[name]
        work = torch.empty(ops.osd_gated_workspace(B), dtype=torch.uint8, device=dev)
        res.update(timed(lambda: ops.osd_gated(g, x, pred, gate, *OSD, llr=llr, out=osd_out,
                                               work=work), a.warmup, a.repeats))
        est, gated = osd_out[0], int(gate.ne(0).sum())
    res['decision_errors'] = ops.decision_errors(g, lg, est, y).tolist()
    res['gated'] = gated
    res['bp_status0'] = int(bp_status.eq(0).sum())
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
                                      'ops.minsum and ops.osd are the yardstick')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bposd_toric5_B65536_f64.json'))
    ap.add_argument('--step', choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    ref = os.path.abspath(a.ref_pkg) if a.ref_pkg else None
    steps = {name: run_step(name, a, ref if name.startswith('ref_') else None) for name in STEPS}
    ms = {n: steps[n]['ms_median'] for n in STEPS}
    ref_sum = ms['ref_minsum'] + ms['ref_osd']
    result = {
        'what': f'toric-5 fp64, B = {a.batch} (ops.sample_toric, seed 0, p uniform over {list(PS)}), '
                f'T = {ITERS}, alpha = {ALPHA}, beta = {BETA}, osd {OSD}: the two separate calls, '
                f'ops.osd_gated under three gates and ops.bposd; each call alone, device events '
                f'around each call, median of {a.repeats} after {a.warmup} warm-up calls, one process '
                f'per step; 1x MI355X',
        'reference': ('ops.minsum and ops.osd of the --ref-pkg build (the parent commit), same machine '
                      'and batch' if ref else "this build's ops.minsum and ops.osd"),
        'ms': ms,
        'ref_minsum_plus_osd_ms': ref_sum,
        'bposd_ratio_to_ref_minsum_plus_osd': ms['bposd'] / ref_sum,
        'gated_minsum_ratio_to_ref_osd': ms['gated_minsum'] / ms['ref_osd'],
        'gated_ones_ratio_to_ref_osd': ms['gated_ones'] / ms['ref_osd'],
        'gated_zeros_ms': ms['gated_zeros'],
        'gated': {n: steps[n]['gated'] for n in STEPS},
        'bp_status0': steps['bposd']['bp_status0'],
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
    print(json.dumps({k: result[k] for k in ('ms', 'ref_minsum_plus_osd_ms',
                                             'bposd_ratio_to_ref_minsum_plus_osd',
                                             'gated_ones_ratio_to_ref_osd', 'gated', 'decision_errors')}))


if __name__ == '__main__':
    main()
