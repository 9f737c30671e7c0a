#!/usr/bin/env python3
"""What BP+LSD costs and decides beside BP+OSD and belief-find, on the input of tools/ufw_bench.py:
toric-5, fp64, B = 65 536 (ops.sample_toric at p = 0.05, seed 0), min-sum T = 10 with early stop:
  bplsd_k       ops.bplsd('zero', bits_per_step = k) for k in 0, 1, 2, 4
  bposd_osd0    ops.bposd('zero', 'osd0', 0)      the elimination bplsd replaces
  bposd_cs10    ops.bposd('zero', 'cs', 10)
  belief_find   ops.belief_find(scale = 2, wmax = 32)
and the same pairs on LDPC(648,324), fp32, B = 16 384 (ops.sample_awgn, the all-zero codeword, SNR
1 / 2 / 3 / 4 dB, seed 0), T = 12, base 'hard', where the code is large and the error small:
  ldpc_bplsd_k, ldpc_bposd_osd0
Each entry is timed alone (warm-up, device events around the entry's call, median over the
repeats) and reports the four decision_errors counts of its final decision, the codewords left to
the second stage and, for bplsd, the mean and the largest `rounds` and the mean `ncols` over them.
With --ref-pkg the bposd entries also run on that package directory (the parent commit's
gnn-decode_amd, built) in the same run, as ref_bposd_osd0 / ref_ldpc_bposd_osd0.  Every GPU step
is a child process under its own `timeout`; a step that fails ends the run.  No threshold on time or on failures: the numbers are
reported as measured.  One condition, a property of the definition and not a measurement: bplsd's
status equals bposd('osd0')'s on every codeword; the run exits 1 after writing its file otherwise.
Writes profiles/lsd_toric5_B65536_f64.json (or --out).

usage: tools/lsd_bench.py [--ref-pkg DIR] [--batch B] [--ldpc-batch B] [--repeats R] [--warmup W]
                          [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0.05
ITERS, LDPC_ITERS = 10, 12
ALPHA, BETA = 0.75, 0.0
SCALE, WMAX = 2.0, 32
BITS = (0, 1, 2, 4)
LDPC_SNR = (1.0, 2.0, 3.0, 4.0)
STEPS = ('toric', 'ldpc')


def timed(fn, warmup, repeats):
    """Median device-event time of fn."""
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
    sys.path.insert(0, os.path.abspath(a.ref_pkg) if a.only_bposd
                    else os.path.join(ROOT, 'gnn-decode_amd'))
    import numpy as np
    import torch
    import gnndecode as gd
    from gnndecode import ops
    dev = torch.device('cuda', 0)
    ldpc = name == 'ldpc'
    if ldpc:
        H = gd.codes.get_code('ldpc_648_324')
        g = gd.TannerGraph(H, device=dev)
        lg, B, iters, base, prefix = None, a.ldpc_batch, LDPC_ITERS, 'hard', 'ldpc_'
        x, y = ops.sample_awgn(g, B, LDPC_SNR, codeword_bit=0, seed=0, dtype=torch.float32)
    else:
        H = gd.codes.toric_code(5)
        g = gd.TannerGraph(H, device=dev)
        lg = torch.from_numpy(gd.codes.toric_logicals(H).astype(np.int32)).to(dev)
        B, iters, base, prefix = a.batch, ITERS, 'zero', ''
        x, y = ops.sample_toric(g, B, [P], seed=0, dtype=torch.float64)
    work = torch.empty(ops.osd_gated_workspace(B), dtype=torch.uint8, device=dev)
    entries = {}

    def counts(decision):
        return ops.decision_errors(g, lg, decision, y).tolist()

    if a.only_bposd:
        methods = (('osd0', 0),)
    else:
        methods = (('osd0', 0),) if ldpc else (('osd0', 0), ('cs', 10))
    status0 = None
    for method, order in methods:
        out = ops.bposd(g, x, iters, ALPHA, BETA, True, base, method, order)
        t = timed(lambda: ops.bposd(g, x, iters, ALPHA, BETA, True, base, method, order, out=out,
                                    work=work), a.warmup, a.repeats)
        entries[f'{prefix}bposd_{method}{order or ""}'] = dict(
            t, decision_errors=counts(out[0]), status0=int(out[1].eq(0).sum()),
            left_to_osd=int(out[4].ne(0).sum()))
        if method == 'osd0':
            status0 = out[1].clone()
    if not a.only_bposd:
        for k in BITS:
            out = ops.bplsd(g, x, iters, ALPHA, BETA, True, base, k)
            t = timed(lambda: ops.bplsd(g, x, iters, ALPHA, BETA, True, base, k, out=out, work=work),
                      a.warmup, a.repeats)
            left = out[6] != 0
            n = max(int(left.sum()), 1)
            entries[f'{prefix}bplsd_{k}'] = dict(
                t, bits_per_step=k, decision_errors=counts(out[0]), status0=int(out[1].eq(0).sum()),
                left_to_lsd=int(left.sum()), status_is_osd0s=bool(torch.equal(out[1], status0)),
                mean_rounds=float(out[2][left].double().sum()) / n,
                max_rounds=int(out[2].max()) if B else 0,
                mean_nclus=float(out[3][left].double().sum()) / n,
                mean_ncols=float(out[4][left].double().sum()) / n)
        if not ldpc:
            out = ops.belief_find(g, x, iters, ALPHA, BETA, True, SCALE, WMAX)
            t = timed(lambda: ops.belief_find(g, x, iters, ALPHA, BETA, True, SCALE, WMAX, out=out),
                      a.warmup, a.repeats)
            entries['belief_find'] = dict(t, decision_errors=counts(out[0]), scale=SCALE, wmax=WMAX,
                                          left_to_ufw=int(out[3].ne(0).sum()))
    print(json.dumps({'step': name, 'device': torch.cuda.get_device_name(dev), 'batch': B,
                      'entries': entries}), flush=True)


def run_step(name, a, ref=False):
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__),
           '--step', name, '--batch', str(a.batch), '--ldpc-batch', str(a.ldpc_batch), '--repeats',
           str(a.repeats), '--warmup', str(a.warmup)]
    if ref:
        cmd += ['--only-bposd', '--ref-pkg', a.ref_pkg]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-3000:])
        raise SystemExit(f'step {name} failed (exit {r.returncode}); nothing further started')
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--ldpc-batch', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--timeout', type=int, default=240, help='seconds per GPU step')
    ap.add_argument('--ref-pkg', help="the parent commit's gnn-decode_amd directory, built: "
                                      "bposd('osd0') on it too")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lsd_toric5_B65536_f64.json'))
    ap.add_argument('--step', choices=STEPS, help=argparse.SUPPRESS)
    ap.add_argument('--only-bposd', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    entries, devices = {}, set()
    for name in STEPS:
        s = run_step(name, a)
        entries.update(s['entries'])
        devices.add(s['device'])
        if a.ref_pkg:
            entries.update({'ref_' + k: v for k, v in run_step(name, a, ref=True)['entries'].items()})
    result = {
        'what': f'toric-5 fp64, B = {a.batch} (ops.sample_toric, seed 0, p = {P}), T = {ITERS}, base '
                f"'zero': ops.bplsd with bits_per_step in {list(BITS)}, ops.bposd ('osd0', 0) and "
                f"('cs', 10), ops.belief_find(scale = {SCALE}, wmax = {WMAX}); LDPC(648,324) fp32, "
                f'B = {a.ldpc_batch} (ops.sample_awgn, all-zero codeword, SNR {list(LDPC_SNR)} dB, '
                f"seed 0), T = {LDPC_ITERS}, base 'hard': ops.bplsd and ops.bposd ('osd0', 0) as "
                f'ldpc_*; alpha = {ALPHA}, beta = {BETA}, early stop; ref_*: ops.bposd on the parent '
                "commit's package in the same run; device events around each entry, median of "
                f'{a.repeats} after {a.warmup} warm-up runs, one process per step; 1x '
                + ' / '.join(sorted(devices)),
        'ms': {k: v['ms_median'] for k, v in entries.items()},
        'decision_errors_fields': ['bit errors', 'codewords with a bit error',
                                   'codewords with a residual syndrome',
                                   'codewords with zero residual syndrome and a logical error'],
        'decision_errors': {k: v['decision_errors'] for k, v in entries.items()},
        'failed': {k: (v['decision_errors'][2] + v['decision_errors'][3]
                       if 'ldpc_' not in k else v['decision_errors'][1])
                   for k, v in entries.items()},
        'rounds': {k: {f: v[f] for f in ('mean_rounds', 'max_rounds', 'mean_nclus', 'mean_ncols')}
                   for k, v in entries.items() if 'bits_per_step' in v},
        'entries': entries,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps({k: result[k] for k in ('ms', 'failed', 'rounds')}))
    wrong = [k for k, v in entries.items() if v.get('status_is_osd0s') is False]
    if wrong:
        raise SystemExit(f'status differs from bposd(osd0) in {wrong}')


if __name__ == '__main__':
    main()
