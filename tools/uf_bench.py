#!/usr/bin/env python3
"""What the union-find decoder costs and decides beside the BP decoders, and what it adds behind
them as the finisher of their unsolved codewords: toric-5, fp64, B = 65 536 (ops.sample_toric at
p = 0.05, seed 0, the input of tools/bpgd_bench.py):
  minsum     ops.minsum(T = 10, early stop)
  bposd      ops.bposd(T = 10, 'zero', 'cs', 10)
  relay      ops.relay, 6 legs x 10 iterations (ops.relay_gammas, seed 0), stop_after = 1
  uf         ops.uf alone
  relay_uf   relay, then ops.uf gated by relay's status into relay's ehat and status
  bpgd_uf    ops.bpgd(10, 5, 16, 1, 'least', clamp 25), then ops.uf gated the same way
all from this build.  Each step is timed alone (warm-up, device events around the step's calls,
median over the repeats) and reports the four decision_errors counts of its final decision; the
two-stage steps also the codewords the first stage left to uf.  Every GPU step is a child process
under its own `timeout`; a step that fails ends the run.  No threshold on time or on logical
failures: the numbers are reported as measured.  One condition, a property of the definition and
not a measurement: every step that ends in uf leaves 0 codewords with a residual syndrome; the run
exits 1 after writing its file otherwise.
Writes profiles/uf_toric5_B65536_f64.json (or --out).

usage: tools/uf_bench.py [--batch B] [--repeats R] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0.05
ITERS = 10
LEGS = 6
BPGD = (10, 5, 16, 1)
CLAMP = 25.0
ALPHA, BETA = 0.75, 0.0
STEPS = ('minsum', 'bposd', 'relay', 'uf', 'relay_uf', 'bpgd_uf')
UF_STEPS = ('uf', 'relay_uf', 'bpgd_uf')


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
    B = a.batch
    x, y = ops.sample_toric(g, B, [P], seed=0, dtype=torch.float64)
    res = {'step': name, 'device': torch.cuda.get_device_name(dev)}
    if name == 'minsum':
        out = ops.minsum(g, x, ITERS, ALPHA, BETA, True)
        res.update(timed(lambda: ops.minsum(g, x, ITERS, ALPHA, BETA, True, out=out), a.warmup,
                         a.repeats))
        decision, status = out[0], out[3]
    elif name == 'bposd':
        out = ops.bposd(g, x, ITERS, ALPHA, BETA, True, 'zero', 'cs', 10)
        work = torch.empty(ops.osd_gated_workspace(B), dtype=torch.uint8, device=dev)
        res.update(timed(lambda: ops.bposd(g, x, ITERS, ALPHA, BETA, True, 'zero', 'cs', 10, out=out,
                                           work=work), a.warmup, a.repeats))
        decision, status = out[0], out[1]
    elif name == 'uf':
        out = ops.uf(g, x)
        res.update(timed(lambda: ops.uf(g, x, out=out), a.warmup, a.repeats))
        decision, status = out[0], out[2]
        res['mean_rounds'] = float(out[1].double().mean())
        res['max_rounds'] = int(out[1].max())
        res['mean_nfull'] = float(out[3].double().mean())
    else:
        if name.startswith('relay'):
            gm = ops.relay_gammas(g.V, LEGS, seed=0, dtype=torch.float64, device=dev)
            out = ops.relay(g, x, gm, ITERS, ITERS, 1, ALPHA, BETA)
            first = lambda: ops.relay(g, x, gm, ITERS, ITERS, 1, ALPHA, BETA, out=out)
            ehat, status = out[0], out[3]
        else:
            out = ops.bpgd(g, x, *BPGD, 'least', CLAMP, ALPHA, BETA)
            first = lambda: ops.bpgd(g, x, *BPGD, 'least', CLAMP, ALPHA, BETA, out=out)
            ehat, status = out[0], out[4]
        if name.endswith('_uf'):
            rounds = torch.zeros(B, dtype=torch.int32, device=dev)

            def both():
                first()
                ops.uf(g, x, gate=status, out=(ehat, rounds, status, None))
            first()
            torch.cuda.synchronize()
            res['left_to_uf'] = int(status.ne(0).sum())
            res.update(timed(both, a.warmup, a.repeats))
        else:
            res.update(timed(first, a.warmup, a.repeats))
        decision = ehat
    res['status0'] = int(status.eq(0).sum())
    res['decision_errors'] = ops.decision_errors(g, lg, decision, y).tolist()
    print(json.dumps(res), flush=True)


def run_step(name, a):
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__),
           '--step', name, '--batch', str(a.batch), '--repeats', str(a.repeats), '--warmup',
           str(a.warmup)]
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'uf_toric5_B65536_f64.json'))
    ap.add_argument('--step', choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    steps = {name: run_step(name, a) for name in STEPS}
    result = {
        'what': f'toric-5 fp64, B = {a.batch} (ops.sample_toric, seed 0, p = {P}): ops.minsum(T = '
                f"{ITERS}, early stop), ops.bposd(T = {ITERS}, 'zero', 'cs', 10), ops.relay ({LEGS} "
                f'legs x {ITERS} iterations, ops.relay_gammas seed 0, stop_after = 1), ops.uf alone, '
                f"and ops.uf gated by the status of relay and of ops.bpgd{BPGD} 'least' (clamp = "
                f'{CLAMP}) into their ehat; alpha = {ALPHA}, beta = {BETA}; each step alone, device '
                f'events around the step, median of {a.repeats} after {a.warmup} warm-up runs, one '
                'process per step; 1x ' + ' / '.join(sorted({steps[n]['device'] for n in STEPS})),
        'ms': {n: steps[n]['ms_median'] for n in STEPS},
        'status0': {n: steps[n]['status0'] for n in STEPS},
        'decision_errors_fields': ['bit errors', 'codewords with a bit error',
                                   'codewords with a residual syndrome',
                                   'codewords with zero residual syndrome and a logical error'],
        'decision_errors': {n: steps[n]['decision_errors'] for n in STEPS},
        'left_to_uf': {n: steps[n]['left_to_uf'] for n in STEPS if 'left_to_uf' in steps[n]},
        'uf_mean_rounds': steps['uf']['mean_rounds'],
        'uf_max_rounds': steps['uf']['max_rounds'],
        'steps': steps,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps({k: result[k] for k in ('ms', 'status0', 'decision_errors', 'left_to_uf',
                                             'uf_mean_rounds', 'uf_max_rounds')}))
    residual = {n: result['decision_errors'][n][2] for n in UF_STEPS}
    if any(residual.values()):
        raise SystemExit(f'uf left codewords with a residual syndrome: {residual}')


if __name__ == '__main__':
    main()
