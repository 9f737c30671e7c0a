#!/usr/bin/env python3
"""What min-sum BP with guided decimation costs and decides beside the decoders it stands next to:
toric-5, fp64, B = 65 536 (ops.sample_toric at p = 0.05, seed 0, the input of tools/relay_bench.py):
  minsum       ops.minsum(T = 10, early stop)
  relay        ops.relay, 6 legs x 10 iterations (ops.relay_gammas, seed 0), stop_after = 1
  bposd        ops.bposd(T = 10, 'zero', 'cs', 10)
  bpgd_least   ops.bpgd(10, 5, 16, 1, 'least', clamp 25)
  bpgd_most    ops.bpgd(10, 5, 16, 1, 'most', clamp 25)
all from this build.  Each call is timed alone (warm-up, device events around each call, median over
the repeats) and reports its codewords with status 0 and its decision_errors counts; bpgd also its
mean iterations and mean decimations.  Every GPU step is a child process under its own `timeout`; a
step that fails ends the run.  No threshold on time or failures: the numbers are reported as
measured.  One condition, from a CPU prototype of the method and not from this code: bpgd_least must
solve more codewords than minsum; the run exits 1 after writing its file if it does not.
Writes profiles/bpgd_toric5_B65536_f64.json (or --out).

usage: tools/bpgd_bench.py [--batch B] [--repeats R] [--warmup W] [--out FILE]"""
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
STEPS = ('minsum', 'relay', 'bposd', 'bpgd_least', 'bpgd_most')


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
        res['bp_status0'] = int(out[4].eq(0).sum())
    elif name == 'relay':
        gm = ops.relay_gammas(g.V, LEGS, seed=0, dtype=torch.float64, device=dev)
        out = ops.relay(g, x, gm, ITERS, ITERS, 1, ALPHA, BETA)
        res.update(timed(lambda: ops.relay(g, x, gm, ITERS, ITERS, 1, ALPHA, BETA, out=out),
                         a.warmup, a.repeats))
        decision, status = out[0], out[3]
        res['mean_iters'] = float(out[2].double().mean())
    else:
        pick = name.split('_')[1]
        out = ops.bpgd(g, x, *BPGD, pick, CLAMP, ALPHA, BETA)
        res.update(timed(lambda: ops.bpgd(g, x, *BPGD, pick, CLAMP, ALPHA, BETA, out=out),
                         a.warmup, a.repeats))
        decision, status = out[0], out[4]
        res['mean_iters'] = float(out[3].double().mean())
        res['mean_ndec'] = float(out[5].double().mean())
        late = out[5][status.eq(0) & out[5].gt(0)]
        res['solved_after_decimation'] = int(late.numel())
        res['mean_ndec_solved_after_decimation'] = (float(late.double().mean()) if late.numel()
                                                    else None)
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bpgd_toric5_B65536_f64.json'))
    ap.add_argument('--step', choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    steps = {name: run_step(name, a) for name in STEPS}
    result = {
        'what': f'toric-5 fp64, B = {a.batch} (ops.sample_toric, seed 0, p = {P}): ops.minsum(T = '
                f"{ITERS}, early stop), ops.relay ({LEGS} legs x {ITERS} iterations, "
                f"ops.relay_gammas seed 0, stop_after = 1), ops.bposd(T = {ITERS}, 'zero', 'cs', 10) "
                f'and ops.bpgd{BPGD} under both picks, clamp = {CLAMP}, alpha = {ALPHA}, beta = '
                f'{BETA}; each call alone, device events around each call, median of {a.repeats} '
                f'after {a.warmup} warm-up calls, one process per step; 1x '
                + ' / '.join(sorted({steps[n]['device'] for n in STEPS})),
        'ms': {n: steps[n]['ms_median'] for n in STEPS},
        'status0': {n: steps[n]['status0'] for n in STEPS},
        'decision_errors_fields': ['bit errors', 'codewords with a bit error',
                                   'codewords with a residual syndrome',
                                   'codewords with zero residual syndrome and a logical error'],
        'decision_errors': {n: steps[n]['decision_errors'] for n in STEPS},
        'mean_iters': {n: steps[n]['mean_iters'] for n in STEPS if 'mean_iters' in steps[n]},
        'bpgd_mean_ndec': {n: steps[n]['mean_ndec'] for n in STEPS if 'mean_ndec' in steps[n]},
        'steps': steps,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps({k: result[k] for k in ('ms', 'status0', 'decision_errors', 'mean_iters',
                                             'bpgd_mean_ndec')}))
    if not result['status0']['bpgd_least'] > result['status0']['minsum']:
        raise SystemExit('bpgd_least solved no more codewords than minsum: the kernel is suspect')


if __name__ == '__main__':
    main()
