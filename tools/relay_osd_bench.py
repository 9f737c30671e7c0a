#!/usr/bin/env python3
"""What relay followed by gated OSD costs and decides beside the two decoders it joins: toric-5,
fp64, B = 65 536 (ops.sample_toric at p = 0.05, seed 0), alpha 0.75, beta 0, OSD ('cs', 10) on the
zero base:
  bposd              ops.bposd(T = 10)                                   (the parent commit's code)
  relay_S1           ops.relay, 6 legs x 10 iterations, stop_after = 1   (the parent commit's code)
  relay_osd_last_S1  ops.relay_osd, the same legs, soft = 'last', stop_after = 1
  relay_osd_mean_S1  the same with soft = 'mean'
  relay_osd_last_S3, relay_osd_mean_S3   stop_after = 3
  relay_soft_last_S1, relay_soft_mean_S1  ops.relay_soft alone: what the MEAN accumulation adds
Each call is timed alone (warm-up, device events around each call, median over the repeats) and
reports the codewords it gates into OSD and its decision_errors counts; the relay_osd steps also
report, on the codewords relay left unsolved, how many end with a residual syndrome or a logical
error.  Every GPU step is a child process under its own `timeout`; a step that fails ends the run.
No threshold: the numbers are reported as measured.
Writes profiles/relay_osd_toric5_B65536_f64.json (or --out).

usage: tools/relay_osd_bench.py [--batch B] [--repeats R] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from relay_bench import ALPHA, BETA, ITERS, LEGS, P, ROOT, timed  # noqa: E402

STEPS = ('bposd', 'relay_S1', 'relay_osd_last_S1', 'relay_osd_mean_S1', 'relay_osd_last_S3',
         'relay_osd_mean_S3', 'relay_soft_last_S1', 'relay_soft_mean_S1')
OSD = ('zero', 'cs', 10)


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
    gm = ops.relay_gammas(g.V, LEGS, seed=0, dtype=torch.float64, device=dev)
    work = torch.empty(ops.osd_gated_workspace(B), dtype=torch.uint8, device=dev)
    res = {'step': name}
    gate = None
    if name == 'bposd':
        out = ops.bposd(g, x, ITERS, ALPHA, BETA, True, *OSD)
        res.update(timed(lambda: ops.bposd(g, x, ITERS, ALPHA, BETA, True, *OSD, out=out,
                                           work=work), a.warmup, a.repeats))
        decision, gate = out[0], out[4]
    elif name.startswith('relay_S'):
        S = int(name[-1])
        out = ops.relay(g, x, gm, ITERS, ITERS, S, ALPHA, BETA)
        res.update(timed(lambda: ops.relay(g, x, gm, ITERS, ITERS, S, ALPHA, BETA, out=out),
                         a.warmup, a.repeats))
        decision = out[0]
        res['unsolved'] = int(out[3].ne(0).sum())
    else:
        _, kind, mode, S = name.split('_')
        S = int(S[1:])
        if kind == 'soft':
            out = ops.relay_soft(g, x, gm, ITERS, ITERS, S, ALPHA, BETA, soft=mode)
            res.update(timed(lambda: ops.relay_soft(g, x, gm, ITERS, ITERS, S, ALPHA, BETA,
                                                    soft=mode, out=out), a.warmup, a.repeats))
            decision = out[2]
            res['unsolved'] = int(out[5].ne(0).sum())
        else:
            out = ops.relay_osd(g, x, gm, ITERS, ITERS, S, ALPHA, BETA, mode, *OSD)
            res.update(timed(lambda: ops.relay_osd(g, x, gm, ITERS, ITERS, S, ALPHA, BETA, mode,
                                                   *OSD, out=out, work=work), a.warmup, a.repeats))
            decision, gate = out[0], out[6]
            res['osd_status1'] = int(out[1].ne(0).sum())
    res['decision_errors'] = ops.decision_errors(g, lg, decision, y).tolist()
    if gate is not None:
        res['gated'] = int(gate.ne(0).sum())
        on = gate.ne(0)
        V = g.V
        if int(on.sum()):
            sub = ops.decision_errors(g, lg, decision.view(B, V)[on].reshape(-1, 1).contiguous(),
                                      y.view(B, V)[on].reshape(-1, 1).contiguous()).tolist()
        else:
            sub = [0, 0, 0, 0]
        res['decision_errors_on_gated'] = sub
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles',
                                                  'relay_osd_toric5_B65536_f64.json'))
    ap.add_argument('--step', choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    steps = {name: run_step(name, a) for name in STEPS}
    result = {
        'what': f'toric-5 fp64, B = {a.batch} (ops.sample_toric, seed 0, p = {P}), alpha = {ALPHA}, '
                f"beta = {BETA}, OSD ('cs', 10) on the zero base: ops.bposd(T = {ITERS}), ops.relay "
                f'({LEGS} legs x {ITERS} iterations, ops.relay_gammas seed 0, stop_after = 1), '
                f"ops.relay_osd on the same legs with soft = 'last' / 'mean' at stop_after = 1 and "
                f'3, and ops.relay_soft alone at stop_after = 1; each call alone, device events '
                f'around each call, median of {a.repeats} after {a.warmup} warm-up calls, one '
                f'process per step; 1x MI355X',
        'ms': {n: [steps[n]['ms_median'], steps[n]['ms_min'], steps[n]['ms_max']] for n in STEPS},
        'ms_fields': ['median', 'min', 'max'],
        'gated': {n: steps[n]['gated'] for n in STEPS if 'gated' in steps[n]},
        'decision_errors_fields': ['bit errors', 'codewords with a bit error',
                                   'codewords with a residual syndrome',
                                   'codewords with zero residual syndrome and a logical error'],
        'decision_errors': {n: steps[n]['decision_errors'] for n in STEPS},
        'failed_codewords': {n: steps[n]['decision_errors'][2] + steps[n]['decision_errors'][3]
                             for n in STEPS},
        'decision_errors_on_gated': {n: steps[n]['decision_errors_on_gated'] for n in STEPS
                                     if 'decision_errors_on_gated' in steps[n]},
        'steps': steps,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps({k: result[k] for k in ('ms', 'gated', 'decision_errors', 'failed_codewords',
                                             'decision_errors_on_gated')}))


if __name__ == '__main__':
    main()
