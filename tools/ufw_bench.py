#!/usr/bin/env python3
"""What weighted union-find and belief-find cost and decide beside uf and bposd, on the input of
tools/uf_bench.py: toric-5, fp64, B = 65 536 (ops.sample_toric at p = 0.05, seed 0):
  uf            ops.uf alone
  ufw_scale0    ops.ufw(scale = 0): uf's bits through the weighted kernel (the cost of the jump)
  ufw_priors    ops.ufw on the channel priors in x (scale = 2, wmax = 32, the untuned defaults)
  belief_find   ops.belief_find(T = 10, early stop) over scale in {0.5, 1, 2, 4} x wmax in
                {8, 32, 128}, one entry per pair
  relay_ufw     ops.relay_soft (6 legs x 10 iterations, ops.relay_gammas seed 0, stop_after = 1,
                soft = 'last'), then ops.ufw on its soft LLRs gated by its status into its ehat
                and status (scale = 2, wmax = 32)
  bposd         ops.bposd(T = 10, 'zero', 'cs', 10)
all from this build.  Each entry is timed alone (warm-up, device events around the entry's calls,
median over the repeats) and reports the four decision_errors counts of its final decision.  uf,
ufw_scale0 and ufw_priors are timed in one process, alternating, so their ratio does not rest on
two processes' clocks.  Every GPU step is a child process under its own `timeout`; a step that
fails ends the run.  No threshold on time or on logical failures: the numbers are reported as
measured, and bposd and uf of the same run are the reference points.  One condition, a property of
the definition and not a measurement: every entry that ends in uf or ufw leaves 0 codewords with a
residual syndrome, and ufw_scale0 decides exactly what uf decides; the run exits 1 after writing
its file otherwise.
Writes profiles/ufw_toric5_B65536_f64.json (or --out).

usage: tools/ufw_bench.py [--batch B] [--repeats R] [--warmup W] [--out FILE]"""
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
ALPHA, BETA = 0.75, 0.0
SCALE, WMAX = 2.0, 32
GRID_SCALE = (0.5, 1.0, 2.0, 4.0)
GRID_WMAX = (8, 32, 128)
STEPS = ('uf_ufw', 'belief_find', 'relay_ufw', 'bposd')


def summary(ms, repeats, warmup):
    return {'ms_median': statistics.median(ms), 'ms_min': min(ms), 'ms_max': max(ms),
            'repeats': repeats, 'warmup': warmup}


def timed(fns, warmup, repeats):
    """Median device-event time of each fn, the fns alternating inside every repeat."""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [summary(m, repeats, warmup) for m in ms]


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
    entries = {}

    def counts(decision):
        return ops.decision_errors(g, lg, decision, y).tolist()

    def growth(rounds, events):
        return {'mean_rounds': float(rounds.double().mean()), 'max_rounds': int(rounds.max()),
                'mean_events': float(events.double().mean())}

    if name == 'uf_ufw':
        o_uf = ops.uf(g, x)
        o_s0 = ops.ufw(g, x, None, 0.0, WMAX)
        o_pr = ops.ufw(g, x, None, SCALE, WMAX)
        t = timed([lambda: ops.uf(g, x, out=o_uf),
                   lambda: ops.ufw(g, x, None, 0.0, WMAX, out=o_s0),
                   lambda: ops.ufw(g, x, None, SCALE, WMAX, out=o_pr)], a.warmup, a.repeats)
        entries['uf'] = dict(t[0], decision_errors=counts(o_uf[0]),
                             mean_rounds=float(o_uf[1].double().mean()))
        entries['ufw_scale0'] = dict(t[1], decision_errors=counts(o_s0[0]),
                                     same_bits_as_uf=all(bool(torch.equal(p, q))
                                                         for p, q in zip(o_s0[:4], o_uf)),
                                     **growth(o_s0[1], o_s0[4]))
        entries['ufw_priors'] = dict(t[2], decision_errors=counts(o_pr[0]), scale=SCALE, wmax=WMAX,
                                     **growth(o_pr[1], o_pr[4]))
    elif name == 'belief_find':
        out = ops.belief_find(g, x, ITERS, ALPHA, BETA, True, SCALE, WMAX)
        for scale in GRID_SCALE:
            for wmax in GRID_WMAX:
                fn = lambda: ops.belief_find(g, x, ITERS, ALPHA, BETA, True, scale, wmax, out=out)
                t = timed([fn], a.warmup, a.repeats)[0]
                entries[f'belief_find_s{scale:g}_w{wmax}'] = dict(
                    t, decision_errors=counts(out[0]), scale=scale, wmax=wmax,
                    left_to_ufw=int(out[3].ne(0).sum()), status0=int(out[1].eq(0).sum()),
                    mean_rounds_of_the_unsolved=float(out[6][out[3] != 0].double().mean()),
                    mean_events_of_the_unsolved=float(out[8][out[3] != 0].double().mean()))
    elif name == 'relay_ufw':
        gm = ops.relay_gammas(g.V, LEGS, seed=0, dtype=torch.float64, device=dev)
        out = ops.relay_soft(g, x, gm, ITERS, ITERS, 1, ALPHA, BETA, 'last')
        pred, soft, ehat, llr, its, status, leg, nsol = out

        def both():
            ops.relay_soft(g, x, gm, ITERS, ITERS, 1, ALPHA, BETA, 'last', out=out)
            ops.ufw(g, x, llr=soft, scale=SCALE, wmax=WMAX, gate=status,
                    out=(ehat, None, status, None, None))
        torch.cuda.synchronize()
        left = int(status.ne(0).sum())
        t = timed([both], a.warmup, a.repeats)[0]
        entries['relay_ufw'] = dict(t, decision_errors=counts(ehat), scale=SCALE, wmax=WMAX,
                                    left_to_ufw=left, status0=int(status.eq(0).sum()))
    else:
        out = ops.bposd(g, x, ITERS, ALPHA, BETA, True, 'zero', 'cs', 10)
        work = torch.empty(ops.osd_gated_workspace(B), dtype=torch.uint8, device=dev)
        t = timed([lambda: ops.bposd(g, x, ITERS, ALPHA, BETA, True, 'zero', 'cs', 10, out=out,
                                     work=work)], a.warmup, a.repeats)[0]
        entries['bposd'] = dict(t, decision_errors=counts(out[0]), status0=int(out[1].eq(0).sum()),
                                left_to_osd=int(out[4].ne(0).sum()))
    print(json.dumps({'step': name, 'device': torch.cuda.get_device_name(dev), 'entries': entries}),
          flush=True)


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ufw_toric5_B65536_f64.json'))
    ap.add_argument('--step', choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    steps = [run_step(name, a) for name in STEPS]
    entries = {k: v for s in steps for k, v in s['entries'].items()}
    result = {
        'what': f'toric-5 fp64, B = {a.batch} (ops.sample_toric, seed 0, p = {P}): ops.uf, '
                f'ops.ufw(scale = 0) and ops.ufw on the priors (scale = {SCALE}, wmax = {WMAX}) '
                f'alternating in one process; ops.belief_find(T = {ITERS}, early stop) over scale in '
                f'{list(GRID_SCALE)} x wmax in {list(GRID_WMAX)}; ops.relay_soft ({LEGS} legs x '
                f"{ITERS} iterations, ops.relay_gammas seed 0, stop_after = 1, 'last') then ops.ufw "
                f'on its soft LLRs gated by its status (scale = {SCALE}, wmax = {WMAX}); '
                f"ops.bposd(T = {ITERS}, 'zero', 'cs', 10); alpha = {ALPHA}, beta = {BETA}; device "
                f'events around each entry, median of {a.repeats} after {a.warmup} warm-up runs, '
                'one process per step; 1x ' + ' / '.join(sorted({s['device'] for s in steps})),
        'ms': {k: v['ms_median'] for k, v in entries.items()},
        'decision_errors_fields': ['bit errors', 'codewords with a bit error',
                                   'codewords with a residual syndrome',
                                   'codewords with zero residual syndrome and a logical error'],
        'decision_errors': {k: v['decision_errors'] for k, v in entries.items()},
        'logical_failures': {k: v['decision_errors'][3] for k, v in entries.items()},
        'residual_syndrome': {k: v['decision_errors'][2] for k, v in entries.items()},
        'failed': {k: v['decision_errors'][2] + v['decision_errors'][3] for k, v in entries.items()},
        'ufw_scale0_over_uf': entries['ufw_scale0']['ms_median'] / entries['uf']['ms_median'],
        'entries': entries,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps({k: result[k] for k in ('ms', 'logical_failures', 'residual_syndrome',
                                             'failed', 'ufw_scale0_over_uf')}))
    residual = {k: v for k, v in result['residual_syndrome'].items() if k != 'bposd' and v}
    if residual or not entries['ufw_scale0']['same_bits_as_uf']:
        raise SystemExit(f'residual syndromes {residual}, ufw(scale = 0) == uf: '
                         f"{entries['ufw_scale0']['same_bits_as_uf']}")


if __name__ == '__main__':
    main()
