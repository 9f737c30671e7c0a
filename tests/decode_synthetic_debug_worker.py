"""The device side of tests/test_gpu_decode_synthetic.py: the fused decoders (gnnd_decode) on the
irregular graphs of tests/synthetic_codes.py.  The tests call model_of(), decode() and plan() case
by case on the release library.  As a program (a child process with GNND_LIB pointing at
libgnnd_debug.so, test_debug_library_runs_every_case_clean) it queries the plan and decodes every
case of synthetic_codes.DECODE_PLAN_CASES at its smallest batch for T in DECODE_ITERS, saves the
outputs to the .npz file named on the command line for the parent to compare bit for bit with the
release run, and prints one JSON line with the plans and gnnd_debug_flags (which synchronises the
device and collects every translation unit's bounds-check word)."""
import os
import sys
import zlib

import numpy as np
import torch

from debug_child import ROOT, report  # first: it puts the package on sys.path
import gnndecode as gd  # noqa: E402
from gnndecode import ops  # noqa: E402
import synthetic_codes as sc  # noqa: E402

DEV = 'cuda:0'
DTYPES = {'float32': torch.float32, 'float64': torch.float64, 'bfloat16': torch.bfloat16}
# the checkpoints the golden files carry that fit any graph (MLP weights only)
SHIPPED = {'cgnni': 'cgnni_bch', 'v24': 'v24_toric5'}

_GRAPHS = {}


def graph_of(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = gd.TannerGraph(sc.decode_matrix(name), device=DEV)
    return _GRAPHS[name]


def model_of(name, model, T, weights='random'):
    """(module on the device, its weights as numpy arrays).  'random': the
    module's seeded default init (nbp and v10 start at all ones: perturbed so every weight counts);
    'shipped': the reference checkpoint of tests/golden."""
    torch.manual_seed(zlib.crc32(f'{name}-{model}'.encode()) & 0xffff)
    m = gd.MODELS[model](T, sc.decode_matrix(name))
    if weights == 'shipped':
        z = np.load(os.path.join(ROOT, 'tests', 'golden', SHIPPED[model] + '.npz'))
        m.load_state_dict({k[2:]: torch.from_numpy(np.array(z[k])) for k in z.files
                           if k.startswith('w/')})
    elif model in ('nbp', 'v10'):
        with torch.no_grad():
            for k, p in m.named_parameters():
                if k == 'alpha':
                    p.fill_(0.3)
                else:
                    p.mul_(1 + 0.25 * torch.randn(p.shape, dtype=p.dtype))
    w = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    return m.to(DEV).eval(), w


def decode(name, m, x, dtype, T=None):
    """gnnd_decode of x (numpy [B * N, 1]) in `dtype` -> torch tensor on the device."""
    dt = DTYPES[dtype]
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dt)
    wdt = torch.float32 if dt == torch.bfloat16 else dt
    return ops.decode(graph_of(name), m.kind, xd, m.Nc if T is None else T,
                      m.prepared_weights(wdt, torch.device(DEV)))


def plan(name, model, dtype):
    return ops.decode_plan(graph_of(name), model, DTYPES[dtype])


def key(case, T):
    return '-'.join(str(a) for a in case[:3]) + f'-T{T}'


def smallest_batch(case):
    """The debug run's batch: one codeword more than a tile of a light model (a full tile and a
    ragged one), 3 for decoder_v2_4 and decoder_v3_0 (one codeword per workgroup)."""
    name, model, dtype = case[:3]
    if model in ('v24', 'v30'):
        return 3
    return ops.decode_tile(graph_of(name), model, DTYPES[dtype])[0] + 1


def run_case(case, T):
    name, model, dtype = case[:3]
    m, _ = model_of(name, model, T)
    x = sc.decode_inputs(name, model, smallest_batch(case))
    return decode(name, m, x, dtype).cpu().numpy().reshape(-1)


def main():
    arrays, plans = {}, {}
    for case in sc.DECODE_PLAN_CASES:
        p = plan(*case[:3])
        plans['-'.join(case[:3])] = [p['kernel'], p['items_per_lane'], p['var_group']]
        for T in sc.DECODE_ITERS:
            arrays[key(case, T)] = run_case(case, T)
    np.savez(sys.argv[1], **arrays)
    report(cases=len(sc.DECODE_PLAN_CASES), plans=plans)


if __name__ == '__main__':
    main()
