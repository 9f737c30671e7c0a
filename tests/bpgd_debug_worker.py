"""Worker for tests/test_gpu_bpgd.py::test_debug_library_runs_bpgd_clean (a child process with
GNND_LIB pointing at libgnnd_debug.so): toric-5 B = 67 (fp64, the working set and the
most-reliable set) and syn_hub B = 9 (fp32, the set that decimates every variable) through
ops.bpgd, then one JSON line with the debug flags and whether every contract output equals the
numpy reference.  The kernel's index checks, the pick's v* among them, are recorded in its own
translation unit's word, read with gnnd_debug_take_bpgd after gnnd_debug_flags has synchronised
the device and collected the other units'."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'gnn-decode_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import gnndecode as gd  # noqa: E402
from gnndecode import _lib, ops  # noqa: E402
import bpgd_cases as bc  # noqa: E402


def main():
    dev = torch.device('cuda', 0)
    equal = {}
    for code, B, dtype, pset in (('toric_5', 67, 'float64', 1), ('toric_5', 67, 'float64', 2),
                                 ('syn_hub', 9, 'float32', 3)):
        H, x = bc.inputs(code, B, dtype)
        g = gd.TannerGraph(H, device=dev)
        iters0, iters_round, rounds, per_round, pick = bc.params(g.V)[pset]
        xd = torch.from_numpy(x.copy()).to(dev)
        out = ops.bpgd(g, xd, iters0, iters_round, rounds, per_round, pick, bc.CLAMP, bc.ALPHA,
                       bc.BETA)
        ref = bc.reference(code, B, dtype, pset)
        got = dict(zip(('ehat', 'llr', 'pred', 'iters', 'status', 'ndec'), out))
        equal[f'{code}/{pset}'] = all(
            bool(np.array_equal(got[k].cpu().numpy().reshape(-1), ref[k])) for k in bc.OUTPUTS)
    f = ctypes.c_uint32()
    _lib.call('gnnd_debug_flags', ctypes.byref(f))
    take = _lib.get().gnnd_debug_take_bpgd
    take.restype = ctypes.c_uint
    take.argtypes = []
    print(json.dumps({'debug': _lib.get().gnnd_debug_enabled(), 'flags': int(f.value) | int(take()),
                      'equal': equal}))


if __name__ == '__main__':
    main()
