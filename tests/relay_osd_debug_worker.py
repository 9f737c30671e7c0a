"""Worker for tests/test_gpu_relay_osd.py::test_debug_library_runs_relay_osd_clean (a child process
with GNND_LIB pointing at libgnnd_debug.so): toric-5 B = 9 (fp64, six legs) and LDPC B = 3 (fp32,
the short legs that run out) through ops.relay_soft and ops.relay_osd in both soft modes, then one
JSON line with the debug flags and whether soft and the relay outputs equal the numpy statement.
The relay kernel's index checks are recorded in its own translation unit's word, read with
gnnd_debug_take_relay after gnnd_debug_flags has synchronised the device and collected the other
units'."""
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
import relay_cases as rc  # noqa: E402
import relay_osd_cases as roc  # noqa: E402


def main():
    dev = torch.device('cuda', 0)
    equal = {}
    for code, B, dtype, params in (('toric_5', 9, 'float64', rc.PARAMS[1]),
                                   ('ldpc_648_324', 3, 'float32', rc.PARAMS[3])):
        legs, iters0, iters_leg, S = params
        H, x = roc.inputs(code, B, dtype, params)
        g = gd.TannerGraph(H, device=dev)
        xd = torch.from_numpy(x.copy()).to(dev)
        gm = torch.from_numpy(rc.gammas(g.V, params, dtype).copy()).to(dev)
        ref = roc.reference(code, B, dtype, params)
        ok = True
        for mode in roc.MODES:
            out = ops.relay_soft(g, xd, gm, iters0, iters_leg, S, rc.ALPHA, rc.BETA, soft=mode)
            ok &= bool(np.array_equal(out[1].cpu().numpy().reshape(-1), ref['soft_' + mode]))
            ok &= all(bool(np.array_equal(t.cpu().numpy().reshape(-1), ref[k]))
                      for t, k in zip(out[2:], rc.OUTPUTS))
            both = ops.relay_osd(g, xd, gm, iters0, iters_leg, S, rc.ALPHA, rc.BETA, soft=mode,
                                 base=roc.base_of(code))
            ok &= bool(torch.equal(both[3], out[0]) and torch.equal(both[6], out[5]))
        equal[code] = ok
    f = ctypes.c_uint32()
    _lib.call('gnnd_debug_flags', ctypes.byref(f))
    take = _lib.get().gnnd_debug_take_relay
    take.restype = ctypes.c_uint
    take.argtypes = []
    print(json.dumps({'debug': _lib.get().gnnd_debug_enabled(), 'flags': int(f.value) | int(take()),
                      'equal': equal}))


if __name__ == '__main__':
    main()
