"""Worker for tests/test_gpu_minsum_layered.py::test_debug_library_runs_layered_clean (a child
process with GNND_LIB pointing at libgnnd_debug.so): toric-5 B = 67 (fp64) and LDPC B = 5 (fp32)
through ops.minsum(schedule='layered'), and toric-5 through ops.bposd(schedule='layered'), then one
JSON line with the debug flags and whether llr, iteration counts and statuses equal the numpy
reference.  The layered kernel's index checks (layer slot, check id, edge id, variable id) are
recorded in its own translation unit's word, read with gnnd_debug_take_minsum_layered after
gnnd_debug_flags has synchronised the device and collected the other units'."""
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
import minsum_layered_cases as lc  # noqa: E402


def main():
    dev = torch.device('cuda', 0)
    alpha, beta, iters, early_stop = lc.PARAMS[0]
    equal = {}
    for code, B, dtype in (('toric_5', 67, 'float64'), ('ldpc_648_324', 5, 'float32')):
        H, x = lc.inputs(code, B, dtype)
        g = gd.TannerGraph(H, device=dev)
        xd = torch.from_numpy(x.copy()).to(dev)
        pred, llr, its, status = ops.minsum(g, xd, iters, alpha, beta, bool(early_stop),
                                            schedule='layered')
        ref_llr, ref_it, ref_st = lc.reference(code, B, dtype, lc.PARAMS[0])
        equal[code] = bool(np.array_equal(llr.cpu().numpy().reshape(-1), ref_llr)
                           and np.array_equal(its.cpu().numpy(), ref_it)
                           and np.array_equal(status.cpu().numpy(), ref_st))
        if code == 'toric_5':
            one = ops.bposd(g, xd, iters, alpha, beta, bool(early_stop), schedule='layered')
            equal[code] = equal[code] and bool(torch.equal(one[6], llr)
                                               and torch.equal(one[4], status))
    f = ctypes.c_uint32()
    _lib.call('gnnd_debug_flags', ctypes.byref(f))
    flags = int(f.value)
    for name in ('gnnd_debug_take_minsum_layered', 'gnnd_debug_take_minsum'):
        take = getattr(_lib.get(), name)
        take.restype = ctypes.c_uint
        take.argtypes = []
        flags |= int(take())
    print(json.dumps({'debug': _lib.get().gnnd_debug_enabled(), 'flags': flags, 'equal': equal}))


if __name__ == '__main__':
    main()
