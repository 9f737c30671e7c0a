"""Worker for tests/test_gpu_minsum.py::test_debug_library_runs_minsum_clean (a child process with
GNND_LIB pointing at libgnnd_debug.so): toric-5 B = 67 (fp64) and LDPC B = 3 (fp32) through
ops.minsum, then one JSON line with the debug flags and whether llr, iteration counts and statuses
equal the numpy reference.  The min-sum kernel's index checks are recorded in its own translation
unit's word, read with gnnd_debug_take_minsum after gnnd_debug_flags has synchronised the device
and collected the other units'."""
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
import minsum_cases as mc  # noqa: E402


def main():
    dev = torch.device('cuda', 0)
    alpha, beta, iters, early_stop = mc.PARAMS[0]
    equal = {}
    for code, B, dtype in (('toric_5', 67, 'float64'), ('ldpc_648_324', 3, 'float32')):
        H, x = mc.inputs(code, B, dtype)
        g = gd.TannerGraph(H, device=dev)
        xd = torch.from_numpy(x.copy()).to(dev)
        pred, llr, its, status = ops.minsum(g, xd, iters, alpha, beta, bool(early_stop))
        ref_llr, ref_it, ref_st = mc.reference(code, B, dtype, mc.PARAMS[0])
        equal[code] = bool(np.array_equal(llr.cpu().numpy().reshape(-1), ref_llr)
                           and np.array_equal(its.cpu().numpy(), ref_it)
                           and np.array_equal(status.cpu().numpy(), ref_st))
    f = ctypes.c_uint32()
    _lib.call('gnnd_debug_flags', ctypes.byref(f))
    take = _lib.get().gnnd_debug_take_minsum
    take.restype = ctypes.c_uint
    take.argtypes = []
    print(json.dumps({'debug': _lib.get().gnnd_debug_enabled(), 'flags': int(f.value) | int(take()),
                      'equal': equal}))


if __name__ == '__main__':
    main()
