"""Worker for tests/test_gpu_osd_hi.py::test_debug_library_runs_osd_clean (a child process with
GNND_LIB pointing at libgnnd_debug.so): (cs, 10) and (e, 8) on toric-7 and the rank-deficient BCH
graph, then one JSON line with the debug flags and whether the bits equal the numpy reference."""
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
import osd_hi_cases as hc  # noqa: E402

CASES = (('toric_7', 9, 'float64', 'zero'), ('bch_dup', 4, 'float32', 'hard'))


def main():
    dev = torch.device('cuda', 0)
    equal = {}
    for code, B, dtype, base in CASES:
        H, x, p = hc.inputs(code, B, dtype)
        g = gd.TannerGraph(H, device=dev)
        xd, pd = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(p.copy()).to(dev)
        for method, order in (('cs', 10), ('e', 8)):
            got = ops.osd(g, xd, pd, base, method, order)
            ref = hc.reference(code, B, dtype, base, method, order)
            equal[f'{code}_{method}'] = bool(all(
                np.array_equal(a.cpu().numpy().reshape(r.shape), r) for a, r in zip(got, ref)))
    f = ctypes.c_uint32()
    _lib.call('gnnd_debug_flags', ctypes.byref(f))
    print(json.dumps({'debug': _lib.get().gnnd_debug_enabled(), 'flags': int(f.value),
                      'equal': equal}))


if __name__ == '__main__':
    main()
