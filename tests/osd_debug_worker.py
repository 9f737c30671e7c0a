"""Worker for tests/test_gpu_osd.py::test_debug_library_runs_osd0_clean (a child process with
GNND_LIB pointing at libgnnd_debug.so): one toric-5 OSD-0 case in both bases, then one JSON line
with the debug flags and whether the bits equal the numpy reference."""
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
import osd_cases as oc  # noqa: E402


def main():
    dev = torch.device('cuda', 0)
    B = 5
    H, x, p = oc.inputs('toric_5', B, 'float64')
    g = gd.TannerGraph(H, device=dev)
    xd, pd = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(p.copy()).to(dev)
    equal = {}
    for base in ('zero', 'hard'):
        ehat, status = ops.osd0(g, xd, pd, base)
        ref_e, ref_s = oc.reference('toric_5', B, 'float64', base)
        equal[base] = bool(np.array_equal(ehat.cpu().numpy().reshape(B, -1), ref_e)
                           and np.array_equal(status.cpu().numpy(), ref_s))
    f = ctypes.c_uint32()
    _lib.call('gnnd_debug_flags', ctypes.byref(f))
    print(json.dumps({'debug': _lib.get().gnnd_debug_enabled(), 'flags': int(f.value),
                      'equal': equal}))


if __name__ == '__main__':
    main()
