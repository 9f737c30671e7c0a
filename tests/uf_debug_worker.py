"""Worker for tests/test_gpu_uf.py::test_debug_library_runs_uf_clean (a child process with GNND_LIB
pointing at libgnnd_debug.so): toric-5 B = 67 (fp64), ring-130 B = 67 (fp32) and two_comp B = 67
(fp64, then three hand-made codewords of which two have no solution) through ops.uf, then one JSON
line with the debug flags and whether every output equals the independent statement.  The kernel's
index checks (labels, endpoints, parent edges, depths) are recorded in its own translation unit's
word, read with gnnd_debug_take_uf after gnnd_debug_flags has synchronised the device and collected
the other units'."""
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
import uf_cases as uc  # noqa: E402


def main():
    dev = torch.device('cuda', 0)
    equal = {}

    def same(out, ref):
        return all(bool(np.array_equal(o.cpu().numpy().reshape(-1), r)) for o, r in zip(out, ref))

    for shape, dtype in (('toric_5', 'float64'), ('ring_130', 'float32'), ('two_comp', 'float64')):
        H, x = uc.inputs(shape, uc.B_ALL, dtype)
        g = gd.TannerGraph(H, device=dev)
        out = ops.uf(g, torch.from_numpy(x.copy()).to(dev))
        equal[shape] = same(out, uc.reference(shape, uc.B_ALL, dtype))
    V, C = H.shape
    x = np.ones((3, V + C))
    x[0, V + 2] = -1
    x[1, V + 1] = x[1, V + 3] = -1
    x[2, V + 0] = x[2, V + 1] = x[2, V + 4] = -1
    r = uc.uf_ref(H, x.reshape(-1))
    out = ops.uf(g, torch.from_numpy(x.reshape(-1)).to(dev))
    equal['two_comp/unsatisfiable'] = same(out, (r['ehat01'].reshape(-1).astype('float64'),
                                                 r['rounds'], r['status'], r['nfull']))
    f = ctypes.c_uint32()
    _lib.call('gnnd_debug_flags', ctypes.byref(f))
    take = _lib.get().gnnd_debug_take_uf
    take.restype = ctypes.c_uint
    take.argtypes = []
    print(json.dumps({'debug': _lib.get().gnnd_debug_enabled(), 'flags': int(f.value) | int(take()),
                      'equal': equal}))


if __name__ == '__main__':
    main()
