"""Worker for tests/test_gpu_bposd.py::test_debug_library_runs_bposd_clean (a child process with
GNND_LIB pointing at libgnnd_debug.so): bposd and osd_gated on toric-5 B = 67 and osd_gated on the
rank-deficient BCH graph, then one JSON line with the debug flags and whether the bits equal the
host mirrors' (for bposd's OSD stage: the mirror on the soft output the device returned).  The gated kernels record their index checks (list entries in [0, B), count <= B)
in the OSD translation unit's word, which gnnd_debug_flags collects; the min-sum stage's word is
read with gnnd_debug_take_minsum."""
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
import bposd_cases as bc  # noqa: E402
import minsum_cases as mc  # noqa: E402
import osd_cases as oc  # noqa: E402


def _eq(got, ref):
    return bool(all(np.array_equal(a.cpu().numpy().reshape(-1), r) for a, r in zip(got, ref)))


def main():
    dev = torch.device('cuda', 0)
    equal = {}
    alpha, beta, iters, early = bc.bp_params('toric_5')
    H, x = mc.inputs('toric_5', 67, 'float64')
    g = gd.TannerGraph(H, device=dev)
    got = ops.bposd(g, torch.from_numpy(x.copy()).to(dev), iters, alpha, beta, True, 'zero', 'cs', 10)
    ref = ops.bposd_host(H, x, iters, alpha, beta, True, 'zero', 'cs', 10)
    # the OSD stage orders by pred, which is each library's own exponential: its mirror runs on
    # the pred the device returned
    n = lambda t: t.cpu().numpy().reshape(-1)
    osd_ref = ops.osd_gated_host(H, x, n(got[5]), n(got[4]), 'zero', 'cs', 10, llr=n(got[6]))
    equal['toric_5_bposd'] = _eq(got[3:5] + got[6:], ref[3:5] + ref[6:]) and _eq(got[:3], osd_ref)
    for code, B, dtype, base, gate in (
            ('toric_5', 67, 'float32', 'zero', bc.gate('toric_5', 67, 'float32', 'alt')),
            ('bch_dup', 4, 'float32', 'hard', np.array([1, 0, 1, 1], np.int32))):
        H, x, p = oc.inputs(code, B, dtype)
        g = gd.TannerGraph(H, device=dev)
        L = bc.llr_input(code, B, dtype)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)
        ok = True
        for method, order in (('cs', 10), ('e', 8)):
            got = ops.osd_gated(g, d(x), d(p), d(gate), base, method, order, llr=d(L))
            ok = ok and _eq(got, ops.osd_gated_host(H, x, p, gate, base, method, order, llr=L))
        equal[f'{code}_gated'] = ok
    f = ctypes.c_uint32()
    _lib.call('gnnd_debug_flags', ctypes.byref(f))
    take = _lib.get().gnnd_debug_take_minsum
    take.restype = ctypes.c_uint
    take.argtypes = []
    print(json.dumps({'debug': _lib.get().gnnd_debug_enabled(), 'flags': int(f.value) | int(take()),
                      'equal': equal}))


if __name__ == '__main__':
    main()
