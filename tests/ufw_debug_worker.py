"""Worker for tests/test_gpu_ufw.py::test_debug_library_runs_ufw_clean (a child process with
GNND_LIB pointing at libgnnd_debug.so): toric-5 B = 67 (fp64, llr), ring-130 B = 67 (fp32, priors),
two_comp B = 67 (fp64, llr, then three hand-made codewords of which two have no solution) through
ops.ufw, the scale = 0 anchor against ops.uf, and ops.belief_find on toric-5 against its host
mirror; then one JSON line with the debug flags and whether every output equals the independent
statement.  The kernel's index checks (labels, endpoints, parent edges, depths) are recorded in its
own translation unit's word, read with gnnd_debug_take_ufw after gnnd_debug_flags has synchronised
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
import ufw_cases as wc  # noqa: E402


def main():
    dev = torch.device('cuda', 0)
    equal = {}

    def same(out, ref):
        return all(bool(np.array_equal(o.cpu().numpy().reshape(-1), r)) for o, r in zip(out, ref))

    def on_dev(a):
        return torch.from_numpy(np.array(a)).to(dev)

    for shape, dtype, with_llr in (('toric_5', 'float64', True), ('ring_130', 'float32', False),
                                   ('two_comp', 'float64', True)):
        H, x, llr = wc.inputs(shape, wc.B_ALL, dtype)
        g = gd.TannerGraph(H, device=dev)
        out = ops.ufw(g, on_dev(x), on_dev(llr) if with_llr else None, wc.SCALE, wc.WMAX)
        equal[shape] = same(out, wc.reference(shape, wc.B_ALL, dtype, with_llr))
        anchor = ops.ufw(g, on_dev(x), on_dev(llr), 0.0, 32)
        equal[shape + '/anchor'] = same(anchor[:4], ops.uf_host(H, x))
    V, C = H.shape
    x = np.ones((3, V + C))
    x[0, V + 2] = -1
    x[1, V + 1] = x[1, V + 3] = -1
    x[2, V + 0] = x[2, V + 1] = x[2, V + 4] = -1
    l3 = llr[:3 * V]
    r = wc.ufw_ref(H, x.reshape(-1), l3)
    out = ops.ufw(g, on_dev(x.reshape(-1)), on_dev(l3), wc.SCALE, wc.WMAX)
    equal['two_comp/unsatisfiable'] = same(out, wc.as_tuple(r, 'float64')) and \
        r['status'].tolist() == [1, 0, 1]
    H, x = wc.bf_inputs('float64')
    g = gd.TannerGraph(H, device=dev)
    args = (wc.BF_ITERS, wc.BF_ALPHA, wc.BF_BETA, True, wc.SCALE, wc.WMAX)
    equal['belief_find'] = same(ops.belief_find(g, on_dev(x), *args),
                                ops.belief_find_host(H, x, *args))
    f = ctypes.c_uint32()
    _lib.call('gnnd_debug_flags', ctypes.byref(f))
    flags = int(f.value)
    for unit in ('ufw', 'minsum'):
        take = getattr(_lib.get(), 'gnnd_debug_take_' + unit)
        take.restype = ctypes.c_uint
        take.argtypes = []
        flags |= int(take())
    print(json.dumps({'debug': _lib.get().gnnd_debug_enabled(), 'flags': flags, 'equal': equal}))


if __name__ == '__main__':
    main()
