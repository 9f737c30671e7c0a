"""Worker for tests/test_gpu_lsd.py::test_debug_library_runs_lsd_clean (a child process with
GNND_LIB pointing at libgnnd_debug.so): toric-5 B = 67 (fp64), syn_c65 B = 9 (fp32: a row in the
second row slot) and syn_tall B = 9 (fp64: unsolvable codewords) through ops.lsd in both bases with
bits_per_step 0 and 1, ops.lsd_gated on toric-5, and ops.bplsd on toric-5 against its host mirror;
then one JSON line with the debug flags and whether every output equals the independent statement.
The kernel's index checks (labels, picks, order entries, graph tables) are recorded in its own
translation unit's word, read with gnnd_debug_take_lsd after gnnd_debug_flags has synchronised the
device and collected the other units'."""
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
import lsd_cases as lc  # noqa: E402
import osd_cases as oc  # noqa: E402


def main():
    dev = torch.device('cuda', 0)
    equal = {}

    def same(out, ref):
        return all(bool(np.array_equal(o.cpu().numpy().reshape(-1), r)) for o, r in zip(out, ref))

    def on_dev(a):
        return torch.from_numpy(np.array(a)).to(dev)

    for code, B, dtype in (('toric_5', 67, 'float64'), ('syn_c65', 9, 'float32'),
                           ('syn_tall', 9, 'float64')):
        H, x, p = oc.inputs(code, B, dtype)
        g = gd.TannerGraph(H, device=dev)
        for base in ('zero', 'hard'):
            for bits in (0, 1):
                out = ops.lsd(g, on_dev(x), on_dev(p), base, bits)
                equal[f'{code}/{base}/{bits}'] = same(
                    out, lc.as_tuple(lc.reference(code, B, dtype, base, bits), dtype))
    H, x, p = oc.inputs('toric_5', 67, 'float64')
    g = gd.TannerGraph(H, device=dev)
    gate = bc.gate('toric_5', 67, 'float64', 'alt')
    equal['gated'] = same(ops.lsd_gated(g, on_dev(x), on_dev(p), on_dev(gate), 'zero', 1),
                          ops.lsd_gated_host(H, x, p, gate, 'zero', 1))
    H, x, args = lc.bp_inputs('float64')
    equal['bplsd'] = same(ops.bplsd(g, on_dev(x), *args, 'zero', 1),
                          ops.bplsd_host(H, x, *args, 'zero', 1))
    f = ctypes.c_uint32()
    _lib.call('gnnd_debug_flags', ctypes.byref(f))
    flags = int(f.value)
    for unit in ('lsd', 'minsum'):
        take = getattr(_lib.get(), 'gnnd_debug_take_' + unit)
        take.restype = ctypes.c_uint
        take.argtypes = []
        flags |= int(take())
    print(json.dumps({'debug': _lib.get().gnnd_debug_enabled(), 'flags': flags, 'equal': equal}))


if __name__ == '__main__':
    main()
