"""Both halves of the debug-library protocol of the tests: a test starts a fresh child process with
GNND_LIB pointing at libgnnd_debug.so (make debug), the child runs its cases and prints one JSON
line, the test reads it.  Workers (tests/*_debug_worker.py) import the first half: the path set-up
a stand-alone child needs, same() / on_dev(), and report(), which asks gnnd_debug_flags alone: it
synchronises the device and returns the OR of every translation unit's index-check word.  Tests
import run()."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'gnn-decode_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
PKG = os.path.join(ROOT, 'gnn-decode_amd', 'gnndecode')
DEBUG_LIB = os.path.join(PKG, 'libgnnd_debug.so')
DEV = 'cuda:0'


# ------------------------------------------------------------------------------------------------
# the worker's half
# ------------------------------------------------------------------------------------------------
def same(out, ref):
    """Every device tensor of `out` equals, flattened, the numpy array of `ref` at its place."""
    import numpy as np
    return all(bool(np.array_equal(o.cpu().numpy().reshape(-1), r)) for o, r in zip(out, ref))


def on_dev(a):
    import numpy as np
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)


def report(**fields):
    """Print the child's one JSON line: whether the library is the debug build, the index-check
    bits of everything run so far, and the caller's fields."""
    import ctypes
    from gnndecode import _lib
    f = ctypes.c_uint32()
    _lib.call('gnnd_debug_flags', ctypes.byref(f))
    print(json.dumps(dict(fields, debug=_lib.get().gnnd_debug_enabled(), flags=int(f.value))))


# ------------------------------------------------------------------------------------------------
# the test's half
# ------------------------------------------------------------------------------------------------
def spawn(lib, script, *args, timeout=300):
    """Run tests/<script> in a fresh child process on the library `lib` -> its JSON line."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', script), *map(str, args)],
                       env=dict(os.environ, GNND_LIB=lib), capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def run(script, *args, timeout=300):
    """spawn() on the debug library; asserts that it is the debug build and that no index check
    fired, and returns the child's fields."""
    assert os.path.exists(DEBUG_LIB), 'build it: make -C gnn-decode_amd debug'
    res = spawn(DEBUG_LIB, script, *args, timeout=timeout)
    assert res['debug'] == 1
    assert res['flags'] == 0, f"debug index checks fired: bits {res['flags']:#x}"
    return res
