"""The bounds-checked debug build (make debug -> gnndecode/libgnnd_debug.so, -DGNND_DEBUG):
every model / kernel family runs under it without a single index-check violation, and its
outputs equal the release library's (the checks never change values; the generic
propagate kernels accumulate with float atomics, so those sums agree to 1e-12)."""
import os

import pytest

import debug_child
from debug_child import DEBUG_LIB, PKG


def _run(lib):
    """debug_build_worker.py on `lib`; on the debug library through the harness, which asserts
    that it is the debug build and that no index check fired."""
    if lib == DEBUG_LIB:
        return debug_child.run('debug_build_worker.py', timeout=600)
    return debug_child.spawn(lib, 'debug_build_worker.py', timeout=600)


def test_debug_library_exports_and_reports_enabled():
    import ctypes
    if not os.path.exists(DEBUG_LIB):
        pytest.skip('libgnnd_debug.so not built (make -C gnn-decode_amd debug)')
    lib = ctypes.CDLL(DEBUG_LIB)
    assert lib.gnnd_debug_enabled() == 1
    from gnndecode import _lib
    assert _lib.get().gnnd_debug_enabled() == (1 if os.environ.get('GNND_LIB') == DEBUG_LIB else 0)


@pytest.mark.gpu
def test_debug_build_runs_clean_and_matches_release():
    assert os.path.exists(DEBUG_LIB), 'build it: make -C gnn-decode_amd debug'
    dbg = _run(DEBUG_LIB)
    rel = _run(os.path.join(PKG, 'libgnnd.so'))
    assert dbg['debug'] == 1 and rel['debug'] == 0
    assert dbg['flags'] == 0, f"debug index checks fired: bits {dbg['flags']:#x}"
    assert dbg['sums'].keys() == rel['sums'].keys()
    for k, v in dbg['sums'].items():
        if k.endswith('/False'):     # generic propagate: float atomics, order-dependent bits
            assert abs(v - rel['sums'][k]) <= 1e-12 * max(1.0, abs(v)), k
        else:
            assert v == rel['sums'][k], k
