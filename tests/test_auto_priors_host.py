"""Host-side checks of the device prior discovery (gnnd_v24_scan_priors,
gnnd_prepare_weights_priors_dev, set_channel_priors('auto')): argument validation returns before
any device work, so these run without a GPU.  The pointers passed are host addresses that are
never dereferenced on the paths tested."""
import ctypes

import pytest
import torch

from gnndecode import _lib

V24, QGNNI = _lib.VARIANT['v24'], _lib.VARIANT['qgnni']


def _fake(n=4):
    """Distinct non-null addresses standing in for device pointers."""
    bufs = [(ctypes.c_double * 8)() for _ in range(n)]
    return bufs, [ctypes.c_void_p(ctypes.addressof(b)) for b in bufs]


def _cap64():
    n = ctypes.c_int64()
    assert _lib.get().gnnd_prepared_weights_count_priors(V24, _lib.F64, 64, ctypes.byref(n)) == _lib.OK
    return n.value


def test_symbols_bound():
    lib = _lib.get()
    for name in ('gnnd_v24_scan_priors', 'gnnd_prepare_weights_priors_dev'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.gnnd_version() == 1


def test_capacity_is_the_64_prior_layout():
    assert _cap64() == 7264 + 64 * 17456 + 34864 == 1159312


def test_prepare_dev_capacity_one_short():
    lib = _lib.get()
    keep, (w, prep, pri, st) = _fake()
    cap = _cap64()
    for short in (cap - 1, 7264, 0, -1):
        assert lib.gnnd_prepare_weights_priors_dev(V24, _lib.F64, w, prep, short, pri, st,
                                                   None) == _lib.ERR_INVALID_ARG
    del keep


def test_prepare_dev_model_and_dtype():
    lib = _lib.get()
    keep, (w, prep, pri, st) = _fake()
    cap = _cap64()
    assert lib.gnnd_prepare_weights_priors_dev(V24, _lib.F32, w, prep, cap, pri, st,
                                               None) == _lib.ERR_UNSUPPORTED
    assert lib.gnnd_prepare_weights_priors_dev(QGNNI, _lib.F64, w, prep, cap, pri, st,
                                               None) == _lib.ERR_UNSUPPORTED
    assert lib.gnnd_prepare_weights_priors_dev(99, _lib.F64, w, prep, cap, pri, st,
                                               None) == _lib.ERR_INVALID_ARG
    assert lib.gnnd_prepare_weights_priors_dev(V24, 7, w, prep, cap, pri, st,
                                               None) == _lib.ERR_INVALID_ARG
    del keep


def test_prepare_dev_null_pointers():
    lib = _lib.get()
    keep, (w, prep, pri, st) = _fake()
    cap = _cap64()
    for args in ((None, prep, cap, pri, st), (w, None, cap, pri, st), (w, prep, cap, None, st),
                 (w, prep, cap, pri, None), (w, w, cap, pri, st)):
        assert lib.gnnd_prepare_weights_priors_dev(V24, _lib.F64, *args, None) == _lib.ERR_INVALID_ARG
    del keep


def test_scan_argument_checks():
    lib = _lib.get()
    keep, (g, x, pri, st) = _fake()
    # dtype first: fp32 / bf16 are not supported, an unknown code is invalid
    assert lib.gnnd_v24_scan_priors(g, _lib.F32, x, 1, pri, st, None) == _lib.ERR_UNSUPPORTED
    assert lib.gnnd_v24_scan_priors(g, _lib.BF16, x, 1, pri, st, None) == _lib.ERR_UNSUPPORTED
    assert lib.gnnd_v24_scan_priors(g, 7, x, 1, pri, st, None) == _lib.ERR_INVALID_ARG
    for args in ((None, _lib.F64, x, 1, pri, st), (g, _lib.F64, None, 1, pri, st),
                 (g, _lib.F64, x, 1, None, st), (g, _lib.F64, x, 1, pri, None),
                 (g, _lib.F64, x, -1, pri, st)):
        assert lib.gnnd_v24_scan_priors(*args, None) == _lib.ERR_INVALID_ARG
    del keep


def test_auto_mode_is_decoder_v2_4_only():
    import gnndecode as gd
    H = gd.codes.toric_code(3)
    with pytest.raises(ValueError):
        gd.MODELS['qgnni'](5, H).set_channel_priors('auto')
    m = gd.MODELS['v24'](2, H)
    m.set_channel_priors('auto')
    assert m._priors == 'auto'
    with pytest.raises(ValueError):
        m.set_channel_priors('automatic')
    m.set_channel_priors((1.5, 2.5))
    assert m._priors == (1.5, 2.5)
    m.set_channel_priors(())
    assert m._priors == ()


def test_ops_reject_cpu_and_fp32_inputs():
    import gnndecode as gd
    assert gd.ops.MAX_PRIORS == 64

    class G:                      # the checks run before the graph handle is touched
        N = 4
    with pytest.raises(RuntimeError):
        gd.ops.scan_channel_priors(G, torch.zeros(8, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        gd.ops.prepare_weights_auto(G, torch.zeros(1283, dtype=torch.float64),
                                    torch.zeros(8, dtype=torch.float64))
