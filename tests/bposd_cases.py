"""Shared by tests/test_bposd_cpu.py and tests/test_gpu_bposd.py: the numpy statement of the gated
OSD and BP+OSD definitions (include/gnnd.h, gnnd_osd_gated / gnnd_bposd), composed from the
statements of tests/osd_hi_cases.py (gnnd_osd) and tests/minsum_cases.py (gnnd_minsum), and the
gates the tests run: all zeros, all ones, alternating, and the min-sum status of
minsum_cases.inputs."""
import functools

import numpy as np

import minsum_cases as mc
import minsum_layered_cases as lc
import osd_cases as oc
import osd_hi_cases as ohc

GATES = ('zeros', 'ones', 'alt', 'minsum')
METHODS = (('osd0', 0), ('cs', 10), ('e', 8))
# (code, B) of the host-mirror and kernel comparisons
SHAPES = (('toric_5', 67), ('toric_7', 9), ('bch_63_45', 33), ('ldpc_648_324', 3))


def bp_params(code):
    """(alpha, beta, iters, early_stop) of the BP stage: the sets tests/test_minsum_cpu.py runs on
    each code, for which minsum_cases.reference holds both statuses."""
    return mc.PARAMS[2] if code.startswith('bch') else mc.PARAMS[0]



@functools.lru_cache(maxsize=None)
def gate(code, B, dtype, name):
    """int32 [B], read-only.  'alt' gates the odd codewords; 'minsum' is the status of the numpy
    min-sum statement on minsum_cases.inputs(code, B, dtype) with bp_params(code) (for
    B >= 5 minsum_cases asserts that it holds both values)."""
    if name == 'zeros':
        g = np.zeros(B, np.int32)
    elif name == 'ones':
        g = np.ones(B, np.int32)
    elif name == 'alt':
        g = (np.arange(B) % 2).astype(np.int32)
    else:
        assert name == 'minsum'
        g = mc.reference(code, B, dtype, bp_params(code))[2].copy()
    if name in ('alt', 'minsum') and B >= 5:
        assert set(g.tolist()) == {0, 1}, (code, B, dtype, name)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def llr_input(code, B, dtype):
    """An LLR array [B*V] for the pass-through of the gated-OSD cases, unrelated to the soft
    output of osd_cases.inputs on purpose (the two hard decisions differ, so a test tells them
    apart): seeded normals with, per codeword, exact 0.0 and -0.0 (not negative) and one NaN
    (not negative)."""
    V = oc.code_matrix(code).shape[0]
    rng = np.random.default_rng([7, B, V, dtype == 'float64'])
    L = rng.normal(size=(B, V)).astype(dtype)
    for b in range(B):
        idx = rng.permutation(V)
        L[b, idx[0:2]] = 0.0
        L[b, idx[2]] = -0.0
        L[b, idx[3]] = np.nan
    L = L.reshape(-1)
    L.setflags(write=False)
    return L


def hard_decision(pred, llr):
    """The pass-through decision, uint8: llr < 0 where an llr is given, else pred > 0.5 (both
    false for a NaN, the first false for -0.0)."""
    with np.errstate(invalid='ignore'):
        return ((llr < 0) if llr is not None else (pred > 0.5)).astype(np.uint8)


def compose(full, g, pred, llr, V):
    """The definition: rows of the ungated result `full` = (ehat [B, V], status, choice) where the
    gate is set, the hard decision, status 0 and choice -1 elsewhere."""
    ehat, status, choice = (a.copy() for a in full)
    h = hard_decision(pred, llr).reshape(-1, V)
    off = g == 0
    ehat[off] = h[off]
    status[off] = 0
    choice[off] = -1
    return ehat, status, choice


def gated_reference(code, B, dtype, base, method, order, gate_name, with_llr):
    """(ehat [B, V] uint8, status, choice int32 [B]) of gnnd_osd_gated on osd_cases.inputs(code, B,
    dtype) with gate(code, B, dtype, gate_name) and llr_input (or no llr)."""
    H, x, p = oc.inputs(code, B, dtype)
    full = ohc.reference(code, B, dtype, base, method, order)
    return compose(full, gate(code, B, dtype, gate_name), p,
                   llr_input(code, B, dtype) if with_llr else None, H.shape[0])


def bposd_reference(code, B, dtype, pred, base, method, order, schedule='flooding'):
    """(ehat [B, V] uint8, status, choice, iters_used, bp_status, llr) of gnnd_bposd (of
    gnnd_bposd_layered with schedule='layered': the BP stage is then the statement of
    tests/minsum_layered_cases.py) on
    minsum_cases.inputs(code, B, dtype) with bp_params(code).  `pred` [B*V] is the soft
    output the implementation under test returned: it is outside the bit-exact contract (the
    exponential is the library's) and the OSD stage orders its columns by it, so the statement
    takes it as given; the tests hold it to minsum_cases.pred_tolerance separately."""
    H, x = mc.inputs(code, B, dtype)
    if schedule == 'layered':
        llr, its, st = lc.reference(code, B, dtype, bp_params(code))
    else:
        assert schedule == 'flooding'
        llr, its, st = mc.reference(code, B, dtype, bp_params(code))
    full = ohc.ref_batch(H, x, pred, base == 'hard', method, order)
    ehat, status, choice = compose(full, st, pred, llr, H.shape[0])
    return ehat, status, choice, its, st, llr


def tiny_llr_inputs(dtype):
    """toric-5, B = 67: minsum_cases.inputs with the variable rows scaled by 2^-100 (exact: the
    same signs, iterations and statuses at alpha = 1, beta = 0) -> (H, x, x_scaled)."""
    H, x = mc.inputs('toric_5', 67, dtype)
    V, C = H.shape
    xs = x.reshape(-1, V + C).copy()
    xs[:, :V] *= np.dtype(dtype).type(2.0 ** -100)
    return H, x, xs.reshape(-1)


TINY_BP = (1.0, 0.0, 12, 1)


@functools.lru_cache(maxsize=None)
def _check_inputs():
    """The conditions on the seeded inputs, checked once: on toric-5 B = 67 ('cs', 10, zero base)
    every mixed gate selects at least one codeword whose chosen candidate is not OSD-0's, in both
    dtypes (seed 0 of osd_cases.inputs / minsum_cases.inputs gives them: no other seed needed)."""
    for dtype in ('float32', 'float64'):
        choice = ohc.reference('toric_5', 67, dtype, 'zero', 'cs', 10)[2]
        for name in ('alt', 'minsum'):
            g = gate('toric_5', 67, dtype, name)
            assert (choice[g != 0] != 0).any(), (dtype, name)
    return True


_check_inputs()
