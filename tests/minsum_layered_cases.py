"""Shared by tests/test_minsum_layered_cpu.py and tests/test_gpu_minsum_layered.py: the numpy
statement of the layered min-sum definition (include/gnnd.h, gnnd_minsum_layered), a numpy greedy
layer rule, and the seeded inputs of tests/minsum_cases.py, unchanged (all-equal priors, exact
ties, 0.0 and -0.0, early exits at several depths next to codewords that never converge)."""
import functools

import numpy as np

import minsum_cases as mc
from minsum_cases import CODES, PARAMS, code_matrix, inputs  # noqa: F401  (re-exported)

# (code, B) of the host-mirror and kernel comparisons: toric-5 B = 67 is not a multiple of the 4
# codewords a wave holds; toric-7 takes the whole wave; LDPC two codewords per wave
SHAPES = (('toric_5', 67), ('toric_7', 9), ('bch_63_45', 9), ('ldpc_648_324', 5))
# the parameter sets run on every code (every set of PARAMS runs on toric-5)
COMMON_PARAMS = (PARAMS[0], PARAMS[2])
# layers and their sizes on the shipped codes
LAYER_SIZES = {'toric_5': [16, 16, 8, 8], 'toric_7': [36, 36, 12, 12], 'bch_63_45': [1] * 18,
               'ldpc_648_324': [27] * 12}


@functools.lru_cache(maxsize=None)
def layer_of_check(code):
    """The rule of the definition, literally: checks in ascending c, layer(c) the smallest k such
    that no earlier check of layer k shares a variable with c.  int32 [C], read-only."""
    H = code_matrix(code).astype(bool)
    C = H.shape[1]
    layer = np.zeros(C, np.int32)
    for c in range(C):
        k = 0
        while any(layer[d] == k and (H[:, d] & H[:, c]).any() for d in range(c)):
            k += 1
        layer[c] = k
    layer.setflags(write=False)
    return layer


def layered_order(code):
    """The checks sorted by (layer, c)."""
    lay = layer_of_check(code)
    return np.lexsort((np.arange(lay.size), lay))


def permuted_order(code, how):
    """The layered order with the checks of every layer reversed ('reversed') or shuffled
    ('shuffled'): the layers keep their sequence."""
    lay = layer_of_check(code)
    rng = np.random.default_rng(5)
    out = []
    for k in range(int(lay.max()) + 1):
        cs = np.nonzero(lay == k)[0]
        out.append(cs[::-1] if how == 'reversed' else rng.permutation(cs))
    return np.concatenate(out)


def _check_step(T, qc, tc, a, b):
    """gnnd_minsum's check step over the messages qc of one check, literally: every edge takes
    the parity and the minimum over the OTHER edges; a * m - b is a product, then a difference,
    each rounded to T once."""
    zero = T(0)
    n = qc.size
    neg = qc < zero
    mags = np.abs(qc)
    others = np.where(np.eye(n, dtype=bool), T(np.inf), mags[None, :])
    m = others.min(axis=1)
    par = (int(tc) + int(neg.sum()) - neg.astype(np.int64)) & 1
    d = (a * m).astype(T) - b
    assert d.dtype == T
    mag = np.where(d > zero, d, zero)
    return np.where(par == 1, -mag, mag).astype(T)


def layered_ref(code, l, t, alpha, beta, iters, early_stop, order=None, parallel=False):
    """One codeword, the literal serial loop of the definition in l's dtype: l [V] priors, t [C]
    0/1 target syndrome -> (L [V], iterations executed, status).  Every operation is a numpy
    operation on values of the dtype, so each rounds once.  `order`: the check sequence (default
    the layered order).  parallel=True runs every layer as the kernel does: all its checks read
    L and r first, then all write."""
    T = l.dtype.type
    ev, ec, chk, vptr = mc._tables(code)
    a, b = T(alpha), T(beta)
    zero = T(0)
    L = l.copy()
    r = np.zeros(ev.size, l.dtype)
    lay = layer_of_check(code)
    if order is None:
        order = layered_order(code)
    groups = ([order[lay[order] == k] for k in range(int(lay.max()) + 1)] if parallel
              else [[c] for c in order])
    it, ok = 0, False
    while it < iters:
        it += 1
        for grp in groups:
            new = []
            for c in grp:
                ce = chk[c]
                q = L[ev[ce]] - r[ce]
                assert q.dtype == l.dtype
                new.append((ce, q, _check_step(T, q, t[c], a, b)))
            for ce, q, rn in new:
                L[ev[ce]] = q + rn
                r[ce] = rn
        h = (L < zero).astype(np.int64)
        syn = np.array([h[ev[ce]].sum() & 1 for ce in chk])
        ok = bool((syn == t).all())
        if early_stop and ok:
            break
    return L, it, 0 if ok else 1


def _batch(code, B, dtype, params, **kw):
    alpha, beta, iters, early_stop = params
    H, x = inputs(code, B, dtype)
    V, C = H.shape
    xb = x.reshape(B, V + C)
    t = (xb[:, V:] < 0).astype(np.int64)
    res = [layered_ref(code, xb[b, :V], t[b], alpha, beta, iters, early_stop, **kw)
           for b in range(B)]
    return (np.concatenate([r[0] for r in res]), np.array([r[1] for r in res], np.int32),
            np.array([r[2] for r in res], np.int32))


@functools.lru_cache(maxsize=None)
def reference(code, B, dtype, params):
    """(llr [B*V] in dtype, iters_used [B] int32, status [B] int32) of the numpy statement on
    minsum_cases.inputs(code, B, dtype), read-only, with minsum_cases.reference's conditions: a
    batch of B >= 5 holds both statuses, and under early stop at least two distinct iteration
    counts with the unconverged codewords at `iters`, so that no seed hides either path."""
    llr, its, status = _batch(code, B, dtype, params)
    mc.assert_coverage(code, B, dtype, params, its, status)
    for arr in (llr, its, status):
        arr.setflags(write=False)
    return llr, its, status


def variant(code, B, dtype, params, how):
    """The statement with another check sequence: 'reversed' / 'shuffled' inside every layer,
    'parallel' (read-all-then-write-all per layer), or 'ascending' (a plain sweep in ascending c,
    ignoring the layers)."""
    if how == 'parallel':
        return _batch(code, B, dtype, params, parallel=True)
    if how == 'ascending':
        return _batch(code, B, dtype, params, order=np.arange(code_matrix(code).shape[1]))
    return _batch(code, B, dtype, params, order=permuted_order(code, how))
