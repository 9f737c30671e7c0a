"""Shared by tests/test_osd_hi_cpu.py and tests/test_gpu_osd_hi.py: the numpy statement of the
higher-order OSD definition (include/gnnd.h, gnnd_osd) on the inputs of tests/osd_cases.py.  The
elimination is OSD-0's, restated here because the candidates need what it leaves behind: the pivot
rows and columns, the reduced syndrome and the reduced matrix."""
import functools

import numpy as np

import osd_cases as oc
from osd_cases import code_matrix, inputs, satisfied  # noqa: F401  (re-exported for the tests)

METHODS = (('osd0', 0), ('cs', 0), ('cs', 10), ('cs', 64), ('e', 0), ('e', 8))


def eliminate(H, t, p, hard):
    """One codeword, everything up to and including OSD-0's Gauss-Jordan -> (z, fail, s_p [R],
    piv_cols [R], free [F], T [R, F]): base vector, failure flag, the reduced syndrome on the
    pivot rows, their pivot columns, the free columns in the column order, and the reduced
    matrix restricted to pivot rows x free columns."""
    V, C = H.shape
    z = (p > 0.5).astype(np.uint8) if hard else np.zeros(V, np.uint8)
    key = -np.abs(p - 0.5) if hard else p.copy()
    key = np.where(np.isnan(key), -np.inf, key)
    order = np.lexsort((np.arange(V), -key))
    A = H.T.astype(np.uint8).copy()
    s = (t ^ (A @ z % 2)).astype(np.uint8)
    used = np.zeros(C, bool)
    piv_rows, piv_cols = [], []
    for j in order:
        rows = np.nonzero(A[:, j] & ~used)[0]
        if rows.size == 0:
            continue
        r = rows[0]
        used[r] = True
        piv_rows.append(r)
        piv_cols.append(j)
        m = A[:, j].astype(bool)
        m[r] = False
        A[m] ^= A[r]
        s[m] ^= s[r]
        if used.all():
            break
    fail = bool(s[~used].any())
    is_piv = np.zeros(V, bool)
    is_piv[piv_cols] = True
    free = np.array([j for j in order if not is_piv[j]], np.int64)
    return z, fail, s[piv_rows], np.array(piv_cols, np.int64), free, A[np.ix_(piv_rows, free)]


def candidate_sets(method, order, F):
    """The candidate list of a method as index tuples into the free list, in candidate order."""
    lam = min(order, F)
    if method == 'osd0':
        return [()]
    if method == 'cs':
        return ([()] + [(i,) for i in range(F)]
                + [(a, b) for a in range(lam) for b in range(a + 1, lam)])
    assert method == 'e'
    return [tuple(i for i in range(lam) if (m >> i) & 1) for m in range(1 << lam)]


def choose(state, method, order):
    """(ehat [V] uint8, status, choice) of one eliminated codeword."""
    z, fail, s_p, piv_cols, free, T = state
    if fail:
        return z, 1, 0
    sets = candidate_sets(method, order, free.size)
    M = np.zeros((len(sets), free.size), np.uint8)          # candidate x free column
    for i, S in enumerate(sets):
        M[i, list(S)] = 1
    # pivot part of every candidate: s xor the XOR of its columns of T
    P = (s_p[None, :] ^ ((M.astype(np.int64) @ T.T.astype(np.int64)) % 2).astype(np.uint8))
    cost = M.sum(1, dtype=np.int64) + P.sum(1, dtype=np.int64)
    best = int(np.argmin(cost))                             # the first minimum: lowest index
    e = np.zeros(z.size, np.uint8)
    e[free] = M[best]
    e[piv_cols] = P[best]
    return z ^ e, 0, best


@functools.lru_cache(maxsize=None)
def eliminated(code, B, dtype, base, seed=0):
    H, x, p = oc.inputs(code, B, dtype, seed)
    V, C = H.shape
    pb = p.reshape(B, V)
    t = (x.reshape(B, V + C)[:, V:] < 0).astype(np.uint8)
    return tuple(eliminate(H, t[b], pb[b], base == 'hard') for b in range(B))


def ref_batch(H, x, p, hard, method, order):
    """Over a batch: x [B*N], p [B*V] -> (ehat [B, V] uint8, status [B], choice [B] int32)."""
    V, C = H.shape
    pb = p.reshape(-1, V)
    t = (x.reshape(-1, V + C)[:, V:] < 0).astype(np.uint8)
    out = [choose(eliminate(H, t[b], pb[b], hard), method, order) for b in range(pb.shape[0])]
    return _stack(out)


def _stack(out):
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out], np.int32))


@functools.lru_cache(maxsize=None)
def reference(code, B, dtype, base, method, order, seed=0):
    """(ehat [B, V] uint8, status [B] int32, choice [B] int32) on oc.inputs(code, B, dtype),
    read-only; the elimination is shared among the methods."""
    res = _stack([choose(s, method, order) for s in eliminated(code, B, dtype, base, seed)])
    for a in res:
        a.setflags(write=False)
    return res


def free_count(code, B, dtype, base):
    """F per codeword."""
    return [s[4].size for s in eliminated(code, B, dtype, base)]


def cost(ehat, p, base):
    """Flips relative to the base vector, per codeword: ehat, p [B, V]."""
    z = (p > 0.5) if base == 'hard' else np.zeros_like(p, bool)
    return ((ehat != 0) ^ z).sum(1)
