"""Shared by tests/test_osd_cpu.py and tests/test_gpu_osd.py: the numpy statement of the OSD-0
definition (include/gnnd.h, gnnd_osd0) and seeded inputs with the content the contract is about:
exact ties, entries saturated to 0.0 / 1.0 and one NaN per batch."""
import functools

import numpy as np

import gnndecode as gd
import synthetic_codes

CODES = ('toric_5', 'toric_7', 'bch_63_45', 'ldpc_648_324')


def osd0_ref(H, t, p, hard):
    """One codeword: H [V, C] 0/1, t [C] target syndrome, p [V] soft output -> (ehat, status)."""
    V, C = H.shape
    z = (p > 0.5).astype(np.uint8) if hard else np.zeros(V, np.uint8)
    key = -np.abs(p - 0.5) if hard else p.copy()
    key = np.where(np.isnan(key), -np.inf, key)
    order = np.lexsort((np.arange(V), -key))
    A = H.T.astype(np.uint8).copy()
    s = (t ^ (A @ z % 2)).astype(np.uint8)
    used = np.zeros(C, bool)
    piv = []
    for j in order:
        rows = np.nonzero(A[:, j] & ~used)[0]
        if rows.size == 0:
            continue
        r = rows[0]
        used[r] = True
        piv.append((r, j))
        m = A[:, j].astype(bool)
        m[r] = False
        A[m] ^= A[r]
        s[m] ^= s[r]
        if used.all():
            break
    if s[~used].any():
        return z, 1
    e = np.zeros(V, np.uint8)
    for r, j in piv:
        e[j] = s[r]
    return z ^ e, 0


def ref_batch(H, x, p, hard):
    """osd0_ref over a batch: x [B*N], p [B*V] -> (ehat [B, V] uint8, status [B] int32)."""
    V, C = H.shape
    pb = p.reshape(-1, V)
    t = (x.reshape(-1, V + C)[:, V:] < 0).astype(np.uint8)
    out = [osd0_ref(H, t[b], pb[b], hard) for b in range(pb.shape[0])]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


@functools.lru_cache(maxsize=None)
def code_matrix(code):
    """H [V, C] of a shipped code, of a synthetic graph of tests/synthetic_codes.py, or 'bch_dup':
    BCH(63,45) with check 0 appended again as check 18 (C = 19, rank 18)."""
    if code == 'bch_dup':
        H = gd.codes.bch_63_45()
        return np.concatenate([H, H[:, :1]], axis=1).copy()
    if synthetic_codes.is_synthetic(code):
        return synthetic_codes.matrix(code)
    return gd.codes.get_code(code)


def soft_outputs(V, B, dtype, rng):
    """p [B, V] in (0, 1) with, per codeword: two groups of exact ties (0.25 / 0.75 also tie in
    the hard base's key), entries saturated to exactly 0.0 and 1.0, and in codeword 0 one NaN."""
    p = rng.random((B, V)).astype(dtype)
    for b in range(B):
        idx = rng.permutation(V)
        p[b, idx[0:5]] = 0.25
        p[b, idx[5:9]] = 0.75
        p[b, idx[9:13]] = p[b, idx[13]]
        p[b, idx[14:20]] = 0.0
        p[b, idx[20:26]] = 1.0
    p[0, rng.integers(V)] = np.nan
    return p


@functools.lru_cache(maxsize=None)
def inputs(code, B, dtype, seed=0):
    """(H, x [B*N], p [B*V]) in `dtype` ('float32' / 'float64'), read-only.  Toric check rows carry
    (-1)^(H^T e) of a random error at flip probability 0.08, and so do the synthetic graphs',
    classical ones 0; 'bch_dup' carries random +-1 with t_0 != t_18 in even codewords and
    t_0 == t_18 in odd ones.  'syn_tall' (more checks than variables, full column rank) has one
    random target flipped in every odd codeword, which leaves the syndrome outside the image of
    H^T unless that unit vector happens to lie in it (reference() asserts that some do fail)."""
    H = code_matrix(code)
    V, C = H.shape
    rng = np.random.default_rng([seed, B, V, C, dtype == 'float64'])
    p = soft_outputs(V, B, np.dtype(dtype), rng)
    x = np.empty((B, V + C), np.dtype(dtype))
    x[:, :V] = rng.normal(size=(B, V))
    if code.startswith('toric') or synthetic_codes.is_synthetic(code):
        e = (rng.random((B, V)) < 0.08).astype(np.int64)
        x[:, V:] = 1 - 2 * ((e @ H.astype(np.int64)) % 2)
        if code == 'syn_tall':
            for b in range(1, B, 2):
                x[b, V + rng.integers(C)] *= -1
    elif code == 'bch_dup':
        x[:, V:] = 1 - 2 * rng.integers(0, 2, (B, C))
        x[:, V + 18] = x[:, V]
        x[0::2, V + 18] *= -1
    else:
        x[:, V:] = 0
    x, p = x.reshape(-1), p.reshape(-1)
    x.setflags(write=False)
    p.setflags(write=False)
    return H, x, p


@functools.lru_cache(maxsize=None)
def reference(code, B, dtype, base, seed=0):
    H, x, p = inputs(code, B, dtype, seed)
    ehat, status = ref_batch(H, x, p, base == 'hard')
    if code == 'syn_tall' and B >= 2:
        assert not status[0::2].any() and status[1::2].any(), (B, dtype, base, status.tolist())
    ehat.setflags(write=False)
    status.setflags(write=False)
    return ehat, status


def satisfied(H, x, ehat):
    """Per codeword: H^T ehat == t."""
    V, C = H.shape
    t = (x.reshape(-1, V + C)[:, V:] < 0).astype(np.int64)
    return (((ehat.reshape(-1, V).astype(np.int64) @ H.astype(np.int64)) % 2) == t).all(axis=1)
