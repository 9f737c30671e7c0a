"""Shared by tests/test_minsum_cpu.py and tests/test_gpu_minsum.py: the numpy statement of the
min-sum definition (include/gnnd.h, gnnd_minsum) and seeded inputs with the content the contract is
about: all-equal priors (every check a tie for the minimum), LLRs quantised to force exact ties,
exact 0.0 and -0.0, and batches that hold early exits at several depths next to codewords that run
to the end without converging."""
import functools

import numpy as np

import gnndecode as gd
import synthetic_codes

CODES = ('toric_5', 'toric_7', 'bch_63_45', 'ldpc_648_324')
# (alpha, beta, iters, early_stop)
PARAMS = ((0.75, 0.0, 12, 1), (1.0, 0.0, 12, 1), (0.8, 0.1, 10, 1), (0.75, 0.0, 3, 0))
TORIC_P = (0.01, 0.04, 0.08, 0.10)
TORIC_FLIP = 0.04
SNR_DB = (1.0, 3.0, 5.0, 7.0)
# added to the seed of a synthetic batch (code, B); searched on the CPU so that the references'
# own coverage conditions (assert_coverage) hold on both schedules and in both dtypes.  Seed 0
# serves syn_hub (B = 1, 11) and syn_sq64 (B = 9) without a search
SYN_SEED = {('syn_wide', 5): 8, ('syn_tall', 9): 4, ('syn_c65', 9): 16}
# Synthetic graphs too easy for min-sum to fail on at TORIC_FLIP: V = 40 or 64 means two or three
# flipped bits per codeword, and on 2 700 codewords each (300 seeds, B = 9) neither schedule left
# one unconverged (syn_tall: every variable sits in 2 to 9 of the 70 checks; syn_sq64: nothing ran
# past 7 iterations).  Their batches hold status 0 only, and assert_coverage states that; the
# early exits at different depths remain.  The unconverged path on a synthetic graph is covered
# by syn_hub, syn_wide and syn_c65.
SYN_EASY = ('syn_tall', 'syn_sq64')


@functools.lru_cache(maxsize=None)
def code_matrix(code):
    """H [V, C] of a shipped code or of a synthetic graph of tests/synthetic_codes.py."""
    if synthetic_codes.is_synthetic(code):
        return synthetic_codes.matrix(code)
    return gd.codes.get_code(code)


def syndrome_style(code):
    """The codes whose inputs carry a measured syndrome on the check rows: the toric family and
    the synthetic graphs."""
    return code.startswith('toric') or synthetic_codes.is_synthetic(code)


@functools.lru_cache(maxsize=None)
def _tables(code):
    """(edge variable [E], edge check [E], edge ids of every check, edge range of every variable),
    edges sorted by (v, c)."""
    H = code_matrix(code)
    ev, ec = np.nonzero(H)
    chk = [np.nonzero(ec == c)[0] for c in range(H.shape[1])]
    vptr = np.concatenate([[0], np.cumsum(np.bincount(ev, minlength=H.shape[0]))])
    return ev, ec, chk, vptr


def minsum_ref(code, l, t, alpha, beta, iters, early_stop):
    """One codeword, the literal loop of the definition in l's dtype: l [V] priors, t [C] 0/1
    target syndrome -> (L [V], iterations executed, status).  Every operation is a numpy operation
    on values of the dtype, so each rounds once; a * m - b is a product, then a difference."""
    T = l.dtype.type
    ev, ec, chk, vptr = _tables(code)
    V = l.size
    a, b = T(alpha), T(beta)
    zero = T(0)
    q = l[ev].copy()
    r = np.empty_like(q)
    L = np.empty_like(l)
    it, ok = 0, False
    while it < iters:
        it += 1
        for c, ce in enumerate(chk):
            qc = q[ce]
            neg = qc < zero
            mag_in = np.abs(qc)
            for j, e in enumerate(ce):
                others = np.arange(ce.size) != j
                par = int(t[c]) ^ (int(neg[others].sum()) & 1)
                m = mag_in[others].min()
                d = T(T(a * m) - b)
                mag = d if d > zero else zero
                r[e] = -mag if par else mag
        for v in range(V):
            s = l[v]
            for e in range(vptr[v], vptr[v + 1]):
                s = T(s + r[e])
            L[v] = s
            for e in range(vptr[v], vptr[v + 1]):
                q[e] = T(s - r[e])
        h = (L < zero).astype(np.int64)
        syn = np.array([h[ev[ce]].sum() & 1 for ce in chk])
        ok = bool((syn == t).all())
        if early_stop and ok:
            break
    return L, it, 0 if ok else 1


def _awgn(rng, B, V, dtype):
    """LLRs 2 y / sigma^2 of the all-zero word (BPSK +1) at SNR_DB[b % 4]; in every codeword six
    LLRs are rounded to multiples of 0.5 and one more pair shares a value (exact ties), two are
    exactly 0.0 and one is -0.0."""
    llr = np.empty((B, V))
    for b in range(B):
        s2 = 10.0 ** (-SNR_DB[b % 4] / 10.0)
        llr[b] = 2.0 * (1.0 + np.sqrt(s2) * rng.normal(size=V)) / s2
    llr = llr.astype(dtype)
    for b in range(B):
        idx = rng.permutation(V)
        llr[b, idx[0:6]] = np.round(llr[b, idx[0:6]] * 2) / 2
        llr[b, idx[6]] = llr[b, idx[7]]
        llr[b, idx[8:10]] = 0.0
        llr[b, idx[10]] = -0.0
    return llr


@functools.lru_cache(maxsize=None)
def inputs(code, B, dtype, seed=0):
    """(H, x [B*N]) in `dtype` ('float32' / 'float64'), read-only.  Toric and synthetic
    (syndrome_style): priors log((1 - p) / p) with p = TORIC_P[b % 4] on every variable of
    codeword b, check rows (-1)^(H^T e) of a random error at flip probability TORIC_FLIP (one rate
    for every prior: each batch then holds early exits at several depths and codewords that never
    converge).  Classical: _awgn at the variable rows, 0 at the check rows.  A synthetic batch
    adds SYN_SEED[code, B] to the seed."""
    H = code_matrix(code)
    V, C = H.shape
    rng = np.random.default_rng([seed + SYN_SEED.get((code, B), 0), B, V, C])
    x = np.zeros((B, V + C), np.dtype(dtype))
    if syndrome_style(code):
        for b in range(B):
            p = TORIC_P[b % 4]
            x[b, :V] = np.log((1 - p) / p)
            e = (rng.random(V) < TORIC_FLIP).astype(np.int64)
            x[b, V:] = 1 - 2 * ((e @ H.astype(np.int64)) % 2)
    else:
        x[:, :V] = _awgn(rng, B, V, np.dtype(dtype))
    x = x.reshape(-1)
    x.setflags(write=False)
    return H, x


def assert_coverage(code, B, dtype, params, its, status):
    """What a reference batch of B >= 5 must hold, shared with minsum_layered_cases.reference:
    both statuses (on a SYN_EASY graph: status 0 only, stated here rather than skipped), and
    under early stop at least two distinct iteration counts with the unconverged codewords at
    `iters`; without early stop every codeword runs exactly `iters` iterations."""
    alpha, beta, iters, early_stop = params
    if B < 5:
        return
    tag = (code, B, dtype, params, its.tolist(), status.tolist())
    if code in SYN_EASY:
        assert not status.any(), tag
    else:
        assert set(status.tolist()) == {0, 1}, tag
    if early_stop:
        assert len(set(its.tolist())) >= 2, tag
        assert (its[status == 1] == iters).all(), tag
    else:
        assert (its == iters).all(), tag


@functools.lru_cache(maxsize=None)
def reference(code, B, dtype, params, seed=0):
    """(llr [B*V] in dtype, iters_used [B] int32, status [B] int32) of the numpy statement,
    read-only.  A batch of B >= 5 must hold both statuses, and under early stop at least two
    distinct iteration counts, so that no seed hides the early exit or the run to the end; without
    early stop every codeword runs exactly `iters` iterations, which is asserted instead."""
    alpha, beta, iters, early_stop = params
    H, x = inputs(code, B, dtype, seed)
    V, C = H.shape
    xb = x.reshape(B, V + C)
    t = (xb[:, V:] < 0).astype(np.int64)
    res = [minsum_ref(code, xb[b, :V], t[b], alpha, beta, iters, early_stop) for b in range(B)]
    llr = np.concatenate([r[0] for r in res])
    its = np.array([r[1] for r in res], np.int32)
    status = np.array([r[2] for r in res], np.int32)
    assert_coverage(code, B, dtype, params, its, status)
    for arr in (llr, its, status):
        arr.setflags(write=False)
    return llr, its, status


def soft_output(llr):
    """1 / (1 + exp(llr)) in llr's dtype."""
    with np.errstate(over='ignore'):
        one = llr.dtype.type(1)
        return one / (one + np.exp(llr))


def pred_tolerance(dtype):
    """The project's soft-output tolerance (rtol 1e-10 fp64, 1e-4 fp32) plus one smallest normal
    of absolute slack: a denormal result may flush to zero."""
    dt = np.dtype(dtype)
    return dict(rtol=1e-10 if dt == np.float64 else 1e-4, atol=float(np.finfo(dt).tiny))


def satisfied(H, x, llr):
    """Per codeword: H^T (llr < 0) == t."""
    V, C = H.shape
    t = (x.reshape(-1, V + C)[:, V:] < 0).astype(np.int64)
    h = (llr.reshape(-1, V) < 0).astype(np.int64)
    return (((h @ H.astype(np.int64)) % 2) == t).all(axis=1)
