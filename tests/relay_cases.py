"""Shared by tests/test_relay_cpu.py and tests/test_gpu_relay.py: the numpy statement of the relay
min-sum definition (include/gnnd.h, gnnd_relay), every operation a numpy operation on values of
the dtype (so each rounds once), the weight tree written out literally; gamma tables from fixed
seeds; and two input families: `plain` (minsum_cases.inputs) and `hard` (toric and synthetic
graphs: disordered priors and a flip rate high enough that later legs find lighter solutions than
the first).  The
references assert their own coverage: both statuses, several chosen legs, solutions replaced by
lighter ones, ties, and codewords that stop short of S solutions."""
import functools

import numpy as np

import minsum_cases as mc

ALPHA, BETA = 0.75, 0.0
# (legs, iters0, iters_leg, S); the first with an all-zero gamma row (plain min-sum), the third for
# the hard family, the last one runs out of legs
PARAMS = ((1, 12, 12, 1), (6, 12, 12, 1), (8, 12, 12, 4), (3, 2, 3, 2))
GAMMA_SEED = 7
HARD_P = (0.04, 0.08, 0.10, 0.12)
HARD_FLIP = 0.10
HARD_SEED = 0          # chosen on the CPU: see reference()'s assertions for what it must give
# minsum_cases.inputs seeds of the plain family, searched on the CPU where seed 0 leaves a small
# batch without an unsolved codeword under the six- and eight-leg sets (relay solves about 95 %)
PLAIN_SEED = {('toric_5', 5): 13, ('toric_5', 9): 1, ('toric_7', 9): 5,
              # synthetic: both statuses under PARAMS[1] and PARAMS[3], five chosen legs
              ('syn_hub', 9): 1}
# seeds of the hard family on the synthetic graphs (HARD_SEED elsewhere), searched on the CPU.
# syn_sq64: both statuses under PARAMS[1] and PARAMS[3].  syn_tall is minsum_cases.SYN_EASY here
# too: on 3 600 codewords per family leg 0 solved every one within 12 iterations, so its batch
# holds status 0 only (reference() asserts that instead); this seed makes the short legs of
# PARAMS[3] choose legs 0, 1 and 2 and stop at one and at two solutions
SYN_HARD_SEED = {('syn_sq64', 9): 1, ('syn_tall', 9): 28}
SOLVED_ONLY = ('syn_tall',)

code_matrix = mc.code_matrix
satisfied = mc.satisfied


@functools.lru_cache(maxsize=None)
def gammas(V, params, dtype):
    """[legs, V] in dtype, read-only: all zero for one leg, else row 0 = 0.125 and the later rows
    uniform in [-0.24, 0.66] from default_rng(GAMMA_SEED)."""
    legs = params[0]
    g = np.zeros((legs, V))
    if legs > 1:
        g[0] = 0.125
        g[1:] = np.random.default_rng(GAMMA_SEED).uniform(0.21 - 0.45, 0.21 + 0.45, (legs - 1, V))
    g = g.astype(dtype)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def inputs(family, code, B, dtype, seed=None):
    """(H, x [B*N]) in dtype, read-only.  plain: minsum_cases.inputs.  hard (toric, synthetic):
    priors log((1 - p) / p) * (1 + 0.25 u), u uniform per variable, p = HARD_P[b % 4]; check rows
    (-1)^(H^T e) of an error drawn at flip rate HARD_FLIP."""
    if family == 'plain':
        return mc.inputs(code, B, dtype, PLAIN_SEED.get((code, B), 0) if seed is None else seed)
    assert family == 'hard' and mc.syndrome_style(code)
    H = code_matrix(code)
    V, C = H.shape
    if seed is None:
        seed = SYN_HARD_SEED.get((code, B), HARD_SEED)
    rng = np.random.default_rng([seed, B, V, C])
    x = np.zeros((B, V + C), np.dtype(dtype))
    for b in range(B):
        p = HARD_P[b % 4]
        x[b, :V] = np.log((1 - p) / p) * (1 + 0.25 * rng.random(V))
        e = (rng.random(V) < HARD_FLIP).astype(np.int64)
        x[b, V:] = 1 - 2 * ((e @ H.astype(np.int64)) % 2)
    x = x.reshape(-1)
    x.setflags(write=False)
    return H, x


@functools.lru_cache(maxsize=None)
def _tables(code):
    """(edge variable [E], edge ids of every check, edge range of every variable, [(variables of
    degree > j, their j-th edge)] for j = 0 .. max degree - 1), edges sorted by (v, c)."""
    H = code_matrix(code)
    ev, ec = np.nonzero(H)
    chk = [np.nonzero(ec == c)[0] for c in range(H.shape[1])]
    deg = np.bincount(ev, minlength=H.shape[0])
    vptr = np.concatenate([[0], np.cumsum(deg)])
    steps = []
    for j in range(int(deg.max())):
        vs = np.nonzero(deg > j)[0]
        steps.append((vs, vptr[vs] + j))
    return ev, chk, vptr, steps


def weight(h, l):
    """The contract's weight of one hard decision h [V] under priors l [V], in l's dtype: 64
    partials over v = j (mod 64) in ascending v from +0, then p_j = p_j + p_{j xor s} for s = 32,
    16, 8, 4, 2, 1; w = p_0."""
    T = l.dtype.type
    p = np.zeros(64, l.dtype)
    for v in range(l.size):
        p[v % 64] = T(p[v % 64] + (l[v] if h[v] else T(0)))
    j = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        p = p + p[j ^ s]
    return p[0]


def _check_step(q, t, chk, a, b):
    """gnnd_minsum's check step on q [B, E] with targets t [B, C] (bool) -> r [B, E]: literally the
    minimum and the sign parity over the other edges of the check."""
    zero = q.dtype.type(0)
    r = np.empty_like(q)
    for c, ce in enumerate(chk):
        qc = q[:, ce]
        neg = qc < zero
        mag_in = np.abs(qc)
        for j, e in enumerate(ce):
            others = np.arange(ce.size) != j
            par = t[:, c] ^ (neg[:, others].sum(axis=1) & 1).astype(bool)
            m = mag_in[:, others].min(axis=1)
            d = a * m - b                                   # two numpy operations: two roundings
            mag = np.where(d > zero, d, zero)
            r[:, e] = np.where(par, -mag, mag)
    return r


def relay_ref(code, xb, g, iters0, iters_leg, S, alpha=ALPHA, beta=BETA):
    """The definition on a batch xb [B, N], gammas g [legs, V], all codewords in lockstep over
    (leg, iteration) with a mask of the ones still inside the leg.  Returns a dict: llr [B, V],
    ehat [B, V], iters, status, leg, nsol [B] int32, and for the coverage checks first_leg [B] (the
    leg of the first solution, -1 if none) and ties [B] (solutions whose weight equalled the best
    so far, which the strict comparison left out)."""
    T = xb.dtype.type
    ev, chk, vptr, steps = _tables(code)
    H = code_matrix(code).astype(np.int64)
    V = H.shape[0]
    B = xb.shape[0]
    a, bt, zero = T(alpha), T(beta), T(0)
    l = xb[:, :V]
    t = xb[:, V:] < zero
    legs = g.shape[0]
    M = l.copy()
    q = np.empty((B, ev.size), xb.dtype)
    best_L = np.zeros((B, V), xb.dtype)
    best_w = np.zeros(B, xb.dtype)
    leg = np.full(B, -1, np.int32)
    first_leg = np.full(B, -1, np.int32)
    nsol = np.zeros(B, np.int32)
    total = np.zeros(B, np.int32)
    ties = np.zeros(B, np.int32)
    done = np.zeros(B, bool)
    with np.errstate(all='ignore'):
        for k in range(legs):
            gk = g[k]
            cl = (T(1) - gk) * l                            # round(1 - g), then round(c * l)

            def lam(M):
                return np.where(gk == zero, l, cl + gk * M)  # round(g * M), then the sum

            act = ~done
            q[act] = lam(M)[:, ev][act]
            for it in range(iters0 if k == 0 else iters_leg):
                if not act.any():
                    break
                total[act] += 1
                r = _check_step(q, t, chk, a, bt)
                s = lam(M)
                for vs, es in steps:
                    s[:, vs] = s[:, vs] + r[:, es]
                M[act] = s[act]
                q[act] = (s[:, ev] - r)[act]
                h = M < zero
                ok = (((h.astype(np.int64) @ H) % 2) == t).all(axis=1) & act
                for b in np.nonzero(ok)[0]:
                    w = weight(h[b], l[b])
                    if nsol[b] == 0 or w < best_w[b]:
                        best_w[b], leg[b] = w, k
                        best_L[b] = M[b]
                    elif w == best_w[b]:
                        ties[b] += 1
                    if nsol[b] == 0:
                        first_leg[b] = k
                    nsol[b] += 1
                act &= ~ok
            done |= nsol >= S
    found = nsol > 0
    llr = np.where(found[:, None], best_L, M)
    return dict(llr=llr, ehat=(llr < zero).astype(xb.dtype), iters=total,
                status=(~found).astype(np.int32), leg=leg, nsol=nsol, first_leg=first_leg, ties=ties)


@functools.lru_cache(maxsize=None)
def reference(family, code, B, dtype, params):
    """The numpy statement on inputs(family, code, B, dtype) with gammas(V, params, dtype): a dict
    of read-only arrays, llr and ehat flattened to [B*V].  Asserts what the batch must hold."""
    legs, iters0, iters_leg, S = params
    H, x = inputs(family, code, B, dtype)
    V, C = H.shape
    res = relay_ref(code, x.reshape(B, V + C).copy(), gammas(V, params, dtype), iters0, iters_leg, S)
    res['llr'] = res['llr'].reshape(-1)
    res['ehat'] = res['ehat'].reshape(-1)
    st, leg, nsol = res['status'], res['leg'], res['nsol']
    tag = (family, code, B, dtype, params)
    full = iters0 + (legs - 1) * iters_leg
    assert (res['iters'][st == 1] == full).all() and (leg[st == 1] == -1).all(), tag
    assert (nsol[st == 1] == 0).all() and (nsol[st == 0] >= 1).all() and (nsol <= S).all(), tag
    if B >= 5 and code in SOLVED_ONLY:
        assert not st.any(), (tag, st.tolist())
    elif B >= 5:
        assert set(st.tolist()) == {0, 1}, (tag, st.tolist())
    if B >= 67 and legs >= 6:
        chosen = set(leg[st == 0].tolist())
        assert 0 in chosen and len(chosen - {0}) >= 2, (tag, sorted(chosen))
    if family == 'hard' and B >= 67:
        assert int((leg[st == 0] != res['first_leg'][st == 0]).sum()) >= 2, tag
        assert int(((nsol < S) & (st == 0)).sum()) >= 1, tag
        assert int(res['ties'].sum()) >= 1, tag
    for arr in res.values():
        arr.setflags(write=False)
    return res


OUTPUTS = ('ehat', 'llr', 'iters', 'status', 'leg', 'nsol')


def assert_equal(got, ref, what=''):
    """got = (ehat, llr, iters, status, leg, nsol) as flat numpy arrays against a reference dict (or
    another such tuple): exact, llr with its sign bit."""
    if isinstance(ref, dict):
        ref = tuple(ref[k] for k in OUTPUTS)
    for name, a, b in zip(OUTPUTS, got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype)
        assert np.array_equal(a, b), (what, name, np.nonzero(a != b)[0][:8].tolist())
    assert np.array_equal(np.signbit(got[1]), np.signbit(ref[1])), (what, 'llr sign bit')
