"""Shared by tests/test_bpgd_cpu.py and tests/test_gpu_bpgd.py: the numpy statement of min-sum BP
with guided decimation (include/gnnd.h, gnnd_bpgd), every operation a numpy operation on values of
the dtype (so each rounds once), on the inputs of tests/minsum_cases.py (uniform priors per
codeword on the syndrome-style graphs, so exact ties between reliabilities are the rule, not the
exception) and the graphs of tests/synthetic_codes.py.  The references assert their own coverage:
for every (shape, parameter set) the set of coverage facts below is recorded in COVERAGE and
asserted exactly, so a fact a shape cannot give is asserted absent rather than skipped, and
REQUIRED names the facts each parameter set exists for, which some recorded shape must give."""
import functools

import numpy as np

import minsum_cases as mc
import relay_cases as rc

ALPHA, BETA, CLAMP = 0.75, 0.0, 25.0
LEAST, MOST = 'least', 'most'


def params(V):
    """(iters0, iters_round, rounds, per_round, pick): plain min-sum; the working set; the
    most-reliable rule with several picks per round; one that exhausts the V variables."""
    return ((12, 12, 0, 1, LEAST), (10, 5, 16, 1, LEAST), (10, 5, 8, 3, MOST), (2, 1, V, 1, LEAST))


# the batches of the CPU and GPU tests
SHAPES = (('toric_5', 9), ('toric_5', 67), ('toric_7', 9), ('bch_63_45', 5), ('bch_63_45', 33),
          ('syn_hub', 9), ('syn_wide', 9), ('syn_sq64', 9))
# minsum_cases.inputs seeds, searched on the CPU for the coverage recorded below (seed 0 where
# absent)
SEED = {('toric_5', 9): 1, ('toric_5', 67): 1, ('bch_63_45', 5): 3, ('bch_63_45', 33): 5,
        ('syn_hub', 9): 4, ('syn_sq64', 9): 11}

# coverage facts of one reference batch:
#   st0 / st1    a codeword of status 0 / 1
#   late         a codeword solved only after at least one decimation (status 0, ndec > 0)
#   tie          a pick decided by the lowest-v rule (another undecimated variable had the same |L|)
#   rounds       a status-1 codeword that stopped on r == rounds with ndec < V
#   full         a status-1 codeword that stopped with ndec == V
#   neg          a pick of negative sign (p_v* = -c)
FACTS = ('st0', 'st1', 'late', 'tie', 'rounds', 'full', 'neg')
# (code, B) -> one string of facts per parameter set, the same in float32 and float64; filled from
# the CPU search that chose SEED
COVERAGE = {
    ('toric_5', 9): ('st0 st1 rounds', 'st0 st1 late tie rounds neg', 'st0 st1 tie rounds',
                     'st0 st1 late tie full neg'),
    # the one toric batch in which the most-reliable rule freezes a bit at -c
    ('toric_5', 67): ('st0 st1 rounds', 'st0 st1 late tie rounds neg', 'st0 st1 tie rounds neg',
                      'st0 st1 late tie full neg'),
    ('toric_7', 9): ('st0 st1 rounds', 'st0 st1 late tie rounds neg', 'st0 st1 tie rounds',
                     'st0 st1 late tie full neg'),
    # AWGN priors: hardly two reliabilities are equal, so no pick is a tie but under set 3 at
    # B = 33; of the five codewords of the small batch the working set rescues none
    ('bch_63_45', 5): ('st0 st1 rounds', 'st0 st1 rounds neg', 'st0 st1 late rounds neg',
                       'st0 st1 late full neg'),
    ('bch_63_45', 33): ('st0 st1 rounds', 'st0 st1 late rounds neg', 'st0 st1 late rounds neg',
                        'st0 st1 late tie full neg'),
    ('syn_hub', 9): ('st0 st1 rounds', 'st0 st1 late tie rounds neg', 'st0 st1 rounds neg',
                     'st0 st1 late tie full neg'),
    # min-sum alone solves none of this batch, and neither does the most-reliable rule
    ('syn_wide', 9): ('st1 rounds', 'st0 st1 late tie rounds neg', 'st1 tie rounds neg',
                      'st0 st1 late tie full neg'),
    # minsum_cases.SYN_EASY: status 0 only under every set; the two-iteration start of set 3 still
    # reaches a decimation
    ('syn_sq64', 9): ('st0', 'st0', 'st0', 'st0 late tie neg'),
}
# parameter set -> facts some recorded shape must give under it
REQUIRED = {0: ('st0', 'st1'), 1: ('st0', 'st1', 'late', 'tie', 'rounds'), 2: ('neg',),
            3: ('full',)}

code_matrix = mc.code_matrix
satisfied = mc.satisfied


def inputs(code, B, dtype):
    """(H, x [B*N]) in dtype, read-only: minsum_cases.inputs at SEED[code, B]."""
    return mc.inputs(code, B, dtype, SEED.get((code, B), 0))


@functools.lru_cache(maxsize=None)
def _check_groups(code):
    """[(checks [n], their edges [n, d])] by check degree d, edges ascending inside a check."""
    chk = rc._tables(code)[1]
    groups = {}
    for c, ce in enumerate(chk):
        groups.setdefault(ce.size, []).append((c, ce))
    return [(np.array([c for c, _ in g]), np.stack([ce for _, ce in g])) for g in groups.values()]


def check_step(code, q, t, a, b):
    """gnnd_minsum's check step on q [B, E] with targets t [B, C] (bool) -> r [B, E]: literally the
    minimum and the sign parity over the other edges of the check, all checks of one degree at
    once (the diagonal of a [d, d] table masked out)."""
    zero = q.dtype.type(0)
    r = np.empty_like(q)
    for cs, es in _check_groups(code):
        d = es.shape[1]
        qc = q[:, es]                                       # [B, n, d]
        neg = qc < zero
        others = ~np.eye(d, dtype=bool)                     # [e, e']: e' != e
        cnt = (neg[:, :, None, :] & others).sum(axis=3)
        par = t[:, cs, None] ^ (cnt & 1).astype(bool)
        m = np.where(others, np.abs(qc)[:, :, None, :], np.inf).min(axis=3).astype(q.dtype)
        dd = a * m - b                                      # two numpy operations: two roundings
        mag = np.where(dd > zero, dd, zero)
        r[:, es] = np.where(par, -mag, mag)
    return r


def bpgd_ref(code, xb, iters0, iters_round, rounds, per_round, pick, clamp=CLAMP, alpha=ALPHA,
             beta=BETA):
    """The definition on a batch xb [B, N], the codewords in lockstep over (round, iteration) with
    a mask of the ones still running.  Returns a dict: llr, ehat [B, V], iters, status, ndec [B]
    int32, and for the coverage facts ties, negs [B] (picks decided by the tie rule / of negative
    sign)."""
    T = xb.dtype.type
    ev, chk, vptr, steps = rc._tables(code)
    H = code_matrix(code).astype(np.int64)
    V = H.shape[0]
    B = xb.shape[0]
    a, bt, zero, c = T(alpha), T(beta), T(0), T(clamp)
    t = xb[:, V:] < zero
    p = xb[:, :V].copy()
    dec = np.zeros((B, V), bool)
    q = p[:, ev]
    L = np.zeros((B, V), xb.dtype)
    total, ndec, ties, negs = (np.zeros(B, np.int32) for _ in range(4))
    status = np.ones(B, np.int32)
    done = np.zeros(B, bool)
    with np.errstate(all='ignore'):
        for r in range(rounds + 1):
            for it in range(iters0 if r == 0 else iters_round):
                act = np.nonzero(~done)[0]
                if act.size == 0:
                    break
                total[act] += 1
                rr = check_step(code, q[act], t[act], a, bt)
                s = p[act]
                for vs, es in steps:
                    s[:, vs] = s[:, vs] + rr[:, es]
                L[act] = s
                q[act] = s[:, ev] - rr
                ok = (((s < zero).astype(np.int64) @ H) % 2 == t[act]).all(axis=1)
                status[act[ok]] = 0
                done[act[ok]] = True
            done |= (r == rounds) | (ndec == V)
            for b in np.nonzero(~done)[0]:
                key = np.abs(L[b])                          # every pick reads this round's last L
                for _ in range(min(per_round, V - ndec[b])):
                    cand = np.nonzero(~dec[b])[0]
                    k = key[cand]
                    # the first occurrence of the extremum: the ascending scan with a strict compare
                    i = int(np.argmax(k) if pick == MOST else np.argmin(k))
                    ties[b] += int((k == k[i]).sum() > 1)
                    v = cand[i]
                    negs[b] += int(L[b, v] < zero)
                    p[b, v] = -c if L[b, v] < zero else c
                    dec[b, v] = True
                    ndec[b] += 1
    return dict(llr=L, ehat=(L < zero).astype(xb.dtype), iters=total, status=status, ndec=ndec,
                ties=ties, negs=negs)


def facts(res, V):
    """The coverage facts (a string over FACTS, in that order) of one bpgd_ref result."""
    st, nd = res['status'], res['ndec']
    have = {'st0': (st == 0).any(), 'st1': (st == 1).any(), 'late': ((st == 0) & (nd > 0)).any(),
            'tie': res['ties'].any(), 'rounds': ((st == 1) & (nd < V)).any(),
            'full': ((st == 1) & (nd == V)).any(), 'neg': res['negs'].any()}
    return ' '.join(f for f in FACTS if have[f])


@functools.lru_cache(maxsize=None)
def reference(code, B, dtype, pset):
    """The numpy statement on inputs(code, B, dtype) under params(V)[pset]: a dict of read-only
    arrays, llr / ehat / pred flattened to [B*V] (pred = 1 / (1 + exp(llr)) by numpy, for the
    tolerance comparison of the float32 soft output).  Asserts the batch's recorded coverage."""
    H, x = inputs(code, B, dtype)
    V, C = H.shape
    iters0, iters_round, rounds, per_round, pick = params(V)[pset]
    res = bpgd_ref(code, x.reshape(B, V + C).copy(), iters0, iters_round, rounds, per_round, pick)
    tag = (code, B, dtype, pset)
    st, nd, its = res['status'], res['ndec'], res['iters']
    # what the definition implies for any batch
    assert ((nd == 0) | (its > iters0)).all() and (nd <= min(V, rounds * per_round)).all(), tag
    assert (its[st == 1] == iters0 + np.minimum(rounds, -(-nd[st == 1] // per_round)
                                                + (nd[st == 1] < V)) * iters_round).all(), tag
    if (code, B) in COVERAGE:
        assert facts(res, V) == COVERAGE[code, B][pset], (tag, facts(res, V))
    res['llr'] = res['llr'].reshape(-1)
    res['ehat'] = res['ehat'].reshape(-1)
    res['pred'] = mc.soft_output(res['llr'])
    for arr in res.values():
        arr.setflags(write=False)
    return res


def assert_required_coverage():
    """Every fact a parameter set exists for is recorded for some shape (and reference() asserts
    the records)."""
    for pset, need in REQUIRED.items():
        for f in need:
            assert any(f in cov[pset].split() for cov in COVERAGE.values()), (pset, f)
    assert set(COVERAGE) == set(SHAPES)


OUTPUTS = ('ehat', 'llr', 'iters', 'status', 'ndec')


def assert_equal(got, ref, what=''):
    """got = (ehat, llr, pred, iters, status, ndec) as flat numpy arrays against a reference dict or
    another such tuple: exact in everything but pred, llr with its sign bit."""
    if not isinstance(ref, dict):
        ref = dict(zip(('ehat', 'llr', 'pred', 'iters', 'status', 'ndec'), ref))
    got = dict(zip(('ehat', 'llr', 'pred', 'iters', 'status', 'ndec'), got))
    for name in OUTPUTS:
        a, b = got[name], ref[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype)
        assert np.array_equal(a, b), (what, name, np.nonzero(a != b)[0][:8].tolist())
    assert np.array_equal(np.signbit(got['llr']), np.signbit(ref['llr'])), (what, 'llr sign bit')
