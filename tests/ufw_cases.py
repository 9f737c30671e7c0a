"""Shared by tests/test_ufw_cpu.py, tests/test_gpu_ufw.py and tools/ufw_host_sanitize.sh: an
independent statement of weighted union-find (include/gnnd.h, gnnd_ufw) and seeded inputs on the
graphs of tests/uf_cases.py.  The statement shares no code with the host mirror and does not jump:
it grows in unit half-steps (every edge gains its rate, capped at its length), takes explicit unions
on a disjoint-set forest over the edges that just filled, and counts rounds as the steps taken and
events as the steps in which an edge filled.  The weights come from numpy in the case's dtype (one
np.float32 / np.float64 multiply, two compares).  uf_cases keeps its forest and peel inside
uf_ref_one, where they cannot be imported apart from its growth loop, so they are stated again here
(level sets instead of a queue, a sort by depth instead of a recursion); test_ufw_cpu.py ties the
two together: with scale = 0 this statement must give uf_cases.uf_ref's outputs on every shape.
COVERAGE holds, per shape, exactly the facts its float64 batch with llr gives (asserted, so a batch
that stops exercising a branch fails), and REQUIRED the facts some shape must give."""
import functools

import numpy as np

import uf_cases as uc

B_ALL = uc.B_ALL
SHAPES = uc.SHAPES
FLIP = uc.FLIP              # codeword 1 and every sixth after it: p = 0, a zero syndrome
SCALE, WMAX = 2.0, 8        # the statement's runs; weights clamp at llr >= (WMAX - 1) / SCALE = 3.5

# coverage facts of one batch:
#   jump3      an edge filled after at least 3 steps in which none did (a jump with d >= 3)
#   overshoot  an edge filled by a rate-2 step from one half-unit short: the overshoot is capped.
#              It cannot happen, and every run asserts that it did not.  Call A_u the steps vertex
#              u has spent in an odd cluster; an uncapped edge holds A_a + A_b.  Every vertex of
#              an odd cluster has A_u = (steps so far) mod 2: true at step 0; a vertex that joins
#              through an edge grown from the other end alone joins when that end's A equals the
#              even length, so at an even step with A_u = 0; a vertex whose cluster went even and
#              is woken by an edge to an odd cluster has A_u = length - A_other, the parity of the
#              other end's.  So an edge with both ends in odd clusters holds an even number and
#              lands on its even length exactly.  (The same holds for gnnd_uf: its min(2, ..) never
#              cuts 3 down to 2.)
#   merge      two odd clusters joined into an even one
#   clamp      a weight clamped at wmax
#   neg        a weight of 1 from a negative reliability
#   vroot      a cluster with a full edge rooted at a virtual vertex
#   zero       a codeword with a zero syndrome (rounds 0, events 0, nfull 0)
FACTS = ('jump3', 'overshoot', 'merge', 'clamp', 'neg', 'vroot', 'zero')
# shape -> the facts of its B_ALL float64 batch with llr; filled from the CPU run of this statement
COVERAGE = {
    'toric_3': 'jump3 merge clamp neg vroot zero',
    'toric_5': 'jump3 merge clamp neg vroot zero',
    'ring_63': 'jump3 merge clamp neg zero',          # a ring has no virtual vertex
    'ring_64': 'jump3 merge clamp neg zero',
    'ring_65': 'jump3 merge clamp neg zero',
    'ring_130': 'jump3 merge clamp neg zero',
    'chain_65': 'jump3 merge clamp neg vroot zero',
    'parallel': 'jump3 merge clamp neg zero',
    'two_comp': 'jump3 merge clamp neg vroot zero',
}
REQUIRED = tuple(f for f in FACTS if f != 'overshoot')


def weights(r, scale, wmax, dtype):
    """w [..] int of reliabilities r, in dtype: m = r * s; wmax where m >= wmax - 1, 1 + trunc(m)
    where m > 0, else 1 (a NaN compares false) -> (w, clamped mask, negative mask)."""
    dt = np.dtype(dtype).type
    with np.errstate(invalid='ignore', over='ignore'):
        m = np.asarray(r, dtype=dt) * dt(scale)
        hi = m >= dt(wmax - 1)
        pos = (m > dt(0)) & ~hi
        w = np.ones(m.shape, np.int64)
        w[hi] = wmax
        w[pos] = 1 + np.trunc(m[pos]).astype(np.int64)
        neg = np.asarray(r, dtype=dt) < 0
    return w, hi, neg


def ufw_ref_one(N, C, ends, cvirt, t, w):
    """One codeword: t [C] 0/1, w [V] weights -> (ehat [V] 0/1, rounds, status, nfull, events,
    set of facts)."""
    V = len(ends)
    facts = set()
    defect = [0] * N
    for c in range(C):
        if t[c]:
            defect[c] ^= 1
            if cvirt[c] >= 0:
                defect[cvirt[c]] ^= 1
    if not any(t):
        facts.add('zero')
    length = [2 * int(k) for k in w]
    grow = [0] * V
    up = list(range(N))
    parity = defect[:]                      # by set root

    def find(u):
        while up[u] != u:
            up[u] = up[up[u]]
            u = up[u]
        return u

    rounds = events = status = quiet = 0
    while True:
        roots = [find(u) for u in range(N)]
        if not any(parity[r] for r in set(roots)):
            break
        rate = [parity[roots[a]] + parity[roots[b]] for a, b in ends]
        if not any(rate[v] and grow[v] < length[v] for v in range(V)):
            status = 1                      # an odd cluster that is a whole component
            break
        fresh = []
        for v in range(V):                  # one unit step
            if grow[v] == length[v] or not rate[v]:
                continue
            if grow[v] + rate[v] > length[v]:
                facts.add('overshoot')
            grow[v] = min(length[v], grow[v] + rate[v])
            if grow[v] == length[v]:
                fresh.append(v)
        rounds += 1
        if not fresh:
            quiet += 1
            continue
        events += 1
        if quiet >= 2:
            facts.add('jump3')
        quiet = 0
        for v in fresh:
            ra, rb = find(ends[v][0]), find(ends[v][1])
            if ra == rb:
                continue
            if parity[ra] and parity[rb]:
                facts.add('merge')
            up[ra] = rb
            parity[rb] ^= parity[ra]
    # forest: every cluster's root is its highest vertex; level sets over the full edges
    full = [v for v in range(V) if grow[v] == length[v]]
    nbrs = {}
    for v in full:
        a, b = ends[v]
        nbrs.setdefault(a, []).append((v, b))
        nbrs.setdefault(b, []).append((v, a))
    top = {}
    for u in nbrs:
        r = find(u)
        top[r] = max(top.get(r, -1), u)
    depth = {}
    level = sorted(top.values())
    for root in level:
        depth[root] = 0
        if root >= C:
            facts.add('vroot')
    d = 0
    while level:
        d += 1
        nxt = []
        for u in level:
            for _, x in nbrs[u]:
                if x not in depth:
                    depth[x] = d
                    nxt.append(x)
        level = nxt
    pedge = {u: min(v for v, x in nbrs[u] if depth[x] == depth[u] - 1)
             for u in nbrs if depth[u] > 0}
    # peel: the deepest vertices first, each handing its subtree parity to its parent
    sub = defect[:]
    ehat = [0] * V
    for u in sorted(pedge, key=lambda k: -depth[k]):
        v = pedge[u]
        a, b = ends[v]
        ehat[v] = sub[u]
        sub[b if a == u else a] ^= sub[u]
    return ehat, rounds, status, len(full), events, facts


def ufw_ref(H, x, llr=None, scale=SCALE, wmax=WMAX):
    """The statement on x [B * N] (and llr [B * V] or None) in x's dtype -> dict of ehat01 [B, V]
    uint8, rounds, status, nfull, events [B] int32, and facts (the union over the batch)."""
    V, C = H.shape
    N, ends, cvirt = uc.matching_ref(H)
    x = np.asarray(x)
    xb = x.reshape(-1, V + C)
    B = xb.shape[0]
    r = xb[:, :V] if llr is None else np.asarray(llr).reshape(B, V)
    w, hi, neg = weights(r, scale, wmax, x.dtype)
    res = dict(ehat01=np.zeros((B, V), np.uint8), facts=set(),
               **{k: np.zeros(B, np.int32) for k in ('rounds', 'status', 'nfull', 'events')})
    pairs = [tuple(int(i) for i in ab) for ab in ends]
    for b in range(B):
        with np.errstate(invalid='ignore'):
            t = xb[b, V:] < 0
        (ehat, res['rounds'][b], res['status'][b], res['nfull'][b], res['events'][b],
         facts) = ufw_ref_one(N, C, pairs, cvirt, t, w[b])
        res['ehat01'][b] = ehat
        res['facts'] |= facts
        if res['rounds'][b]:                # the weights of a codeword that grew
            if hi[b].any():
                res['facts'].add('clamp')
            if neg[b].any():
                res['facts'].add('neg')
    return res


@functools.lru_cache(maxsize=None)
def _inputs_all(shape):
    """x [B_ALL, V + C] float64: the channel LLR ln((1 - p) / p) of the codeword's flip probability
    on the variable rows (+inf for p = 0), -/+ a magnitude in [0.5, 1.5] for a syndrome bit 1 / 0 of
    a random error pattern on the check rows; llr [B_ALL, V] float64 from N(1.5, 2.5) with one value
    in sixteen set to an exact zero."""
    H = uc.code_matrix(shape)
    V, C = H.shape
    rng = np.random.default_rng([SHAPES.index(shape), 20261])
    p = np.array([FLIP[b % len(FLIP)] for b in range(B_ALL)])
    e = rng.random((B_ALL, V)) < p[:, None]
    t = uc.syndrome(H, e)
    x = np.empty((B_ALL, V + C))
    with np.errstate(divide='ignore'):
        x[:, :V] = np.log((1 - p) / p)[:, None]
    x[:, V:] = (1 - 2 * t) * rng.uniform(0.5, 1.5, (B_ALL, C))
    llr = rng.normal(1.5, 2.5, (B_ALL, V))
    llr[rng.random((B_ALL, V)) < 1 / 16] = 0.0
    assert (llr < 0).mean() > 0.2 and (llr == 0).any() and (llr * SCALE >= WMAX - 1).any()
    x.setflags(write=False)
    llr.setflags(write=False)
    return x, llr


def inputs(shape, B, dtype):
    """(H, x [B * N], llr [B * V]) in dtype, read-only: the first B codewords of the shape's batch."""
    xa, la = _inputs_all(shape)
    x = xa[:B].reshape(-1).astype(dtype)
    llr = la[:B].reshape(-1).astype(dtype)
    x.setflags(write=False)
    llr.setflags(write=False)
    return uc.code_matrix(shape), x, llr


@functools.lru_cache(maxsize=None)
def _reference_all(shape, dtype, with_llr):
    H, x, llr = inputs(shape, B_ALL, dtype)
    res = ufw_ref(H, x, llr if with_llr else None)
    V, C = H.shape
    # what the definition implies for any batch
    t = (x.reshape(B_ALL, V + C)[:, V:] < 0)
    assert not res['status'].any(), shape
    assert np.array_equal(uc.syndrome(H, res['ehat01']), t), shape
    assert ((res['rounds'] == 0) == ~t.any(axis=1)).all(), shape
    assert (res['rounds'] <= 2 * WMAX * V).all() and (res['events'] <= V).all(), shape
    assert (res['events'] <= res['rounds']).all(), shape
    assert ((res['nfull'] == 0) == (res['rounds'] == 0)).all(), shape
    assert 'overshoot' not in res['facts'], shape
    if with_llr and dtype == 'float64':
        got = ' '.join(f for f in FACTS if f in res['facts'])
        assert got == COVERAGE[shape], (shape, got)
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def reference(shape, B, dtype, with_llr):
    """(ehat [B * V] in dtype, rounds, status, nfull, events [B] int32) of inputs(shape, B, dtype)
    at SCALE / WMAX, on llr or on the priors: the first B codewords of the one reference batch."""
    r = _reference_all(shape, dtype, bool(with_llr))
    V = uc.code_matrix(shape).shape[0]
    return (r['ehat01'][:B].reshape(B * V).astype(dtype), r['rounds'][:B], r['status'][:B],
            r['nfull'][:B], r['events'][:B])


def as_tuple(res, dtype):
    return (res['ehat01'].reshape(-1).astype(dtype), res['rounds'], res['status'], res['nfull'],
            res['events'])


def assert_required_coverage():
    assert set(COVERAGE) == set(SHAPES)
    for f in REQUIRED:
        assert any(f in cov.split() for cov in COVERAGE.values()), f


def assert_equal(got, ref, what=''):
    """(ehat, rounds, status, nfull, events) flat numpy arrays against another such tuple: exact,
    dtypes included."""
    assert len(got) == len(ref) == 5, what
    for name, a, b in zip(('ehat', 'rounds', 'status', 'nfull', 'events'), got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape)
        assert np.array_equal(a, b), (what, name, np.nonzero(a != b)[0][:8].tolist())


def dirty_inputs(H, x, llr, B):
    """(x [B, N], llr [B, V]) copies with NaN, +-0 and +-inf over half of llr and of the priors and
    of a quarter of the syndrome rows (only -inf sets a syndrome bit).  For graphs whose components all
    have a virtual vertex: any syndrome is satisfiable there."""
    V, C = H.shape
    xb = x.reshape(B, V + C).copy()
    lb = llr.reshape(B, V).copy()
    rng = np.random.default_rng(5)
    vals = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf], xb.dtype)
    k = rng.integers(0, 10, lb.shape)
    lb[k < 5] = vals[k[k < 5]]
    k = rng.integers(0, 10, (B, V))
    xb[:, :V][k < 5] = vals[k[k < 5]]
    k = rng.integers(0, 20, (B, C))
    xb[:, V:][k < 5] = vals[k[k < 5]]                       # -inf sets a syndrome bit, the rest clear it
    assert np.isnan(lb).any() and np.isinf(lb).any() and np.isnan(xb[:, V:]).any()
    return xb, lb


# ---- belief-find: toric-5, B_ALL codewords, finite channel LLRs (min-sum needs finite input) ----
BF_SHAPE = 'toric_5'
BF_FLIP = (0.02, 0.06, 0.10, 0.14)
BF_ITERS, BF_ALPHA, BF_BETA = 10, 0.75, 0.0


@functools.lru_cache(maxsize=None)
def bf_inputs(dtype):
    """(H, x [B_ALL * N]) in dtype: the channel LLR on the variable rows, +/-1 on the check rows.
    tests/test_ufw_cpu.py asserts that min-sum leaves both statuses on it."""
    H = uc.code_matrix(BF_SHAPE)
    V, C = H.shape
    rng = np.random.default_rng(20262)
    p = np.array([BF_FLIP[b % len(BF_FLIP)] for b in range(B_ALL)])
    e = rng.random((B_ALL, V)) < p[:, None]
    x = np.empty((B_ALL, V + C))
    x[:, :V] = np.log((1 - p) / p)[:, None]
    x[:, V:] = 1 - 2 * uc.syndrome(H, e)
    x = x.reshape(-1).astype(dtype)
    x.setflags(write=False)
    return H, x
