"""Shared by tests/test_uf_cpu.py and tests/test_gpu_uf.py: an independent statement of the
union-find decoder (include/gnnd.h, gnnd_uf), the small matchable graphs it is checked on, and
seeded syndromes.  The statement is serial and shares nothing with the host mirror's sweeps: the
clusters are a disjoint-set forest with explicit unions, the depths come from a breadth-first queue,
the parent of a vertex is chosen from its explicit candidate list, and the subtree parities come
from a recursion.  It records which branches a batch exercised; COVERAGE holds, per shape, exactly
the facts its batch of B_ALL codewords gives (asserted, so a fact a shape cannot give is asserted
absent rather than skipped), and REQUIRED the facts some shape must give."""
import collections
import functools
import sys

import numpy as np

import gnndecode as gd

sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))

B_ALL = 67          # every batch of the tests is the first B codewords of this one
# flip probabilities, by codeword index: codeword 1 (and every sixth after it) has a zero syndrome
FLIP = (0.08, 0.0, 0.03, 0.15, 0.25, 0.05)

SHAPES = ('toric_3', 'toric_5', 'ring_63', 'ring_64', 'ring_65', 'ring_130', 'chain_65',
          'parallel', 'two_comp')

# coverage facts of one batch:
#   rounds3   a codeword that ran at least 3 growth rounds
#   merge     two odd clusters joined into an even one
#   vroot     a cluster with a full edge rooted at a virtual vertex
#   tie       a parent edge chosen among several candidates by the lowest index
#   zero      a codeword with a zero syndrome (rounds 0, nfull 0)
FACTS = ('rounds3', 'merge', 'vroot', 'tie', 'zero')
# shape -> the facts of its B_ALL batch; filled from the CPU run of this reference
COVERAGE = {
    'toric_3': 'merge vroot tie zero',              # too small for a third round
    'toric_5': 'rounds3 merge vroot tie zero',
    # a ring has no virtual vertex, and a parent-edge tie needs a cluster that closes the ring
    'ring_63': 'rounds3 merge zero',
    'ring_64': 'rounds3 merge zero',
    'ring_65': 'rounds3 merge zero',
    'ring_130': 'rounds3 merge zero',
    'chain_65': 'rounds3 merge vroot zero',
    'parallel': 'rounds3 merge tie zero',           # the tie between the two parallel edges
    'two_comp': 'merge vroot zero',
}
REQUIRED = FACTS


def ring(n):
    """n checks and n variables, variable i joining checks i and i + 1 mod n: no virtual vertex."""
    H = np.zeros((n, n), np.uint8)
    H[np.arange(n), np.arange(n)] = 1
    H[np.arange(n), (np.arange(n) + 1) % n] = 1
    return H


def chain(n):
    """ring(n + 1) with its last check deleted: n checks, n + 1 variables of which the last two
    have degree 1, one virtual vertex."""
    return np.ascontiguousarray(ring(n + 1)[:, :n])


@functools.lru_cache(maxsize=None)
def code_matrix(shape):
    """H [V, C] of a shape, read-only."""
    kind, _, n = shape.partition('_')
    if kind == 'toric':
        H = np.asarray(gd.codes.toric_code(int(n))).astype(np.uint8)
    elif kind == 'ring':
        H = ring(int(n))
    elif kind == 'chain':
        H = chain(int(n))
    elif shape == 'parallel':
        # ring(8) with a ninth variable on the check pair (0, 1) of variable 0: parallel edges
        H = np.vstack([ring(8), ring(8)[:1]])
    elif shape == 'two_comp':
        # checks 0 .. 4 a ring (no virtual vertex), checks 5 .. 10 a chain (one)
        H = np.zeros((5 + 7, 5 + 6), np.uint8)
        H[:5, :5] = ring(5)
        H[5:, 5:] = chain(6)
    else:
        raise KeyError(shape)
    H.setflags(write=False)
    return H


def matching_ref(H):
    """(N, endpoints [V, 2]) of the decoding graph, by the rule of include/gnnd.h: components by a
    flood fill over the checks, the virtual vertices numbered in ascending order of a component's
    lowest check."""
    V, C = H.shape
    checks_of = [np.nonzero(H[v])[0].tolist() for v in range(V)]
    assert all(1 <= len(cs) <= 2 for cs in checks_of), 'not matchable'
    nbr = collections.defaultdict(set)
    for cs in checks_of:
        if len(cs) == 2:
            nbr[cs[0]].add(cs[1])
            nbr[cs[1]].add(cs[0])
    comp = [-1] * C
    ncomp = 0
    for c in range(C):                       # ascending: a component is met at its lowest check
        if comp[c] >= 0:
            continue
        todo = [c]
        comp[c] = ncomp
        while todo:
            for d in nbr[todo.pop()]:
                if comp[d] < 0:
                    comp[d] = ncomp
                    todo.append(d)
        ncomp += 1
    needs = sorted({comp[cs[0]] for cs in checks_of if len(cs) == 1})
    virt = {k: C + i for i, k in enumerate(needs)}
    ends = np.array([[cs[0], cs[1] if len(cs) == 2 else virt[comp[cs[0]]]] for cs in checks_of],
                    np.int32)
    cvirt = [virt.get(comp[c], -1) for c in range(C)]
    return C + len(needs), ends, cvirt


def uf_ref_one(N, C, ends, cvirt, t):
    """One codeword: t [C] 0/1 -> (ehat [V] 0/1, rounds, status, nfull, set of facts)."""
    V = len(ends)
    facts = set()
    defect = [0] * N
    for c in range(C):
        defect[c] = int(t[c])
        if t[c] and cvirt[c] >= 0:
            defect[cvirt[c]] ^= 1
    if not any(t):
        facts.add('zero')
    up = list(range(N))                     # the disjoint-set forest
    top = list(range(N))                    # by set root: the highest vertex of the cluster
    parity = defect[:]                      # by set root: the XOR of its defects

    def find(u):
        while up[u] != u:
            up[u] = up[up[u]]
            u = up[u]
        return u

    grow = [0] * V
    rounds = status = 0
    while True:
        odd = {r for r in set(map(find, range(N))) if parity[r]}
        if not odd:
            break
        add = [(find(a) in odd) + (find(b) in odd) for a, b in ends]
        fresh = [v for v in range(V) if grow[v] < 2 <= grow[v] + add[v]]
        if not any(add[v] and grow[v] < 2 for v in range(V)):
            status = 1                      # an odd cluster that is a whole component
            break
        for v in range(V):
            grow[v] = min(2, grow[v] + add[v])
        rounds += 1
        for v in fresh:                     # explicit unions over the edges that just became full
            ra, rb = find(ends[v][0]), find(ends[v][1])
            if ra == rb:
                continue
            if parity[ra] and parity[rb]:
                facts.add('merge')
            up[ra] = rb
            top[rb] = max(top[ra], top[rb])
            parity[rb] ^= parity[ra]
    if rounds >= 3:
        facts.add('rounds3')
    # the forest: a breadth-first queue from each cluster's highest vertex
    full = [v for v in range(V) if grow[v] == 2]
    inc = collections.defaultdict(list)     # vertex -> [(edge, other end)], ascending edge
    for v in full:
        a, b = ends[v]
        inc[a].append((v, b))
        inc[b].append((v, a))
    depth, pedge, kids = {}, {}, collections.defaultdict(list)
    for root in sorted({top[find(u)] for u in inc}):
        if root >= C:
            facts.add('vroot')
        depth[root] = 0
        queue = collections.deque([root])
        while queue:
            u = queue.popleft()
            for _, w in inc[u]:
                if w not in depth:
                    depth[w] = depth[u] + 1
                    queue.append(w)
    for u in inc:
        if depth[u] == 0:
            continue
        cands = [v for v, w in inc[u] if depth[w] == depth[u] - 1]
        if len(cands) > 1:
            facts.add('tie')
        pedge[u] = min(cands)
        a, b = ends[pedge[u]]
        kids[b if a == u else a].append(u)
    ehat = [0] * V

    def subtree(u):
        s = defect[u]
        for k in kids[u]:
            sk = subtree(k)
            ehat[pedge[k]] = sk
            s ^= sk
        return s

    for u in inc:
        if depth[u] == 0:
            subtree(u)
    return ehat, rounds, status, len(full), facts


def syndrome(H, ehat):
    """H^T ehat mod 2 for ehat [B, V] -> [B, C] 0/1."""
    return (ehat.astype(np.int64) @ H.astype(np.int64)) % 2


@functools.lru_cache(maxsize=None)
def _inputs_all(shape):
    """x [B_ALL, V + C] float64: junk priors (the decoder must not read them), and on the check
    rows -/+ a magnitude in [0.5, 1.5] for a syndrome bit 1 / 0 of a random error pattern."""
    H = code_matrix(shape)
    V, C = H.shape
    rng = np.random.default_rng([SHAPES.index(shape), 20260])
    p = np.array([FLIP[b % len(FLIP)] for b in range(B_ALL)])
    e = rng.random((B_ALL, V)) < p[:, None]
    t = syndrome(H, e)
    x = np.empty((B_ALL, V + C))
    x[:, :V] = rng.normal(0.0, 3.0, (B_ALL, V))
    x[:, V:] = (1 - 2 * t) * rng.uniform(0.5, 1.5, (B_ALL, C))
    x.setflags(write=False)
    return x


def inputs(shape, B, dtype):
    """(H, x [B * N]) in dtype, read-only: the first B codewords of the shape's batch."""
    x = _inputs_all(shape)[:B].reshape(-1).astype(dtype)
    x.setflags(write=False)
    return code_matrix(shape), x


def uf_ref(H, x):
    """The statement on x [B * N] of any float dtype -> dict of ehat01 [B, V] uint8, rounds, status,
    nfull [B] int32, and facts (the union over the batch)."""
    V, C = H.shape
    N, ends, cvirt = matching_ref(H)
    xb = np.asarray(x).reshape(-1, V + C)
    B = xb.shape[0]
    res = dict(ehat01=np.zeros((B, V), np.uint8), rounds=np.zeros(B, np.int32),
               status=np.zeros(B, np.int32), nfull=np.zeros(B, np.int32), facts=set())
    pairs = [tuple(int(i) for i in ab) for ab in ends]
    for b in range(B):
        with np.errstate(invalid='ignore'):
            t = xb[b, V:] < 0
        ehat, res['rounds'][b], res['status'][b], res['nfull'][b], facts = uf_ref_one(
            N, C, pairs, cvirt, t)
        res['ehat01'][b] = ehat
        res['facts'] |= facts
    return res


@functools.lru_cache(maxsize=None)
def _reference_all(shape):
    H, x = inputs(shape, B_ALL, 'float64')
    res = uf_ref(H, x)
    V, C = H.shape
    # what the definition implies for any batch
    t = (x.reshape(B_ALL, V + C)[:, V:] < 0)
    assert not res['status'].any(), shape
    assert np.array_equal(syndrome(H, res['ehat01']), t), shape
    assert ((res['rounds'] == 0) == ~t.any(axis=1)).all() and (res['rounds'] <= 2 * V).all(), shape
    assert ((res['nfull'] == 0) == (res['rounds'] == 0)).all(), shape
    got = ' '.join(f for f in FACTS if f in res['facts'])
    assert got == COVERAGE[shape], (shape, got)
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def reference(shape, B, dtype):
    """(ehat [B * V] in dtype, rounds, status, nfull [B] int32) of inputs(shape, B, dtype): the
    first B codewords of the shape's one reference batch, whose recorded coverage is asserted."""
    r = _reference_all(shape)
    V = code_matrix(shape).shape[0]
    return (r['ehat01'][:B].reshape(B * V).astype(dtype), r['rounds'][:B], r['status'][:B],
            r['nfull'][:B])


def assert_required_coverage():
    assert set(COVERAGE) == set(SHAPES)
    for f in REQUIRED:
        assert any(f in cov.split() for cov in COVERAGE.values()), f


def assert_equal(got, ref, what=''):
    """(ehat, rounds, status, nfull) flat numpy arrays against another such tuple: exact, dtypes
    included."""
    for name, a, b in zip(('ehat', 'rounds', 'status', 'nfull'), got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape)
        assert np.array_equal(a, b), (what, name, np.nonzero(a != b)[0][:8].tolist())
