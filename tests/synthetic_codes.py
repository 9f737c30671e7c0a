"""Seeded synthetic parity-check matrices for tests/test_synthetic_graphs_cpu.py and
tests/test_gpu_synthetic_graphs.py: small irregular Tanner graphs, each built to reach one launch
plan branch or loop shape of the min-sum, layered, relay and OSD kernels that the shipped codes
(toric-5, toric-7, BCH(63,45), LDPC(648,324)) never reach.  Every matrix asserts the properties
that make it worth having, so a change of recipe that loses the coverage fails here.

  syn_wide   a greedy layer of 80 checks (more than the 64 lanes of a wave: the layered kernel's
             layer loop runs twice per lane), three isolated variables
  syn_hub    four hub variables of degree 37 or 38 (long sums in edge order), 38 layers of at most
             4 checks, and a codeword tile of which eight fit 64 KiB in fp32 but not in fp64 (the
             layered plan's LDS-driven doubling of the lanes per codeword)
  syn_tall   C = 70 > V = 40 with full column rank: the elimination ends on the last column, unused
             rows remain and there is no free column; V < 64 with C > 64
  syn_sq64   V = C = 64 (exact word and wave boundaries), rank-deficient, degree-0 variables and
             degree-2 checks
  syn_c65    C = 65: one row alone in the second row slot of the elimination"""
import functools

import numpy as np

NAMES = ('syn_wide', 'syn_hub', 'syn_tall', 'syn_sq64', 'syn_c65')

# The cases the CPU tests, the GPU tests and tests/synthetic_debug_worker.py share.
# (code, B) of min-sum on both schedules: the last wave is partial.  syn_hub holds 8 (fp32) or 4
# (fp64) codewords per wave of the layered kernel: B = 11 is a full wave and three active groups
MINSUM_SHAPES = (('syn_wide', 5), ('syn_hub', 1), ('syn_hub', 11), ('syn_tall', 9),
                 ('syn_sq64', 9), ('syn_c65', 9))
# (family, code, B) of tests/relay_cases.py, each with PARAMS[1] and PARAMS[3]
RELAY_CASES = (('plain', 'syn_hub', 9), ('hard', 'syn_tall', 9), ('hard', 'syn_sq64', 9))
RELAY_PARAMS = (1, 3)
# (code, B) of OSD; every method in both bases
OSD_SHAPES = (('syn_tall', 9), ('syn_sq64', 9), ('syn_c65', 9), ('syn_wide', 5))
OSD_METHODS = (('osd0', 0), ('cs', 10), ('e', 8))
# (code, B) of BP+OSD on both schedules, ('cs', 10)
BPOSD_SHAPES = (('syn_hub', 11), ('syn_tall', 9))


def is_synthetic(name):
    return name.startswith('syn_')


def gf2_rank(H):
    """Rank over GF(2) of H [V, C]."""
    A = (np.asarray(H).T % 2).astype(np.uint8)
    rank = 0
    for j in range(A.shape[1]):
        rows = np.nonzero(A[rank:, j])[0]
        if rows.size == 0:
            continue
        r = rank + rows[0]
        A[[rank, r]] = A[[r, rank]]
        m = A[:, j].astype(bool)
        m[rank] = False
        A[m] ^= A[rank]
        rank += 1
        if rank == A.shape[0]:
            break
    return rank


def greedy_layers(H):
    """Checks in ascending c, layer(c) the smallest k such that no earlier check of layer k shares
    a variable with c: the rule of gnnd_graph_layers, by a per-layer occupancy mask."""
    Hb = np.asarray(H).astype(bool)
    taken = []                                               # per layer: the variables in use
    layer = np.zeros(Hb.shape[1], np.int32)
    for c in range(Hb.shape[1]):
        k = 0
        while k < len(taken) and (taken[k] & Hb[:, c]).any():
            k += 1
        if k == len(taken):
            taken.append(np.zeros(Hb.shape[0], bool))
        taken[k] |= Hb[:, c]
        layer[c] = k
    return layer


def _wide():
    rng = np.random.default_rng(1)
    H = np.zeros((243, 120), np.uint8)
    for c in range(80):
        H[3 * c:3 * c + 3, c] = 1
    for c in range(80, 120):
        H[rng.choice(240, 4, replace=False), c] = 1
    sizes = np.bincount(greedy_layers(H))
    assert sizes.tolist()[0] == 80 and sizes.max() == 80 and sizes.size == 4, sizes.tolist()
    assert (H.sum(1) == 0).sum() == 3 and not H[240:].any()
    assert gf2_rank(H) == 120
    return H


def _hub():
    rng = np.random.default_rng(2)
    H = np.zeros((300, 150), np.uint8)
    for c in range(150):
        H[c % 4, c] = 1
        H[4 + rng.choice(296, 5, replace=False), c] = 1
    sizes = np.bincount(greedy_layers(H))
    assert int(H.sum()) == 900 and (H.sum(0) == 6).all()
    assert sizes.max() == 4 and sizes.size == 38, sizes.tolist()
    assert H.sum(1)[:4].tolist() == [38, 38, 37, 37] and H.sum(1)[4:].max() <= 12
    # one codeword's layered tile: r[E] and L[V], each rounded up to 16 bytes, made an odd number
    # of 16-byte units; eight of them fit 64 KiB in fp32, not in fp64
    for elem, fits in ((4, True), (8, False)):
        tile = 900 * elem + 300 * elem
        assert tile % 16 == 0
        tile += 16 * (1 - (tile // 16) % 2)
        assert (8 * tile <= 65536) == fits and 4 * tile <= 65536
    return H


def _tall():
    rng = np.random.default_rng(3)
    H = np.zeros((40, 70), np.uint8)
    for c in range(70):
        H[rng.choice(40, 3, replace=False), c] = 1
    assert gf2_rank(H) == 40                                 # full column rank: no free column
    assert (H.sum(1) > 0).all()
    return H


def _ragged(seed, V, C):
    rng = np.random.default_rng(seed)
    H = np.zeros((V, C), np.uint8)
    for c in range(C):
        H[rng.choice(V, int(rng.integers(2, 7)), replace=False), c] = 1
    dc = H.sum(0)
    assert dc.min() == 2 and dc.max() == 6
    return H


def _sq64():
    H = _ragged(4, 64, 64)
    assert gf2_rank(H) == 62
    assert (H.sum(1) == 0).any()
    return H


def _c65():
    H = _ragged(5, 96, 65)
    assert gf2_rank(H) == 65
    return H


_BUILD = {'syn_wide': _wide, 'syn_hub': _hub, 'syn_tall': _tall, 'syn_sq64': _sq64,
          'syn_c65': _c65}


@functools.lru_cache(maxsize=None)
def matrix(name):
    """H [V, C] uint8 of a synthetic graph, read-only."""
    H = np.ascontiguousarray(_BUILD[name]())
    assert H.dtype == np.uint8 and (H.sum(0) >= 2).all()
    H.setflags(write=False)
    return H
