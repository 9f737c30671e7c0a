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


# ------------------------------------------------------------------------------------------------
# Graphs for the fused decoders (gnnd_decode): tests/test_decode_synthetic_cpu.py and
# tests/test_gpu_decode_synthetic.py.  The shipped codes reach five launch plans; these reach the
# rest of make_plan / launch_decode.  (G, R) below is the resident slot plan (tie preference 1).
#
#   syn_leaf   checks of degree 1 and 0, a variable of degree 0, max check degree <= 6: fp32/fp64
#              cbp and qbp leave the resident kernel (ratio_bad), cgnni / qgnni stay on it
#   syn_g8     check degrees ragged in 2 .. 20: (8, 3), padded with padr = R
#   syn_g16    check degrees ragged, max 40: (16, 3), the largest resident group
#   syn_g32    max check degree 70: (32, 3), every light model on the streaming kernel
#   syn_g64    max check degree 100: preference 0 and 2 give (64, 2), the only way decoder_v2_4
#              runs an R = 2 plan (slot_plan's docstring has the arithmetic)
#   syn_full8  every check of degree 8, variable degrees ragged, V = 150: unpadded off the toric
#              code; preference 0 gives (8, 1), 1 gives (2, 4), 2 gives (4, 2)
#   syn_pad1   every check of degree 5 or 6: (2, 3) with padr = 1
#   syn_twin   two copies of one connected ragged graph: the component split
#   syn_two    two different connected components of one shape
# ------------------------------------------------------------------------------------------------
DECODE_NAMES = NAMES + ('syn_leaf', 'syn_g8', 'syn_g16', 'syn_g32', 'syn_g64', 'syn_full8',
                        'syn_pad1', 'syn_twin', 'syn_two')


def slot_plan(max_dc, pref):
    """(G, R) of build_plan (gnnd_graph.hip) for the largest check degree: R slots per lane, G = the
    power of two >= ceil(max_dc / R) lanes per check, fewest slots G * R; ties go to the smaller R
    (pref 0), the larger R (pref 1) or to R = 2 over a smaller R (pref 2).  None: degree > 256.
    With p(n) the power of two >= n, p(d) <= 2 p(ceil(d / 2)), so R = 2 never beats R = 1 and
    preference 0 takes R = 2 only where R = 1 needs G > 64 and R = 3 is no better: 97 <= d <= 128."""
    best = None
    for R in (1, 2, 3, 4):
        G = 1
        while G < -(-max_dc // R):
            G *= 2
        if G > 64:
            continue
        tie_wins = pref == 1 or (pref == 2 and R == 2)
        if best is None or G * R < best[0] * best[1] or (tie_wins and G * R == best[0] * best[1]):
            best = (G, R)
    return best


def slot_form(H, pref):
    """(G, R, padding form) of a graph's slot plan: 'none', 'one' (padr == 1) or 'R' (launch_decode's
    three padding templates)."""
    dc = np.asarray(H).sum(0).astype(int)
    G, R = slot_plan(int(dc.max()), pref)
    padr = int(np.minimum(R, G * R - dc).max())
    return G, R, 'none' if padr == 0 else 'one' if padr == 1 else 'R'


def components(H):
    """Number of connected components of the Tanner graph, variables of degree 0 and checks of
    degree 0 counted as components of their own."""
    Hb = np.asarray(H).astype(bool)
    V, C = Hb.shape
    seen = np.zeros(V + C, bool)
    n = 0
    for s in range(V + C):
        if seen[s]:
            continue
        n += 1
        seen[s] = True
        todo = [s]
        while todo:
            u = todo.pop()
            nb = np.nonzero(Hb[u])[0] + V if u < V else np.nonzero(Hb[:, u - V])[0]
            for w in nb[~seen[nb]]:
                seen[w] = True
                todo.append(int(w))
    return n


def _degrees(seed, V, degrees):
    """H [V, len(degrees)]: check c on degrees[c] distinct random variables."""
    rng = np.random.default_rng(seed)
    H = np.zeros((V, len(degrees)), np.uint8)
    for c, d in enumerate(degrees):
        H[rng.choice(V, int(d), replace=False), c] = 1
    assert np.array_equal(H.sum(0), np.asarray(degrees))
    return H


def _leaf():
    rng = np.random.default_rng(11)
    H = np.zeros((96, 66), np.uint8)
    for c in range(64):
        H[rng.choice(95, int(rng.integers(2, 7)), replace=False), c] = 1
    H[7, 64] = 1                                             # a check of degree 1; check 65: none
    dc, dv = H.sum(0), H.sum(1)
    assert dc[64] == 1 and dc[65] == 0 and dc.max() == 6 and dv[95] == 0
    assert slot_form(H, 1) == (2, 3, 'R')
    return H


def _ragged_max(seed, V, C, top):
    rng = np.random.default_rng(seed)
    deg = rng.integers(2, top + 1, C)
    deg[0], deg[1] = top, 2
    H = _degrees(seed + 100, V, deg)
    assert H.sum(0).max() == top and np.unique(H.sum(0)).size >= 5
    assert H.shape[0] <= 320 and H.sum() <= 1000
    return H


def _g8():
    H = _ragged_max(12, 200, 48, 20)
    assert slot_form(H, 1) == (8, 3, 'R') and slot_form(H, 0)[:2] == (8, 3)
    return H


def _g16():
    H = _ragged_max(13, 200, 16, 40)
    assert slot_form(H, 1) == (16, 3, 'R') and slot_form(H, 0)[:2] == (16, 3)
    return H


def _g32():
    H = _ragged_max(14, 160, 12, 70)
    assert all(slot_form(H, p)[:2] == (32, 3) for p in (0, 1, 2))
    return H


def _g64():
    H = _ragged_max(18, 128, 8, 100)
    assert slot_form(H, 0)[:2] == (64, 2) and slot_form(H, 2)[:2] == (64, 2)
    assert slot_form(H, 1)[:2] == (32, 4)
    return H


def _full8():
    H = _degrees(15, 150, [8] * 48)
    dv = H.sum(1)
    assert H.shape[0] % 64 and np.unique(dv).size >= 4
    assert [slot_form(H, p) for p in (0, 1, 2)] == [(8, 1, 'none'), (2, 4, 'none'), (4, 2, 'none')]
    return H


def _pad1():
    rng = np.random.default_rng(16)
    H = _degrees(116, 128, rng.integers(5, 7, 64))
    assert set(H.sum(0).tolist()) == {5, 6} and slot_form(H, 1) == (2, 3, 'one')
    return H


def _component(seed, V=40, C=24, extra=22):
    """A connected ragged graph: a chain (check c on variables c and c + 1), every further variable
    on one random check, then `extra` random edges that keep every check degree <= 6 and bring
    check 0 to exactly 6."""
    rng = np.random.default_rng(seed)
    H = np.zeros((V, C), np.uint8)
    for c in range(C):
        H[c, c] = H[c + 1, c] = 1
    for v in range(C + 1, V):
        H[v, int(rng.integers(1, C))] = 1
    left = extra
    while left:
        v, c = int(rng.integers(V)), 0 if H[:, 0].sum() < 6 else int(rng.integers(1, C))
        if not H[v, c] and H[:, c].sum() < 6:
            H[v, c] = 1
            left -= 1
    assert components(H) == 1 and H.sum() == 2 * C + (V - C - 1) + extra
    assert H.sum(0).max() == 6 and H.sum(0).min() >= 2 and np.unique(H.sum(0)).size >= 4
    return H


def _block2(A, B):
    H = np.zeros((A.shape[0] + B.shape[0], A.shape[1] + B.shape[1]), np.uint8)
    H[:A.shape[0], :A.shape[1]] = A
    H[A.shape[0]:, A.shape[1]:] = B
    assert components(H) == 2
    return H


def _twin():
    A = _component(17)
    return _block2(A, A)


def _two():
    A, B = _component(17), _component(20)
    # one shape (V, C, E, largest degrees, padding form: what the split compares), other edges
    assert A.shape == B.shape and A.sum() == B.sum() and not np.array_equal(A, B)
    assert slot_form(A, 1) == slot_form(B, 1) and A.sum(1).max() == B.sum(1).max()
    return _block2(A, B)


_BUILD_DECODE = {'syn_leaf': _leaf, 'syn_g8': _g8, 'syn_g16': _g16, 'syn_g32': _g32, 'syn_g64': _g64,
                 'syn_full8': _full8, 'syn_pad1': _pad1, 'syn_twin': _twin, 'syn_two': _two}


@functools.lru_cache(maxsize=None)
def decode_matrix(name):
    """H [V, C] uint8 of a graph of DECODE_NAMES, read-only."""
    if name in NAMES:
        return matrix(name)
    H = np.ascontiguousarray(_BUILD_DECODE[name]())
    assert H.dtype == np.uint8 and H.shape[0] <= 320 and int(H.sum()) <= 1000
    H.setflags(write=False)
    return H


CLASSICAL = ('cgnni', 'cbp')


def decode_inputs(name, model, B, seed=0):
    """x [B * N, 1] of the model's own dtype (fp32 classical, fp64 quantum).  Classical: the all-zeros
    word over AWGN at 1 .. 6 dB, LLR = 2 y / sigma^2, zeros on the check rows.  Quantum: errors of
    rate p in {0.01, 0.05, 0.1} per codeword, the prior log((1 - p) / p) on the variable rows and
    the syndrome as +-1 on the check rows."""
    H = decode_matrix(name)
    V, C = H.shape
    rng = np.random.default_rng([seed, DECODE_NAMES.index(name), B])
    if model in CLASSICAL:
        sigma = np.sqrt(10.0 ** (-(1 + np.arange(B) % 6) / 10.0))[:, None]
        llr = 2 * (1 + sigma * rng.standard_normal((B, V))) / sigma ** 2
        x = np.concatenate([llr, np.zeros((B, C))], 1).astype(np.float32)
    else:
        p = np.array([0.01, 0.05, 0.1])[np.arange(B) % 3][:, None]
        e = (rng.random((B, V)) < p).astype(np.int64)
        syn = (e @ H.astype(np.int64)) % 2
        x = np.concatenate([np.broadcast_to(np.log((1 - p) / p), (B, V)), 1.0 - 2.0 * syn], 1)
    return np.ascontiguousarray(x.reshape(-1, 1))


# (graph, model, dtype, kernel, items_per_lane, var_group): the launch plan ops.decode_plan reports,
# derived from make_plan (gnnd_decode_impl.h) and confirmed on an MI355X.  'R' = the resident
# kernel, 'S' = the streaming kernel (items_per_lane and var_group 0).  The parity tests decode
# every one of these cases.
DECODE_PLAN_CASES = (
    ('syn_tall', 'cgnni', 'float32', 'R', 6, 1),
    ('syn_leaf', 'cgnni', 'float32', 'R', 9, 1),
    ('syn_g8', 'cgnni', 'float32', 'R', 9, 1),
    ('syn_g16', 'cgnni', 'float32', 'R', 9, 1),
    ('syn_g32', 'cgnni', 'float32', 'S', 0, 0),
    ('syn_full8', 'cgnni', 'float32', 'R', 3, 8),
    ('syn_pad1', 'cgnni', 'float32', 'R', 6, 1),
    ('syn_leaf', 'cbp', 'float32', 'S', 0, 0),
    ('syn_g16', 'cbp', 'float32', 'R', 9, 1),
    ('syn_g32', 'cbp', 'float32', 'S', 0, 0),
    ('syn_full8', 'cbp', 'float32', 'R', 3, 8),
    ('syn_leaf', 'qbp', 'float32', 'S', 0, 0),
    ('syn_g8', 'qbp', 'float32', 'R', 9, 1),
    ('syn_g32', 'qbp', 'float32', 'S', 0, 0),
    ('syn_leaf', 'qbp', 'float64', 'S', 0, 0),
    ('syn_g8', 'qbp', 'float64', 'R', 6, 16),
    ('syn_g32', 'qbp', 'float64', 'S', 0, 0),
    ('syn_full8', 'qbp', 'float64', 'R', 3, 8),
    ('syn_leaf', 'qgnni', 'float32', 'R', 9, 1),
    ('syn_pad1', 'qgnni', 'float32', 'R', 6, 1),
    ('syn_g16', 'qgnni', 'float32', 'R', 9, 1),
    ('syn_g32', 'qgnni', 'float32', 'S', 0, 0),
    ('syn_leaf', 'qgnni', 'float64', 'R', 6, 1),
    ('syn_g8', 'qgnni', 'float64', 'R', 6, 16),
    ('syn_g32', 'qgnni', 'float64', 'S', 0, 0),
    ('syn_full8', 'qgnni', 'float64', 'R', 3, 8),
    ('syn_twin', 'qgnni', 'float64', 'R', 6, 4),
    ('syn_leaf', 'nbp', 'float64', 'R', 6, 1),
    ('syn_g8', 'nbp', 'float64', 'R', 6, 1),
    ('syn_g32', 'nbp', 'float64', 'S', 0, 0),
    ('syn_full8', 'nbp', 'float64', 'R', 3, 1),
    ('syn_g16', 'v10', 'float64', 'R', 6, 1),
    ('syn_g32', 'v10', 'float64', 'S', 0, 0),
    ('syn_pad1', 'v10', 'float64', 'R', 6, 1),
    ('syn_leaf', 'v30', 'float64', 'S', 0, 0),
    ('syn_g16', 'v30', 'float64', 'S', 0, 0),
    ('syn_full8', 'v30', 'float64', 'S', 0, 0),
    ('syn_full8', 'v24', 'float32', 'S', 0, 0),
    ('syn_hub', 'v24', 'float32', 'S', 0, 0),
    ('syn_g64', 'v24', 'float32', 'S', 0, 0),
    ('syn_leaf', 'v24', 'float32', 'S', 0, 0),
    ('syn_full8', 'v24', 'float64', 'S', 0, 0),
    ('syn_hub', 'v24', 'float64', 'S', 0, 0),
    ('syn_leaf', 'v24', 'float64', 'S', 0, 0),
)
DECODE_ITERS = (0, 1, 4)
LIGHT = ('cgnni', 'cbp', 'qbp', 'qgnni', 'nbp', 'v10')           # make_plan's light models (+ v22)
# decoder_v2_4's batches: each threshold of make_plan crossed (256, 512, 4 096)
V24_BATCHES = (1, 67, 300, 600, 4097)
# (graph, B) of the component split, decoder_v2_4 in fp32 and fp64
SPLIT_GRAPHS = ('syn_twin', 'syn_two')
SPLIT_BATCHES = (3, 300)
# one resident and one streaming plan per model (decoder_v2_4 and decoder_v3_0: streaming only)
POSITION_CASES = tuple(c for c in DECODE_PLAN_CASES if c[:3] in (
    ('syn_g8', 'cgnni', 'float32'), ('syn_g32', 'cgnni', 'float32'),
    ('syn_full8', 'cbp', 'float32'), ('syn_leaf', 'cbp', 'float32'),
    ('syn_g8', 'qbp', 'float64'), ('syn_g32', 'qbp', 'float32'),
    ('syn_full8', 'qgnni', 'float64'), ('syn_g32', 'qgnni', 'float64'),
    ('syn_g8', 'nbp', 'float64'), ('syn_g32', 'nbp', 'float64'),
    ('syn_g16', 'v10', 'float64'), ('syn_g32', 'v10', 'float64'),
    ('syn_leaf', 'v30', 'float64'), ('syn_g64', 'v24', 'float32'), ('syn_hub', 'v24', 'float64')))

REQUIRED_BRANCHES = frozenset(
    [f'resident G={G}' for G in (1, 2, 8, 16)]
    + [f'resident padding {f}' for f in ('none', 'one', 'R')]
    + ['var_group 1', 'var_group > 1']
    + [f'streaming {m}: G > 16' for m in LIGHT]
    + [f'streaming {m}: ratio_bad' for m in ('cbp', 'qbp')]
    + [f'v24 R={R}' for R in (1, 2, 3)])


def v24_form(name, dtype, B):
    """(G, R, unit split) of make_plan's decoder_v2_4 kernel at batch B: fp64 runs preference 0's
    plan; fp32 the same up to B = 4 096 where it has R = 1, else preference 2's where that has
    R = 2, else preference 1's.  Plans with R <= 2 split the MLP units over 4 waves up to B = 256
    and over 2 up to B = 512 (there one codeword runs per workgroup)."""
    H = decode_matrix(name)
    G, R = slot_form(H, 0)[:2]
    if dtype == 'float32' and not (B <= 4096 and R == 1):
        G, R = slot_form(H, 2)[:2] if B <= 4096 and slot_form(H, 2)[1] == 2 else slot_form(H, 1)[:2]
    return G, R, (4 if B <= 256 else 2 if B <= 512 else 1) if R <= 2 else 1


def case_branches(case):
    """The names of REQUIRED_BRANCHES a case of DECODE_PLAN_CASES reaches, from the host mirrors."""
    name, model, dtype, kernel, q, vg = case
    H = decode_matrix(name)
    G, R, form = slot_form(H, 1)
    if model == 'v24':
        return {f'v24 R={v24_form(name, dtype, B)[1]}' for B in V24_BATCHES}
    if kernel == 'R':
        assert G <= 16 and q in (3, 6, 9, 12) and vg >= 1
        return {f'resident G={G}', f'resident padding {form}',
                'var_group 1' if vg == 1 else 'var_group > 1'}
    out = set()
    if model in LIGHT and G > 16:
        out.add(f'streaming {model}: G > 16')
    elif model in ('cbp', 'qbp') and H.sum(0).min() < 2:
        out.add(f'streaming {model}: ratio_bad')
    return out
