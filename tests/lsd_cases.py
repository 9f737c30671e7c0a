"""Shared by tests/test_lsd_cpu.py, tests/test_gpu_lsd.py and tests/decoder_debug_worker.py: an
independent numpy statement of localized-statistics decoding (include/gnnd.h, gnnd_lsd), written
from the definition with sets and dense matrices, and the seeded inputs of tests/osd_cases.py
and tests/minsum_cases.py on the shipped codes and the synthetic graphs.  The statement also
returns the final cluster variables (inV) and whether a valid cluster sat out a round in which
another grew.  The coverage facts the tests rely on are asserted at import."""
import functools

import numpy as np

import bposd_cases as bc
import minsum_cases as mc
import osd_cases as oc
import synthetic_codes

# (code, B): the shipped codes with the batches of bposd_cases.SHAPES, then the synthetic graphs
SHAPES = bc.SHAPES + synthetic_codes.OSD_SHAPES
BITS = (0, 1, 3)
NAMES = ('ehat', 'status', 'rounds', 'nclus', 'ncols')


def lsd_ref(H, t, p, hard, bits):
    """One codeword: H [V, C] 0/1, t [C] target syndrome, p [V] soft output -> dict with ehat
    (uint8 [V]), status, rounds, nclus, ncols, inV (bool [V]) and sat_out."""
    V, C = H.shape
    Hb = H.astype(bool)
    z = (p > 0.5).astype(np.uint8) if hard else np.zeros(V, np.uint8)
    key = -np.abs(p - 0.5) if hard else p.copy()
    key = np.where(np.isnan(key), -np.inf, key)
    order = np.lexsort((np.arange(V), -key))
    s = (t ^ (H.T.astype(np.int64) @ z % 2)).astype(np.uint8)
    inV = np.zeros(V, bool)
    inC = s.astype(bool)
    label = np.arange(C)
    out = dict(ehat=z, status=0, rounds=0, nclus=0, ncols=0, inV=inV, sat_out=False)
    if not s.any():
        return out
    invalid = set()
    while True:
        out['rounds'] += 1
        if out['rounds'] == 1:
            active = inC.copy()
        else:
            active = inC & np.isin(label, sorted(invalid))
        joined = set()
        for K in sorted(set(label[active].tolist())):
            at_K = Hb[:, active & (label == K)].any(axis=1) & ~inV
            cand = order[at_K[order]].tolist()
            joined |= set(cand if bits == 0 else cand[:bits])
        if out['rounds'] > 1 and joined and set(label[inC].tolist()) - invalid:
            out['sat_out'] = True
        if not joined:
            out['status'] = 1
            break
        inV[sorted(joined)] = True
        inC |= Hb[inV].any(axis=0)
        for v in np.nonzero(inV)[0]:                 # union by the smallest check index
            ls = label[Hb[v]]
            label[np.isin(label, ls)] = ls.min()
        # gnnd_osd0's elimination over the cluster columns, in `order` order: a skipped column is
        # never a pivot and never read, so the matrix of the walked columns alone is the same walk
        cols = [v for v in order if inV[v]]
        A = np.packbits(H.T[:, cols].astype(np.uint8), axis=1)     # column i: bit 7 - i % 8 of byte i // 8
        sw = s.copy()
        used = np.zeros(C, bool)
        piv = []
        for i, j in enumerate(cols):
            m = ((A[:, i >> 3] >> (7 - (i & 7))) & 1).astype(bool)
            rows = np.nonzero(m & ~used)[0]
            if rows.size == 0:
                continue
            r = rows[0]
            used[r] = True
            piv.append((r, j))
            m[r] = False
            A[m] ^= A[r]
            sw[m] ^= sw[r]
        bad = ~used & sw.astype(bool)
        if not bad.any():
            e = np.zeros(V, np.uint8)
            for r, j in piv:
                e[j] = sw[r]
            out['ehat'] = z ^ e
            break
        assert inC[bad].all()
        invalid = set(label[bad].tolist())
    out['nclus'] = len(set(label[inC].tolist()))
    out['ncols'] = int(inV.sum())
    return out


def ref_batch(H, x, p, hard, bits):
    """lsd_ref over a batch: x [B*N], p [B*V] -> dict of arrays (ehat [B, V] uint8, the int32 [B]
    outputs, inV [B, V] bool, sat_out [B] bool)."""
    V, C = H.shape
    pb = p.reshape(-1, V)
    with np.errstate(invalid='ignore'):
        t = (x.reshape(-1, V + C)[:, V:] < 0).astype(np.uint8)
    rows = [lsd_ref(H, t[b], pb[b], hard, bits) for b in range(pb.shape[0])]
    res = {k: np.stack([r[k] for r in rows]) for k in ('ehat', 'inV')}
    res.update({k: np.array([r[k] for r in rows], np.int32) for k in NAMES[1:]})
    res['sat_out'] = np.array([r['sat_out'] for r in rows])
    return res


@functools.lru_cache(maxsize=None)
def reference(code, B, dtype, base, bits):
    """The statement on osd_cases.inputs(code, B, dtype); read-only arrays."""
    H, x, p = oc.inputs(code, B, dtype)
    res = ref_batch(H, x, p, base == 'hard', bits)
    for a in res.values():
        a.setflags(write=False)
    return res


def as_tuple(res, dtype):
    """The five outputs in the order of ops.lsd, ehat flat in `dtype`."""
    return (res['ehat'].reshape(-1).astype(dtype),) + tuple(res[k] for k in NAMES[1:])


def assert_equal(got, want, what=''):
    """Exact equality of the five outputs (flat arrays), with their dtypes."""
    for name, a, b in zip(NAMES, got, want):
        a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, name)


# ---- BP+LSD: the batch and the min-sum parameters of tests/bposd_cases.py ----
BP_SHAPE, BP_B = 'toric_5', 67


def bp_inputs(dtype):
    """(H, x) of minsum_cases.inputs on toric-5, B = 67, and the min-sum parameters."""
    H, x = mc.inputs(BP_SHAPE, BP_B, dtype)
    alpha, beta, iters, early = bc.bp_params(BP_SHAPE)
    return H, x, (iters, alpha, beta, bool(early))


def hand_case(L, flips):
    """toric(L) with the given variables flipped and pred high on exactly them -> (H, x, p) in
    float64, one codeword."""
    H = oc.code_matrix(f'toric_{L}')
    V, C = H.shape
    e = np.zeros(V, np.int64)
    e[list(flips)] = 1
    x = np.ones(V + C)
    x[V:] = 1 - 2 * ((e @ H.astype(np.int64)) % 2)
    p = np.full(V, 0.01)
    p[list(flips)] = 0.9
    return H, x, p


@functools.lru_cache(maxsize=None)
def _check_inputs():
    """The coverage facts, each on the seed-0 inputs (no other seed or p was needed)."""
    t5 = {k: reference('toric_5', 67, 'float64', 'zero', k) for k in (0, 1)}
    assert (reference('bch_63_45', 33, 'float64', 'zero', 1)['rounds'] == 0).all()   # t = 0, z = 0
    assert (t5[1]['rounds'] >= 3).any()
    assert (t5[1]['nclus'] >= 2).any()
    tall = reference('syn_tall', 9, 'float64', 'zero', 1)
    assert tall['status'][1::2].any() and not tall['status'][0::2].any()
    ok = (t5[0]['status'] == 0) & (t5[1]['status'] == 0)
    assert (t5[0]['ehat'][ok] != t5[1]['ehat'][ok]).any()
    assert t5[1]['sat_out'].any()
    return True


_check_inputs()
