"""Shared by tests/test_relay_osd_cpu.py and tests/test_gpu_relay_osd.py: the numpy statement of the
soft relay definition (include/gnnd.h, gnnd_relay_soft), every operation a numpy operation on
values of the dtype (so each rounds once), layered on the relay statement of tests/relay_cases.py
(the loop is restated here because the accumulator lives inside it; reference() asserts that its
relay outputs are relay_cases.relay_ref's), and composed with the numpy OSD statement of
tests/osd_hi_cases.py / tests/bposd_cases.py into the statement of gnnd_relay_osd.

The reference asserts its own coverage for every (code, B, params) it serves, from the numpy
statement alone (the soft probability through numpy's exp):
  * both relay statuses occur in the batch;
  * at least one unsolved codeword has an OSD column order that differs between LAST and MEAN;
  * at least one unsolved codeword has a final ehat that differs between LAST and MEAN;
  * at least one gated codeword has choice > 0.
SEEDS holds the relay_cases.inputs seed of every (shape, parameter set): the first of seeds
0 .. 3999, searched on the CPU (with the host mirrors, then confirmed by reference() here), that
gives all four in both dtypes.  syn_sq64 (V = C = 64,
rank-deficient) is the exception: on 4 000 seeds per parameter set no unsolved codeword got a
different estimate from the two modes (the column orders differ, the lightest candidate does not),
so its seeds give the other three and reference() asserts that the estimates agree."""
import functools

import numpy as np

import bposd_cases as bc
import minsum_cases as mc
import osd_hi_cases as ohc
import relay_cases as rc

MODES = ('last', 'mean')
METHOD, ORDER = 'cs', 10
# (family, code, B) of the device comparisons -> the seed of relay_cases.inputs
SHAPES = (('plain', 'toric_5', 9), ('plain', 'toric_7', 9), ('plain', 'bch_63_45', 5),
          ('plain', 'ldpc_648_324', 3), ('plain', 'syn_hub', 9), ('hard', 'syn_sq64', 9))
P0, P1, P2, P3 = rc.PARAMS
SEEDS = {('toric_5', 9): {P0: 162, P1: 2, P2: 2, P3: 2},
         ('toric_7', 9): {P0: 10, P1: 8, P2: 16, P3: 2},
         ('bch_63_45', 5): {P0: 0, P1: 0, P2: 0, P3: 0},
         ('ldpc_648_324', 3): {P0: 0, P1: 1, P2: 0, P3: 0},
         ('syn_hub', 9): {P0: 178, P1: 66, P2: 43, P3: 0},
         ('syn_sq64', 9): {P0: 638, P1: 1, P2: 1, P3: 1}}
EHAT_SAME = ('syn_sq64',)


def family_of(code):
    return {c: f for f, c, _ in SHAPES}[code]


def base_of(code):
    """The OSD base the BP+OSD tests use: zero on the syndrome-style graphs, hard on the classical
    codes."""
    return 'zero' if mc.syndrome_style(code) else 'hard'


def inputs(code, B, dtype, params):
    """(H, x [B*N]) of relay_cases.inputs at the seed of this shape and parameter set."""
    return rc.inputs(family_of(code), code, B, dtype, SEEDS[(code, B)][params])


def relay_soft_ref(code, xb, g, iters0, iters_leg, S, alpha=rc.ALPHA, beta=rc.BETA):
    """relay_cases.relay_ref's loop with the accumulator of gnnd_relay_soft: A = +0 before leg 0,
    A = A + L after the variable step of every executed iteration.  Returns relay_ref's dict plus
    soft_last and soft_mean [B, V]: best.L where a solution was kept, else the last L (LAST) or
    round(A * inv) with inv = T(1 / (iters0 + (legs - 1) * iters_leg)) (MEAN)."""
    T = xb.dtype.type
    ev, chk, vptr, steps = rc._tables(code)
    H = rc.code_matrix(code).astype(np.int64)
    V = H.shape[0]
    B = xb.shape[0]
    a, bt, zero = T(alpha), T(beta), T(0)
    l = xb[:, :V]
    t = xb[:, V:] < zero
    legs = g.shape[0]
    M = l.copy()
    acc = np.zeros((B, V), xb.dtype)
    q = np.empty((B, ev.size), xb.dtype)
    best_L = np.zeros((B, V), xb.dtype)
    best_w = np.zeros(B, xb.dtype)
    leg = np.full(B, -1, np.int32)
    nsol = np.zeros(B, np.int32)
    total = np.zeros(B, np.int32)
    done = np.zeros(B, bool)
    with np.errstate(all='ignore'):
        for k in range(legs):
            gk = g[k]
            cl = (T(1) - gk) * l

            def lam(M):
                return np.where(gk == zero, l, cl + gk * M)

            act = ~done
            q[act] = lam(M)[:, ev][act]
            for it in range(iters0 if k == 0 else iters_leg):
                if not act.any():
                    break
                total[act] += 1
                r = rc._check_step(q, t, chk, a, bt)
                s = lam(M)
                for vs, es in steps:
                    s[:, vs] = s[:, vs] + r[:, es]
                M[act] = s[act]
                acc[act] = (acc + s)[act]                   # one addition in T
                q[act] = (s[:, ev] - r)[act]
                h = M < zero
                ok = (((h.astype(np.int64) @ H) % 2) == t).all(axis=1) & act
                for b in np.nonzero(ok)[0]:
                    w = rc.weight(h[b], l[b])
                    if nsol[b] == 0 or w < best_w[b]:
                        best_w[b], leg[b] = w, k
                        best_L[b] = M[b]
                    nsol[b] += 1
                act &= ~ok
            done |= nsol >= S
        inv = T(1.0 / float(iters0 + (legs - 1) * iters_leg))
        mean = acc * inv                                    # one multiply in T
    found = nsol > 0
    llr = np.where(found[:, None], best_L, M)
    return dict(llr=llr, ehat=(llr < zero).astype(xb.dtype), iters=total,
                status=(~found).astype(np.int32), leg=leg, nsol=nsol, soft_last=llr.copy(),
                soft_mean=np.where(found[:, None], best_L, mean))


def column_order(p, hard):
    """The OSD column order of one codeword's soft output p [V] (osd_hi_cases.eliminate's)."""
    key = -np.abs(p - 0.5) if hard else p.copy()
    key = np.where(np.isnan(key), -np.inf, key)
    return np.lexsort((np.arange(p.size), -key))


def osd_stage(code, x, pred, relay_status, llr, base=None, method=METHOD, order=ORDER):
    """The second stage of gnnd_relay_osd in numpy for a given soft probability pred [B*V]:
    (ehat [B, V] uint8, status, choice) = gnnd_osd on the gated codewords, the hard decision of llr
    passed through elsewhere."""
    H = rc.code_matrix(code)
    base = base_of(code) if base is None else base
    full = ohc.ref_batch(H, x, pred, base == 'hard', method, order)
    return bc.compose(full, relay_status, pred, llr, H.shape[0])


def _coverage(code, x, res):
    """The four conditions on one reference, as a dict of booleans."""
    st = res['status']
    V = rc.code_matrix(code).shape[0]
    hard = base_of(code) == 'hard'
    unsolved = np.nonzero(st == 1)[0]
    pl = res['pred_last'].reshape(-1, V)
    pm = res['pred_mean'].reshape(-1, V)
    return dict(
        both_statuses=set(st.tolist()) == {0, 1},
        order_differs=any(not np.array_equal(column_order(pl[b], hard), column_order(pm[b], hard))
                          for b in unsolved),
        ehat_differs=any(not np.array_equal(res['osd_last'][0][b], res['osd_mean'][0][b])
                         for b in unsolved),
        choice_positive=any(bool((res['osd_' + m][2][unsolved] > 0).any()) for m in MODES))


def _reference(code, B, dtype, params, seed):
    legs, iters0, iters_leg, S = params
    H, x = rc.inputs(family_of(code), code, B, dtype, seed)
    V, C = H.shape
    res = relay_soft_ref(code, x.reshape(B, V + C).copy(), rc.gammas(V, params, dtype), iters0,
                         iters_leg, S)
    for k in ('llr', 'ehat', 'soft_last', 'soft_mean'):
        res[k] = res[k].reshape(-1)
    for m in MODES:
        res['pred_' + m] = mc.soft_output(res['soft_' + m])
        res['osd_' + m] = osd_stage(code, x, res['pred_' + m], res['status'], res['llr'])
    return x, res


@functools.lru_cache(maxsize=None)
def reference(code, B, dtype, params):
    """The numpy statement on inputs(code, B, dtype, params) with relay_cases.gammas(V, params,
    dtype): a dict of read-only arrays: relay's six outputs, soft_last / soft_mean [B*V], pred_last /
    pred_mean (numpy's exp) and osd_last / osd_mean = (ehat [B, V] uint8, status, choice) on those.
    Asserts that the relay outputs are relay_cases.relay_ref's (V <= 128) and what the batch must
    hold."""
    legs, iters0, iters_leg, S = params
    x, res = _reference(code, B, dtype, params, SEEDS[(code, B)][params])
    H = rc.code_matrix(code)
    V, C = H.shape
    tag = (code, B, dtype, params)
    if V <= 128:            # the larger codes: tests/test_relay_osd_cpu.py holds both to the mirrors
        plain = rc.relay_ref(code, x.reshape(B, V + C).copy(), rc.gammas(V, params, dtype), iters0,
                             iters_leg, S)
        for k in rc.OUTPUTS:
            assert np.array_equal(res[k].reshape(-1), plain[k].reshape(-1)), (tag, k)
    solved = res['status'] == 0
    for m in MODES:
        assert np.array_equal(res['soft_' + m].reshape(B, V)[solved],
                              res['llr'].reshape(B, V)[solved]), (tag, m)
    assert np.array_equal(res['soft_last'], res['llr']), tag
    cov = _coverage(code, x, res)
    if code in EHAT_SAME:
        cov['ehat_differs'] = not cov['ehat_differs']
    assert all(cov.values()), (tag, cov)
    for arr in res.values():
        for a in (arr if isinstance(arr, tuple) else (arr,)):
            a.setflags(write=False)
    return res


def search_seed(code, B, params, seeds=range(4000)):
    """The first seed whose batch gives the four conditions in both dtypes (how SEEDS was filled;
    slow on the larger codes)."""
    for seed in seeds:
        if all(all(_coverage(code, *_reference(code, B, dt, params, seed)).values())
               for dt in ('float64', 'float32')):
            return seed
    return None
