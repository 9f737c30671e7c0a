"""Worker for the test_debug_library_runs_*_clean tests of the post-processing and BP decoder
modules (a child process with GNND_LIB pointing at libgnnd_debug.so, tests/debug_child.py): runs
the family named on the command line through its ops and prints one JSON line with the debug flags
and, per case, whether every output equals the family's reference bit for bit.  Each family imports
its own case modules, so a child loads what its family needs and no more."""
import sys

import numpy as np
import torch

from debug_child import DEV, on_dev, report, same  # first: it puts the package on sys.path
import gnndecode as gd  # noqa: E402
from gnndecode import ops  # noqa: E402


def osd():
    """One toric-5 OSD-0 case in both bases against the numpy reference."""
    import osd_cases as oc
    B = 5
    H, x, p = oc.inputs('toric_5', B, 'float64')
    g = gd.TannerGraph(H, device=DEV)
    equal = {}
    for base in ('zero', 'hard'):
        ehat, status = ops.osd0(g, on_dev(x), on_dev(p), base)
        ref_e, ref_s = oc.reference('toric_5', B, 'float64', base)
        equal[base] = bool(np.array_equal(ehat.cpu().numpy().reshape(B, -1), ref_e)
                           and np.array_equal(status.cpu().numpy(), ref_s))
    return equal


def osd_hi():
    """(cs, 10) and (e, 8) on toric-7 and the rank-deficient BCH graph against the numpy
    reference."""
    import osd_hi_cases as hc
    equal = {}
    for code, B, dtype, base in (('toric_7', 9, 'float64', 'zero'), ('bch_dup', 4, 'float32', 'hard')):
        H, x, p = hc.inputs(code, B, dtype)
        g = gd.TannerGraph(H, device=DEV)
        for method, order in (('cs', 10), ('e', 8)):
            got = ops.osd(g, on_dev(x), on_dev(p), base, method, order)
            ref = hc.reference(code, B, dtype, base, method, order)
            equal[f'{code}_{method}'] = bool(all(
                np.array_equal(a.cpu().numpy().reshape(r.shape), r) for a, r in zip(got, ref)))
    return equal


def _minsum(cases, schedule, ldpc_B):
    """llr, iteration counts and statuses of ops.minsum against the numpy reference; on the layered
    schedule toric-5 also goes through the one-call ops.bposd, whose BP outputs are the same."""
    equal = {}
    alpha, beta, iters, early_stop = cases.PARAMS[0]
    for code, B, dtype in (('toric_5', 67, 'float64'), ('ldpc_648_324', ldpc_B, 'float32')):
        H, x = cases.inputs(code, B, dtype)
        g = gd.TannerGraph(H, device=DEV)
        pred, llr, its, status = ops.minsum(g, on_dev(x), iters, alpha, beta, bool(early_stop),
                                            schedule=schedule)
        equal[code] = same((llr, its, status), cases.reference(code, B, dtype, cases.PARAMS[0]))
        if schedule == 'layered' and code == 'toric_5':
            one = ops.bposd(g, on_dev(x), iters, alpha, beta, bool(early_stop), schedule='layered')
            equal[code] = equal[code] and bool(torch.equal(one[6], llr)
                                               and torch.equal(one[4], status))
    return equal


def minsum():
    """toric-5 B = 67 (fp64) and LDPC B = 3 (fp32)."""
    import minsum_cases as mc
    return _minsum(mc, 'flooding', 3)


def minsum_layered():
    """toric-5 B = 67 (fp64) and LDPC B = 5 (fp32)."""
    import minsum_layered_cases as lc
    return _minsum(lc, 'layered', 5)


def bposd():
    """bposd and osd_gated on toric-5 B = 67 and osd_gated on the rank-deficient BCH graph against
    the host mirrors."""
    import bposd_cases as bc
    import minsum_cases as mc
    import osd_cases as oc
    equal = {}
    alpha, beta, iters, early = bc.bp_params('toric_5')
    H, x = mc.inputs('toric_5', 67, 'float64')
    g = gd.TannerGraph(H, device=DEV)
    got = ops.bposd(g, on_dev(x), iters, alpha, beta, True, 'zero', 'cs', 10)
    ref = ops.bposd_host(H, x, iters, alpha, beta, True, 'zero', 'cs', 10)
    # the OSD stage orders by pred, which is each library's own exponential: its mirror runs on
    # the pred the device returned
    n = lambda t: t.cpu().numpy().reshape(-1)
    osd_ref = ops.osd_gated_host(H, x, n(got[5]), n(got[4]), 'zero', 'cs', 10, llr=n(got[6]))
    equal['toric_5_bposd'] = same(got[3:5] + got[6:], ref[3:5] + ref[6:]) and same(got[:3], osd_ref)
    for code, B, dtype, base, gate in (
            ('toric_5', 67, 'float32', 'zero', bc.gate('toric_5', 67, 'float32', 'alt')),
            ('bch_dup', 4, 'float32', 'hard', np.array([1, 0, 1, 1], np.int32))):
        H, x, p = oc.inputs(code, B, dtype)
        g = gd.TannerGraph(H, device=DEV)
        L = bc.llr_input(code, B, dtype)
        d = lambda a: on_dev(np.ascontiguousarray(a))
        equal[f'{code}_gated'] = all(
            same(ops.osd_gated(g, d(x), d(p), d(gate), base, method, order, llr=d(L)),
                 ops.osd_gated_host(H, x, p, gate, base, method, order, llr=L))
            for method, order in (('cs', 10), ('e', 8)))
    return equal


def _relay_cases(toric_B, inputs):
    """toric-5 (fp64, six legs) and LDPC B = 3 (fp32, the short legs that run out) -> the case and
    the arguments every relay op starts with."""
    import relay_cases as rc
    for case in (('toric_5', toric_B, 'float64', rc.PARAMS[1]),
                 ('ldpc_648_324', 3, 'float32', rc.PARAMS[3])):
        code, B, dtype, params = case
        legs, iters0, iters_leg, S = params
        H, x = inputs(*case)
        g = gd.TannerGraph(H, device=DEV)
        yield case, (g, on_dev(x), on_dev(rc.gammas(g.V, params, dtype)), iters0, iters_leg, S,
                     rc.ALPHA, rc.BETA)


def relay():
    """toric-5 B = 67 and LDPC through ops.relay, every output against the numpy reference."""
    import relay_cases as rc
    equal = {}
    for case, args in _relay_cases(67, lambda code, B, dtype, params:
                                   rc.inputs('plain', code, B, dtype)):
        ref = rc.reference('plain', *case)
        equal[case[0]] = same(ops.relay(*args), [ref[k] for k in rc.OUTPUTS])
    return equal


def relay_osd():
    """toric-5 B = 9 and LDPC through ops.relay_soft and ops.relay_osd in both soft modes: soft and
    the relay outputs against the numpy statement, the one call against the two."""
    import relay_cases as rc
    import relay_osd_cases as roc
    equal = {}
    for case, args in _relay_cases(9, roc.inputs):
        ref = roc.reference(*case)
        ok = True
        for mode in roc.MODES:
            out = ops.relay_soft(*args, soft=mode)
            ok &= same(out[1:], [ref['soft_' + mode]] + [ref[k] for k in rc.OUTPUTS])
            both = ops.relay_osd(*args, soft=mode, base=roc.base_of(case[0]))
            ok &= bool(torch.equal(both[3], out[0]) and torch.equal(both[6], out[5]))
        equal[case[0]] = ok
    return equal


def bpgd():
    """toric-5 B = 67 (fp64, the working set and the most-reliable set) and syn_hub B = 9 (fp32,
    the set that decimates every variable) against the numpy reference."""
    import bpgd_cases as bc
    equal = {}
    for code, B, dtype, pset in (('toric_5', 67, 'float64', 1), ('toric_5', 67, 'float64', 2),
                                 ('syn_hub', 9, 'float32', 3)):
        H, x = bc.inputs(code, B, dtype)
        g = gd.TannerGraph(H, device=DEV)
        iters0, iters_round, rounds, per_round, pick = bc.params(g.V)[pset]
        out = ops.bpgd(g, on_dev(x), iters0, iters_round, rounds, per_round, pick, bc.CLAMP,
                       bc.ALPHA, bc.BETA)
        ref = bc.reference(code, B, dtype, pset)
        got = dict(zip(('ehat', 'llr', 'pred', 'iters', 'status', 'ndec'), out))
        equal[f'{code}/{pset}'] = same([got[k] for k in bc.OUTPUTS], [ref[k] for k in bc.OUTPUTS])
    return equal


def _unsatisfiable(H):
    """Three hand-made two_comp codewords, of which the first and the last have no solution."""
    V, C = H.shape
    x = np.ones((3, V + C))
    x[0, V + 2] = -1
    x[1, V + 1] = x[1, V + 3] = -1
    x[2, V + 0] = x[2, V + 1] = x[2, V + 4] = -1
    return x.reshape(-1)


def uf():
    """toric-5 (fp64), ring-130 (fp32) and two_comp (fp64, then the unsatisfiable codewords), all
    B = 67, against the independent statement."""
    import uf_cases as uc
    equal = {}
    for shape, dtype in (('toric_5', 'float64'), ('ring_130', 'float32'), ('two_comp', 'float64')):
        H, x = uc.inputs(shape, uc.B_ALL, dtype)
        g = gd.TannerGraph(H, device=DEV)
        equal[shape] = same(ops.uf(g, on_dev(x)), uc.reference(shape, uc.B_ALL, dtype))
    x = _unsatisfiable(H)
    r = uc.uf_ref(H, x)
    equal['two_comp/unsatisfiable'] = same(
        ops.uf(g, on_dev(x)),
        (r['ehat01'].reshape(-1).astype('float64'), r['rounds'], r['status'], r['nfull']))
    return equal


def ufw():
    """toric-5 (fp64, llr), ring-130 (fp32, priors) and two_comp (fp64, llr, then the unsatisfiable
    codewords), all B = 67, against the independent statement; the scale = 0 anchor against the
    unweighted mirror; ops.belief_find on toric-5 against its host mirror."""
    import ufw_cases as wc
    equal = {}
    for shape, dtype, with_llr in (('toric_5', 'float64', True), ('ring_130', 'float32', False),
                                   ('two_comp', 'float64', True)):
        H, x, llr = wc.inputs(shape, wc.B_ALL, dtype)
        g = gd.TannerGraph(H, device=DEV)
        out = ops.ufw(g, on_dev(x), on_dev(llr) if with_llr else None, wc.SCALE, wc.WMAX)
        equal[shape] = same(out, wc.reference(shape, wc.B_ALL, dtype, with_llr))
        anchor = ops.ufw(g, on_dev(x), on_dev(llr), 0.0, 32)
        equal[shape + '/anchor'] = same(anchor[:4], ops.uf_host(H, x))
    x, l3 = _unsatisfiable(H), llr[:3 * H.shape[0]]
    r = wc.ufw_ref(H, x, l3)
    out = ops.ufw(g, on_dev(x), on_dev(l3), wc.SCALE, wc.WMAX)
    equal['two_comp/unsatisfiable'] = same(out, wc.as_tuple(r, 'float64')) and \
        r['status'].tolist() == [1, 0, 1]
    H, x = wc.bf_inputs('float64')
    g = gd.TannerGraph(H, device=DEV)
    args = (wc.BF_ITERS, wc.BF_ALPHA, wc.BF_BETA, True, wc.SCALE, wc.WMAX)
    equal['belief_find'] = same(ops.belief_find(g, on_dev(x), *args),
                                ops.belief_find_host(H, x, *args))
    return equal


def lsd():
    """toric-5 B = 67 (fp64), syn_c65 B = 9 (fp32: a row in the second row slot) and syn_tall B = 9
    (fp64: unsolvable codewords) through ops.lsd in both bases with bits_per_step 0 and 1 against
    the independent statement; ops.lsd_gated and ops.bplsd on toric-5 against their host mirrors."""
    import bposd_cases as bc
    import lsd_cases as lc
    import osd_cases as oc
    equal = {}
    for code, B, dtype in (('toric_5', 67, 'float64'), ('syn_c65', 9, 'float32'),
                           ('syn_tall', 9, 'float64')):
        H, x, p = oc.inputs(code, B, dtype)
        g = gd.TannerGraph(H, device=DEV)
        for base in ('zero', 'hard'):
            for bits in (0, 1):
                out = ops.lsd(g, on_dev(x), on_dev(p), base, bits)
                equal[f'{code}/{base}/{bits}'] = same(
                    out, lc.as_tuple(lc.reference(code, B, dtype, base, bits), dtype))
    H, x, p = oc.inputs('toric_5', 67, 'float64')
    g = gd.TannerGraph(H, device=DEV)
    gate = bc.gate('toric_5', 67, 'float64', 'alt')
    equal['gated'] = same(ops.lsd_gated(g, on_dev(x), on_dev(p), on_dev(gate), 'zero', 1),
                          ops.lsd_gated_host(H, x, p, gate, 'zero', 1))
    H, x, args = lc.bp_inputs('float64')
    equal['bplsd'] = same(ops.bplsd(g, on_dev(x), *args, 'zero', 1),
                          ops.bplsd_host(H, x, *args, 'zero', 1))
    return equal


FAMILIES = {f.__name__: f for f in (osd, osd_hi, minsum, minsum_layered, bposd, relay, relay_osd,
                                    bpgd, uf, ufw, lsd)}

if __name__ == '__main__':
    report(equal=FAMILIES[sys.argv[1]]())
