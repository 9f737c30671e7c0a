"""The min-sum, layered, relay, OSD and BP+OSD kernels on the synthetic irregular graphs of
tests/synthetic_codes.py, which reach the launch plan branches and loop shapes the shipped codes
never do: a layer of 80 checks on 64 lanes (the layered kernel's layer loop runs twice per lane),
the LDS-driven doubling of the lanes per codeword (8 in fp32, 16 in fp64 on one graph), sums over
38 edges in edge order, variables of degree 0 and checks of degree 2, an elimination that ends on
the last column with unused rows left and no free column, V = 64 / C = 64 / C = 65 in OSD, and
V < 64 with C > 64.  First the plan query proves the branch is reached; then every output is
compared with the numpy statement (tests/*_cases.py) and with the host mirror, bit for bit (pred to
minsum_cases.pred_tolerance); then the same cases run under the bounds-checked debug library."""
import numpy as np
import pytest
import torch

from gnndecode import ops

import bposd_cases as bc
import debug_child
import minsum_cases as mc
import minsum_layered_cases as lc
import osd_cases as oc
import osd_hi_cases as ohc
import relay_cases as rc
import synthetic_codes as sc
import synthetic_debug_worker as work

pytestmark = pytest.mark.gpu

REFS = {'flooding': mc.reference, 'layered': lc.reference}


def _bits(got, ref, tag):
    """Equal arrays; floating ones with their sign bit."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (tag, got.dtype, ref.dtype)
    assert np.array_equal(got, ref), (tag, np.nonzero(got != ref)[0][:8].tolist())
    if got.dtype.kind == 'f':
        assert np.array_equal(np.signbit(got), np.signbit(ref)), (tag, 'sign bit')


def check_minsum(out, code, B, dtype, schedule):
    alpha, beta, iters, early = params = mc.PARAMS[0]
    pred, llr, its, status = out
    H, x = mc.inputs(code, B, dtype)
    ref_llr, ref_it, ref_st = REFS[schedule](code, B, dtype, params)
    _bits(its, ref_it, 'iters_used')
    _bits(status, ref_st, 'status')
    _bits(llr, ref_llr, 'llr')
    tol = mc.pred_tolerance(dtype)
    np.testing.assert_allclose(pred, mc.soft_output(ref_llr), **tol)
    assert np.array_equal(status == 0, mc.satisfied(H, x, llr))
    h_pred, h_llr, h_it, h_st = ops.minsum_host(H, x, iters, alpha, beta, bool(early),
                                                schedule=schedule)
    _bits(llr, h_llr, 'llr, host')
    _bits(its, h_it, 'iters_used, host')
    _bits(status, h_st, 'status, host')
    np.testing.assert_allclose(pred, h_pred, **tol)


def check_relay(out, family, code, B, dtype, pi):
    params = legs, iters0, iters_leg, S = rc.PARAMS[pi]
    H, x = rc.inputs(family, code, B, dtype)
    rc.assert_equal(out, rc.reference(family, code, B, dtype, params), 'numpy statement')
    assert np.array_equal(out[3] == 0, rc.satisfied(H, x, out[1]))
    mirror = ops.relay_host(H, x, rc.gammas(H.shape[0], params, dtype), iters0, iters_leg, S,
                            rc.ALPHA, rc.BETA)
    rc.assert_equal(out, mirror, 'host mirror')


def check_osd(out, code, B, dtype, base):
    H, x, p = oc.inputs(code, B, dtype)
    e0, s0 = out[:2]
    ref_e, ref_s = oc.reference(code, B, dtype, base)
    _bits(s0, ref_s, 'osd0 status')
    _bits(e0, ref_e.reshape(-1).astype(dtype), 'osd0 ehat')
    h_e, h_s = ops.osd0_host(H, x, p, base)
    _bits(s0, h_s, 'osd0 status, host')
    _bits(e0, h_e, 'osd0 ehat, host')
    if code == 'syn_tall':
        # the flipped targets of the odd codewords: unused rows decide, and some must fail
        assert not s0[0::2].any() and s0[1::2].any(), s0.tolist()
    else:
        assert not s0.any()
    for i, (method, order) in enumerate(sc.OSD_METHODS):
        ehat, status, choice = out[2 + 3 * i:5 + 3 * i]
        tag = (method, order)
        r_e, r_s, r_c = ohc.reference(code, B, dtype, base, method, order)
        _bits(status, r_s, tag)
        _bits(choice, r_c, tag)
        _bits(ehat, r_e.reshape(-1).astype(dtype), tag)
        assert oc.satisfied(H, x, ehat)[status == 0].all(), tag
        for a, b in zip((ehat, status, choice), ops.osd_host(H, x, p, base, method, order)):
            _bits(a, b, (tag, 'host'))
        if method == 'osd0' or code == 'syn_tall':           # syn_tall: no free column
            _bits(ehat, e0, tag)
            _bits(status, s0, tag)
            assert not choice.any(), tag


def check_bposd(out, code, B, dtype, schedule):
    alpha, beta, iters, early = bc.bp_params(code)
    ehat, status, choice, its, bp, pred, llr = out
    H, x = mc.inputs(code, B, dtype)
    r_e, r_s, r_c, r_it, r_bp, r_llr = bc.bposd_reference(code, B, dtype, pred, 'zero', 'cs', 10,
                                                          schedule=schedule)
    _bits(llr, r_llr, 'llr')
    _bits(its, r_it, 'iters_used')
    _bits(bp, r_bp, 'bp_status')
    np.testing.assert_allclose(pred, mc.soft_output(r_llr), **mc.pred_tolerance(dtype))
    _bits(ehat, r_e.reshape(-1).astype(dtype), 'ehat')
    _bits(status, r_s, 'status')
    _bits(choice, r_c, 'choice')
    # the host mirror: the BP stage outright, the OSD stage on the soft output the device
    # returned (it orders its columns by pred, whose exponential is each library's own)
    host = ops.bposd_host(H, x, iters, alpha, beta, bool(early), 'zero', 'cs', 10,
                          schedule=schedule)
    _bits(its, host[3], 'iters_used, host')
    _bits(bp, host[4], 'bp_status, host')
    _bits(llr, host[6], 'llr, host')
    np.testing.assert_allclose(pred, host[5], **mc.pred_tolerance(dtype))
    for a, b in zip((ehat, status, choice),
                    ops.osd_gated_host(H, x, pred, bp, 'zero', 'cs', 10, llr=llr)):
        _bits(a, b, 'OSD stage, host')
    ok = bp == 0
    assert oc.satisfied(H, x, ehat)[status == 0].all() and (choice[ok] == -1).all()
    if code in mc.SYN_EASY:
        assert ok.all()
    else:
        assert ok.any() and (~ok).any() and not status.any()


def check_gated(out, code, B, dtype):
    H, x, p = oc.inputs(code, B, dtype)
    gate = bc.gate(code, B, dtype, 'alt')
    for i, (method, order) in enumerate((('cs', 10), ('e', 8))):
        ehat, status, choice = out[3 * i:3 * i + 3]
        r_e, r_s, r_c = bc.gated_reference(code, B, dtype, 'hard', method, order, 'alt', False)
        _bits(ehat, r_e.reshape(-1).astype(dtype), method)
        _bits(status, r_s, method)
        _bits(choice, r_c, method)
        for a, b in zip((ehat, status, choice),
                        ops.osd_gated_host(H, x, p, gate, 'hard', method, order)):
            _bits(a, b, (method, 'host'))
        assert status[1::2].any() and not status[0::2].any()


CHECK = {'minsum': check_minsum, 'relay': check_relay, 'osd': check_osd, 'bposd': check_bposd,
         'gated': check_gated}


def test_plans_reach_the_intended_branches():
    """syn_wide: a layer wider than the wave on 64 lanes.  syn_hub: the layers need 8 lanes, and
    the codeword tiles of a wave push fp64 to 16.  Prints every graph's plan."""
    plans = {}
    for code in sc.NAMES:
        g = work.graph_of(code)
        lay = g.layers()
        assert np.array_equal(lay, lc.layer_of_check(code))
        for dt in (torch.float32, torch.float64):
            plans[code, dt] = p = ops.minsum_layered_plan(g, dt)
            print(code, dt, p)
            assert p['layers'] == int(lay.max()) + 1
            assert p['largest_layer'] == int(np.bincount(lay).max())
    for dt in (torch.float32, torch.float64):
        assert plans['syn_wide', dt]['largest_layer'] > 64
        assert plans['syn_wide', dt]['lanes_per_codeword'] == 64
        assert plans['syn_hub', dt]['largest_layer'] == 4
    assert plans['syn_hub', torch.float32]['lanes_per_codeword'] == 8
    assert plans['syn_hub', torch.float64]['lanes_per_codeword'] == 16


@pytest.mark.parametrize('case', work.CASES, ids=lambda c: '-'.join(str(a) for a in c))
def test_device_equals_reference_and_host_mirror(case):
    CHECK[case[0]](work.run(case), *case[1:])


def test_debug_library_runs_every_case_clean(tmp_path):
    """Every case above under the bounds-checked build (GNND_LIB, a fresh child process): no index
    check fires in any translation unit, and the bits are the references' and the mirrors'."""
    npz = str(tmp_path / 'outputs.npz')
    res = debug_child.run('synthetic_debug_worker.py', npz)
    assert res['cases'] == len(work.CASES)
    with np.load(npz) as z:
        for case in work.CASES:
            out = []
            while work.key(case, len(out)) in z.files:
                out.append(z[work.key(case, len(out))])
            CHECK[case[0]](tuple(out), *case[1:])
