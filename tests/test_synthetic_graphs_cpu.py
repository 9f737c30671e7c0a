"""The min-sum, layered, relay, OSD and BP+OSD host mirrors on the synthetic irregular graphs of
tests/synthetic_codes.py (a layer wider than a wave, hub variables of degree 38, isolated variables,
checks of degree 2, more checks than variables with full column rank, V = C = 64, C = 65), exact
equality with the numpy statements of the *_cases.py modules, LLRs with their sign bit; the host
graph tables and the greedy layers of every graph.  CPU only."""
import ctypes

import numpy as np
import pytest

from gnndecode import _lib, ops

import bposd_cases as bc
import minsum_cases as mc
import minsum_layered_cases as lc
import osd_cases as oc
import osd_hi_cases as ohc
import relay_cases as rc
import synthetic_codes as sc

DTYPES = ('float32', 'float64')
REFS = {'flooding': mc.reference, 'layered': lc.reference}


@pytest.mark.parametrize('code', sc.NAMES)
def test_graph_tables_and_layers(code):
    H = sc.matrix(code)
    assert H.dtype == np.uint8 and not H.flags.writeable and sc.matrix(code) is H
    assert mc.code_matrix(code) is H and oc.code_matrix(code) is H
    v, c = (np.ascontiguousarray(a, np.int64) for a in np.nonzero(H))
    rep = (ctypes.c_int32 * 4)()
    P = ctypes.POINTER(ctypes.c_int64)
    st = _lib.get().gnnd_graph_validate_host(v.ctypes.data_as(P), c.ctypes.data_as(P), v.size,
                                             H.shape[0], H.shape[1], rep)
    assert st == _lib.OK and rep[3] == 0 and rep[1] >= 7, (st, list(rep))
    lay = ops.layers_host(H)
    assert lay.dtype == np.int32
    assert np.array_equal(lay, lc.layer_of_check(code))
    assert np.array_equal(lay, sc.greedy_layers(H))


@pytest.mark.parametrize('schedule', ['flooding', 'layered'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('code,B', sc.MINSUM_SHAPES)
def test_minsum_host_equals_reference(code, B, dtype, schedule):
    params = alpha, beta, iters, early = mc.PARAMS[0]
    H, x = mc.inputs(code, B, dtype)
    ref_llr, ref_it, ref_st = REFS[schedule](code, B, dtype, params)
    pred, llr, its, status = ops.minsum_host(H, x, iters, alpha, beta, bool(early),
                                             schedule=schedule)
    assert llr.dtype == np.dtype(dtype) and its.dtype == np.int32 and status.dtype == np.int32
    assert np.array_equal(its, ref_it) and np.array_equal(status, ref_st)
    assert np.array_equal(llr, ref_llr)
    assert np.array_equal(np.signbit(llr), np.signbit(ref_llr))
    np.testing.assert_allclose(pred, mc.soft_output(ref_llr), **mc.pred_tolerance(dtype))
    assert np.array_equal(status == 0, mc.satisfied(H, x, llr))
    # a variable of degree 0 keeps its prior: L = l
    V, C = H.shape
    iso = np.nonzero(H.sum(1) == 0)[0]
    assert np.array_equal(llr.reshape(B, V)[:, iso], x.reshape(B, V + C)[:, iso])


def test_isolated_variables_are_covered():
    assert (sc.matrix('syn_wide').sum(1) == 0).sum() == 3
    assert (sc.matrix('syn_sq64').sum(1) == 0).any()


@pytest.mark.parametrize('pi', sc.RELAY_PARAMS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('family,code,B', sc.RELAY_CASES)
def test_relay_host_equals_reference(family, code, B, dtype, pi):
    params = legs, iters0, iters_leg, S = rc.PARAMS[pi]
    H, x = rc.inputs(family, code, B, dtype)
    ref = rc.reference(family, code, B, dtype, params)
    got = ops.relay_host(H, x, rc.gammas(H.shape[0], params, dtype), iters0, iters_leg, S,
                         rc.ALPHA, rc.BETA)
    rc.assert_equal(got, ref, 'host mirror against the numpy statement')
    assert np.array_equal(got[3] == 0, rc.satisfied(H, x, got[1]))


@pytest.mark.parametrize('dtype', DTYPES)
def test_relay_batches_pick_several_legs(dtype):
    """Across the synthetic relay cases: the six-leg set chooses leg 0 and at least two later
    legs, and the short legs of PARAMS[3] stop at one and at two solutions."""
    chosen, nsol = set(), set()
    for family, code, B in sc.RELAY_CASES:
        ref = rc.reference(family, code, B, dtype, rc.PARAMS[1])
        chosen |= set(ref['leg'][ref['status'] == 0].tolist())
        ref = rc.reference(family, code, B, dtype, rc.PARAMS[3])
        nsol |= set(ref['nsol'].tolist())
        if code == 'syn_tall':
            assert len(set(ref['leg'].tolist())) >= 2, ref['leg'].tolist()
    assert 0 in chosen and len(chosen - {0}) >= 2, sorted(chosen)
    assert {1, 2} <= nsol, sorted(nsol)


@pytest.mark.parametrize('base', ['zero', 'hard'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('code,B', sc.OSD_SHAPES)
def test_osd_host_equals_reference(code, B, dtype, base):
    H, x, p = oc.inputs(code, B, dtype)
    V = H.shape[0]
    ref_e, ref_s = oc.reference(code, B, dtype, base)
    ehat, status = ops.osd0_host(H, x, p, base)
    assert ehat.dtype == p.dtype and status.dtype == np.int32
    assert np.array_equal(status, ref_s) and np.array_equal(ehat.reshape(B, V), ref_e)
    assert oc.satisfied(H, x, ehat)[status == 0].all()
    if code == 'syn_tall':
        # the odd codewords carry a flipped target: unused rows decide, and some must fail
        assert not status[0::2].any() and status[1::2].any(), status.tolist()
    else:
        assert not status.any()
    for method, order in sc.OSD_METHODS:
        tag = (method, order)
        r_e, r_s, r_c = ohc.reference(code, B, dtype, base, method, order)
        h_e, h_s, h_c = ops.osd_host(H, x, p, base, method, order)
        assert np.array_equal(h_s, r_s) and np.array_equal(h_c, r_c), tag
        assert np.array_equal(h_e.reshape(B, V), r_e), tag
        assert np.array_equal(h_s, status), tag
        if method == 'osd0':
            assert np.array_equal(h_e, ehat) and not h_c.any()
        if code == 'syn_tall':
            # full column rank: no free column, every method is OSD-0 with candidate 0
            assert ohc.free_count(code, B, dtype, base) == [0] * B
            assert np.array_equal(h_e, ehat) and not h_c.any(), tag
    if code != 'syn_tall':
        assert min(ohc.free_count(code, B, dtype, base)) > 0


@pytest.mark.parametrize('schedule', ['flooding', 'layered'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('code,B', sc.BPOSD_SHAPES)
def test_bposd_host_equals_reference(code, B, dtype, schedule):
    alpha, beta, iters, early = bc.bp_params(code)
    H, x = mc.inputs(code, B, dtype)
    V = H.shape[0]
    ehat, status, choice, its, bp, pred, llr = ops.bposd_host(
        H, x, iters, alpha, beta, bool(early), 'zero', 'cs', 10, schedule=schedule)
    r_e, r_s, r_c, r_it, r_bp, r_llr = bc.bposd_reference(code, B, dtype, pred, 'zero', 'cs', 10,
                                                          schedule=schedule)
    assert np.array_equal(llr, r_llr) and np.array_equal(np.signbit(llr), np.signbit(r_llr))
    assert np.array_equal(its, r_it) and np.array_equal(bp, r_bp)
    np.testing.assert_allclose(pred, mc.soft_output(r_llr), **mc.pred_tolerance(dtype))
    assert np.array_equal(ehat.reshape(B, V), r_e.astype(ehat.dtype))
    assert np.array_equal(status, r_s) and np.array_equal(choice, r_c)
    ok = bp == 0
    assert np.array_equal(ehat.reshape(B, V)[ok], (llr.reshape(B, V)[ok] < 0).astype(ehat.dtype))
    assert (choice[ok] == -1).all() and oc.satisfied(H, x, ehat)[status == 0].all()
    if code in mc.SYN_EASY:
        assert ok.all()                                     # min-sum solves all: nothing is gated
    else:
        assert ok.any() and (~ok).any() and not status.any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_gated_osd_host_on_the_tall_graph(dtype):
    """osd_gated on syn_tall with the alternating gate selects exactly the codewords with a
    flipped target: the gated path on unused rows, failures included, with no free column."""
    code, B = 'syn_tall', 9
    H, x, p = oc.inputs(code, B, dtype)
    gate = bc.gate(code, B, dtype, 'alt')
    for method, order in (('cs', 10), ('e', 8)):
        got = ops.osd_gated_host(H, x, p, gate, 'hard', method, order)
        ref = bc.gated_reference(code, B, dtype, 'hard', method, order, 'alt', False)
        assert np.array_equal(got[0].reshape(B, -1), ref[0].astype(got[0].dtype))
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        assert got[1][1::2].any() and not got[1][0::2].any()
