"""The graphs and case lists of the fused decoders' irregular-graph tests (tests/synthetic_codes.py
DECODE_*; the GPU side is tests/test_gpu_decode_synthetic.py): every graph's host tables hold the
invariants the kernels index by, the (G, R) mirror gives the table's slot plans, and the case lists
are consistent.  CPU only."""
import ctypes

import numpy as np
import pytest

from gnndecode import _lib

import synthetic_codes as sc


def _validate(H):
    v, c = (np.ascontiguousarray(a, np.int64) for a in np.nonzero(np.asarray(H)))
    rep = (ctypes.c_int32 * 4)()
    P = ctypes.POINTER(ctypes.c_int64)
    rc = _lib.get().gnnd_graph_validate_host(v.ctypes.data_as(P), c.ctypes.data_as(P), v.size,
                                             H.shape[0], H.shape[1], rep)
    return rc, list(rep)


@pytest.mark.parametrize('name', sc.DECODE_NAMES)
def test_graph_tables_consistent(name):
    H = sc.decode_matrix(name)
    assert H.dtype == np.uint8 and not H.flags.writeable and sc.decode_matrix(name) is H
    assert H.shape[0] <= 320 and int(H.sum()) <= 1000
    if name in sc.NAMES:
        assert H is sc.matrix(name)
    rc, rep = _validate(H)
    assert rc == _lib.OK and rep[3] == 0 and rep[1] >= 7, (rc, rep)


# (largest check degree, (G, R) by tie preference 0, 1, 2): build_plan by hand
SLOT_PLANS = ((1, (1, 1), (1, 1), (1, 1)), (2, (2, 1), (1, 2), (1, 2)), (4, (4, 1), (1, 4), (2, 2)),
              (6, (2, 3), (2, 3), (2, 3)), (8, (8, 1), (2, 4), (4, 2)), (20, (8, 3), (8, 3), (8, 3)),
              (40, (16, 3), (16, 3), (16, 3)), (70, (32, 3), (32, 3), (32, 3)),
              (100, (64, 2), (32, 4), (64, 2)), (256, (64, 4), (64, 4), (64, 4)))


@pytest.mark.parametrize('row', SLOT_PLANS, ids=lambda r: f'dc{r[0]}')
def test_slot_plan_mirror(row):
    assert tuple(sc.slot_plan(row[0], p) for p in (0, 1, 2)) == row[1:]


def test_slot_plan_mirror_limits():
    assert sc.slot_plan(257, 0) is None
    # R = 2 is preference 0's plan for no degree below 97: decoder_v2_4 reaches it on syn_g64 alone
    assert [d for d in range(1, 257) if sc.slot_plan(d, 0)[1] == 2] == list(range(97, 129))
    # the resident plan (preference 1) has R <= 2, which items_per_lane = 12 needs, only for
    # checks of degree <= 2
    assert [d for d in range(1, 257) if sc.slot_plan(d, 1)[1] <= 2] == [1, 2]


def test_graphs_have_the_planned_slot_forms():
    want = {'syn_wide': (1, 4, 'one'), 'syn_hub': (2, 3, 'none'), 'syn_tall': (1, 3, 'none'),
            'syn_sq64': (2, 3, 'R'), 'syn_c65': (2, 3, 'R'), 'syn_leaf': (2, 3, 'R'),
            'syn_g8': (8, 3, 'R'), 'syn_g16': (16, 3, 'R'), 'syn_g32': (32, 3, 'R'),
            'syn_g64': (32, 4, 'R'), 'syn_full8': (2, 4, 'none'), 'syn_pad1': (2, 3, 'one'),
            'syn_twin': (2, 3, 'R'), 'syn_two': (2, 3, 'R')}
    assert {n: sc.slot_form(sc.decode_matrix(n), 1) for n in sc.DECODE_NAMES} == want
    H = sc.decode_matrix('syn_leaf')
    assert H.sum(0).min() == 0 and (H.sum(0) == 1).any() and H.sum(1).min() == 0
    assert sc.components(sc.decode_matrix('syn_twin')) == 2
    assert sc.components(sc.decode_matrix('syn_two')) == 2


def test_case_lists_are_consistent():
    cases = sc.DECODE_PLAN_CASES
    assert len({c[:3] for c in cases}) == len(cases)
    for name, model, dtype, kernel, q, vg in cases:
        assert name in sc.DECODE_NAMES and dtype in ('float32', 'float64') and kernel in 'RS'
        assert (kernel == 'R') == (q > 0) == (vg > 0)
        assert dtype == 'float32' or model not in sc.CLASSICAL
    reached = set().union(*(sc.case_branches(c) for c in cases))
    assert reached >= sc.REQUIRED_BRANCHES, sorted(sc.REQUIRED_BRANCHES - reached)
    assert len({c[4] for c in cases if c[3] == 'R'}) >= 3           # items per lane: 3, 6, 9
    assert set(sc.POSITION_CASES) <= set(cases) and len(sc.POSITION_CASES) == 15
    # every new graph is decoded by some case; the earlier graphs that the resident G = 1 and the
    # long variable sums need are too
    used = {c[0] for c in cases} | set(sc.SPLIT_GRAPHS)
    assert used >= set(sc.DECODE_NAMES) - {'syn_wide', 'syn_sq64', 'syn_c65'}, used
    # decoder_v2_4 crosses each batch threshold on an R = 1, an R = 2 and an R = 3 plan
    for name, R in (('syn_full8', 1), ('syn_g64', 2), ('syn_hub', 3)):
        forms = [sc.v24_form(name, 'float32', B) for B in sc.V24_BATCHES if B <= 4096]
        assert {f[1] for f in forms} == {R}, (name, forms)
        assert [f[2] for f in forms] == ([4, 4, 2, 1] if R <= 2 else [1] * 4)


def test_inputs_are_seeded_and_shaped():
    for model in ('cgnni', 'qbp'):
        H = sc.decode_matrix('syn_leaf')
        x = sc.decode_inputs('syn_leaf', model, 5)
        assert x.shape == (5 * sum(H.shape), 1)
        assert x.dtype == (np.float32 if model == 'cgnni' else np.float64)
        assert np.array_equal(x, sc.decode_inputs('syn_leaf', model, 5))
        xc = x.reshape(5, -1)[:, H.shape[0]:]
        assert (xc == 0).all() if model == 'cgnni' else (np.abs(xc) == 1).all()
