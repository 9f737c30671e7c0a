"""The fused decoders (gnnd_decode) on the irregular graphs of tests/synthetic_codes.py, held to the
oracle (oracle/gnn_oracle.py, itself pinned to the reference on four of these graphs by
tests/test_oracle_golden.py) in every launch plan the shipped codes never reach: resident groups
of 1, 2, 8 and 16 lanes per check, the three padding templates, 3, 6 and 9 items per lane, padded
variable layouts for groups of 4, 8 and 16 variables, the streaming kernel by both of its routes
(a group above 16 lanes; a check of degree < 2 under the ratio-form BP step), decoder_v2_4 on
R = 1, 2 and 3 slot plans across its batch thresholds, and the component split off the toric code.

items_per_lane = 12 is not among the cases: launch_decode instantiates it for R <= 2 only, and the
resident plan (tie preference 1) has R <= 2 only where every check has degree <= 2
(test_decode_synthetic_cpu.py, test_slot_plan_mirror_limits); 3, 6 and 9 are three distinct values.
decoder_v2_4 in fp64 has no R = 2 case: preference 0 takes R = 2 only for a check of degree 97 ..
128, where the check-MLP table make_plan reserves, 16 (d - 1) + 1 entries of 96 bytes >= 147 552
bytes, with the 33 KB Softplus table exceeds the 160 KB of LDS: the plan is refused (asserted
below).  decoder_v2_2 is not run: gd.MODELS['v22'] raises on a non-toric H without edge types.

Tolerances are those of tests/test_gpu_parity.py.  No case needed the fp32 conditioning criterion
(CONDITIONED is empty)."""
import numpy as np
import pytest
import torch

import gnn_oracle as O
from gnndecode import _lib, ops

import debug_child
import decode_synthetic_debug_worker as work
import synthetic_codes as sc

pytestmark = pytest.mark.gpu

KERNEL = {'R': 'decode_resident_kernel', 'S': 'decode_kernel'}
# fp32 cases judged by the criterion of test_classical_bp_fp32_conditioning_at_scale instead of the
# fixed tolerance: (graph, model, dtype) -> the measured ratio of the GPU's error against the fp64
# oracle to the fp32 oracle's own.  None needed it.
CONDITIONED = {}


def _id(case):
    return '-'.join(str(a) for a in case[:3])


def _oracle(name, model, x, T, w, dtype=None):
    """[B, V] (decoder_v3_0: [2 B, N]) of the oracle in x's dtype, or in `dtype`."""
    H = sc.decode_matrix(name)
    if dtype is not None:
        x = x.astype(dtype)
        w = {k: (v.astype(dtype) if v.dtype.kind == 'f' else v) for k, v in w.items()}
    out = O.decode(model, H, x, T, w)
    if model == 'v30':
        return np.concatenate([o.reshape(-1, sum(H.shape)) for o in out])
    return out.reshape(-1, H.shape[0])


def _rows(name, model, t):
    H = sc.decode_matrix(name)
    return t.cpu().numpy().reshape(-1, sum(H.shape) if model == 'v30' else H.shape[0])


def _sel(model, pick, B):
    """Rows of the output that belong to the codewords `pick` (decoder_v3_0: two tensors)."""
    pick = np.asarray(pick)
    return np.concatenate([pick, pick + B]) if model == 'v30' else pick


def assert_parity(case, got, x, T, w, tag):
    """got [rows, width] of the device against the oracle on the same inputs."""
    name, model, dtype = case[:3]
    native = 'float32' if model in sc.CLASSICAL else 'float64'
    ref = _oracle(name, model, x, T, w)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f'{_id(case)} {tag}: max abs err {err:.3e}')
    if dtype == 'float64':
        np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12, err_msg=tag)
        near = np.abs(ref - 0.5) < 1e-12
    elif case[:3] in CONDITIONED:
        o64 = _oracle(name, model, x, T, w, np.float64)
        o32 = _oracle(name, model, x, T, w, np.float32).astype(np.float64)
        own = float(np.abs(o32 - o64).max())
        mine = float(np.abs(got.astype(np.float64) - o64).max())
        print(f'{_id(case)} {tag}: conditioning ratio {mine / max(own, 1e-300):.3f}')
        assert mine <= 2 * own + 2e-5, (tag, mine, own)
        near = np.abs(o64 - 0.5) < 2 * own + 2e-5
        ref = o64
    elif native == 'float32':
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-5, err_msg=tag)
        near = np.abs(ref - 0.5) < 1e-6
    else:                                   # the fp32 kernel on an fp64 model
        assert err <= 1e-4, (tag, err)
        near = np.abs(ref - 0.5) < 1e-3
    assert ((got > 0.5) == (ref > 0.5))[~near].all(), tag


# ------------------------------------------------------------------------------------------------
# f. the bounds-checked build first: it records an index out of range where the release build
# would read through it
# ------------------------------------------------------------------------------------------------
def test_debug_library_runs_every_case_clean(tmp_path):
    npz = str(tmp_path / 'outputs.npz')
    res = debug_child.run('decode_synthetic_debug_worker.py', npz, timeout=600)
    assert res['cases'] == len(sc.DECODE_PLAN_CASES)
    for case in sc.DECODE_PLAN_CASES:
        assert res['plans'][_id(case)] == [KERNEL[case[3]], case[4], case[5]], _id(case)
    with np.load(npz) as z:
        for case in sc.DECODE_PLAN_CASES:
            for T in sc.DECODE_ITERS:
                rel = work.run_case(case, T)
                dbg = z[work.key(case, T)]
                assert rel.dtype == dbg.dtype and np.array_equal(rel, dbg), (work.key(case, T))


# ------------------------------------------------------------------------------------------------
# a. the plan is reached
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sc.DECODE_PLAN_CASES, ids=_id)
def test_plan_is_reached(case):
    name, model, dtype, kernel, q, vg = case
    p = work.plan(name, model, dtype)
    print(_id(case), p)
    assert (p['kernel'], p['items_per_lane'], p['var_group']) == (KERNEL[kernel], q, vg), p
    if kernel == 'R':
        G = sc.slot_form(sc.decode_matrix(name), 1)[0]
        assert p['cw'] * sc.decode_matrix(name).shape[1] * G <= q * 256


def test_plans_cover_every_branch():
    cases = sc.DECODE_PLAN_CASES
    reached = set().union(*(sc.case_branches(c) for c in cases))
    assert reached >= sc.REQUIRED_BRANCHES, sorted(sc.REQUIRED_BRANCHES - reached)
    assert len({work.plan(*c[:3])['items_per_lane'] for c in cases if c[3] == 'R'}) >= 3
    # fp64 decoder_v2_4 has no R = 2 plan (module docstring): refused, not run
    with pytest.raises(_lib.GnndError) as e:
        work.plan('syn_g64', 'v24', 'float64')
    assert e.value.status == _lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------
# b. parity with the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in sc.DECODE_PLAN_CASES if c[1] != 'v24'], ids=_id)
def test_light_model_matches_oracle(case):
    """B in {1, cw + 1, 3 cw + 1} (a ragged last tile), T in {0, 1, 4}, seeded random weights."""
    name, model, dtype = case[:3]
    cw = ops.decode_tile(work.graph_of(name), model, work.DTYPES[dtype])[0]
    assert 3 * cw + 1 <= 193
    for T in sc.DECODE_ITERS:
        m, w = work.model_of(name, model, T)
        for B in (1, cw + 1, 3 * cw + 1):
            x = sc.decode_inputs(name, model, B)
            got = _rows(name, model, work.decode(name, m, x, dtype))
            assert_parity(case, got, x, T, w, f'B={B} T={T}')


def test_cgnni_shipped_checkpoint_matches_oracle():
    case = next(c for c in sc.DECODE_PLAN_CASES if c[:3] == ('syn_g16', 'cgnni', 'float32'))
    m, w = work.model_of('syn_g16', 'cgnni', 4, weights='shipped')
    x = sc.decode_inputs('syn_g16', 'cgnni', 28)
    assert_parity(case, _rows('syn_g16', 'cgnni', work.decode('syn_g16', m, x, 'float32')), x, 4, w,
                  'shipped B=28 T=4')


def _sample(B, n=64):
    rng = np.random.default_rng(B)
    return np.sort(np.concatenate([[0, B - 1], rng.choice(np.arange(1, B - 1), n - 2, False)]))


def _v24_batches(case, weights, iters):
    name, model, dtype = case[:3]
    N = sum(sc.decode_matrix(name).shape)
    xall = sc.decode_inputs(name, model, max(sc.V24_BATCHES)).reshape(-1, N)
    for T in iters:
        m, w = work.model_of(name, model, T, weights)
        first = None
        for B in sc.V24_BATCHES:
            got = _rows(name, model, work.decode(name, m, xall[:B].reshape(-1, 1), dtype))
            pick = np.arange(B) if B < 300 else _sample(B)
            assert_parity(case, got[pick], xall[pick].reshape(-1, 1), T, w, f'{weights} B={B} T={T}')
            if B == 67:
                first = got
            elif B > 67 and sc.v24_form(name, dtype, B) == sc.v24_form(name, dtype, 67):
                assert np.array_equal(got[:67], first), (B, T)


@pytest.mark.parametrize('case', [c for c in sc.DECODE_PLAN_CASES if c[1] == 'v24'], ids=_id)
def test_v24_matches_oracle_across_batch_thresholds(case):
    """B in {1, 67, 300, 600, 4 097}: every batch is a prefix of one input set.  From B = 300 up a
    seeded sample of 64 codewords is held to the oracle; the first 67 codewords are bit-equal to
    the B = 67 run wherever the kernel form (slot plan and unit split, sc.v24_form) is the same."""
    _v24_batches(case, 'random', sc.DECODE_ITERS)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_v24_shipped_checkpoint_matches_oracle(dtype):
    case = next(c for c in sc.DECODE_PLAN_CASES if c[:3] == ('syn_full8', 'v24', dtype))
    _v24_batches(case, 'shipped', (4,))


# ------------------------------------------------------------------------------------------------
# c. position independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sc.POSITION_CASES, ids=_id)
def test_codeword_decodes_alone_as_in_the_batch(case):
    name, model, dtype = case[:3]
    cw = ops.decode_tile(work.graph_of(name), model, work.DTYPES[dtype])[0]
    B = 3 * cw + 1
    N = sum(sc.decode_matrix(name).shape)
    m, _ = work.model_of(name, model, 4)
    x = sc.decode_inputs(name, model, B)
    full = work.decode(name, m, x, dtype)
    assert torch.equal(full, work.decode(name, m, x, dtype))
    full = _rows(name, model, full)
    for b in sorted({0, cw - 1, cw, B - 1}):
        one = _rows(name, model, work.decode(name, m, x.reshape(B, N)[b:b + 1].reshape(-1, 1), dtype))
        assert np.array_equal(one, full[_sel(model, [b], B)]), b


# ------------------------------------------------------------------------------------------------
# d. component split
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('B', sc.SPLIT_BATCHES)
@pytest.mark.parametrize('name', sc.SPLIT_GRAPHS)
def test_split_decode_matches_oracle_and_whole_graph(name, B, dtype):
    g = work.graph_of(name)
    ncomp = g.components
    print(name, 'components', ncomp)
    assert ncomp in (1, 2) and (name != 'syn_twin' or ncomp == 2)
    case = (name, 'v24', dtype)
    m, w = work.model_of(name, 'v24', 4)
    x = sc.decode_inputs(name, 'v24', B)
    try:
        g.set_split(True)
        a = work.decode(name, m, x, dtype)
        g.set_split(False)
        b = work.decode(name, m, x, dtype)
    finally:
        g.set_split(True)
    assert_parity(case, _rows(name, 'v24', a), x, 4, w, f'split B={B}')
    assert_parity(case, _rows(name, 'v24', b), x, 4, w, f'whole B={B}')
    if ncomp > 1:
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
# e. refusals
# ------------------------------------------------------------------------------------------------
def test_bf16_on_a_streaming_plan_is_refused_and_writes_nothing():
    name = 'syn_g32'
    g = work.graph_of(name)
    assert work.plan(name, 'cgnni', 'bfloat16')['kernel'] == 'decode_kernel'
    m, _ = work.model_of(name, 'cgnni', 4)
    x = torch.from_numpy(sc.decode_inputs(name, 'cgnni', 5)).to(work.DEV).to(torch.bfloat16)
    out = torch.full((5 * g.V, 1), -7.0, dtype=torch.bfloat16, device=work.DEV)
    with pytest.raises(_lib.GnndError) as e:
        ops.decode(g, 'cgnni', x, 4, m.prepared_weights(torch.float32, torch.device(work.DEV)), out=out)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == -7.0).all()


def test_check_of_degree_257_is_refused():
    import gnndecode as gd
    H = np.zeros((300, 3), np.uint8)
    H[:257, 0] = 1
    H[5:9, 1] = H[100:103, 2] = 1
    with pytest.raises(_lib.GnndError) as e:
        gd.TannerGraph(H, device=work.DEV)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    H[256, 0] = 0                                            # degree 256 is the limit
    assert gd.TannerGraph(H, device=work.DEV).max_chk_degree == 256
