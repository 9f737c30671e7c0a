"""Message-MLP live units on the GPU: the fp32 resident decoder (CGNNI, QGNNI; f32 and bf16
storage) puts the live hidden units of the message MLP into the first slots and, on the plans with
more than 64 item-state registers (BCH(63,45): Q = 9, R = 3), runs an iteration loop instantiated
per live count (10, 9, 8; fewer run the 8-unit loop over zero weights).  The lighter plans (the
toric codes) run all ten slots, the dead ones with zero weights.

Bit-equality: weights A have dead units (pre-activation <= 0 on the whole reachable input range,
tests/test_mlp_live_units_cpu.py).  Weights B replace each dead unit by (W1 = 0, b1 = +1, W2 = 0):
live, so all ten units run, and its contribution fma(h, 0, acc) = acc is the same function and the
same bits.  The decodes of A and B must be identical, and A matches the oracle at the tolerances of
tests/test_gpu_parity.py (native fp32: rtol 1e-4, atol 2e-5, decisions outside 1e-6 of 0.5; fp32
on the fp64 quantum models: 1e-4 absolute, decisions outside 1e-3 of 0.5; fp64: rtol 1e-10, atol
1e-12) and, for bf16 storage, the rule of tests/test_gpu_bf16.py (the fp32 result on the widened
inputs, rounded to bf16)."""
import os

import numpy as np
import pytest
import torch

import gnn_oracle as O
from conftest import weights_of
from test_gpu_parity import run_fused

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = os.path.join(ROOT, 'gnn-decode_amd', 'gnndecode', 'weights')
MSG = {'cgnni': 'ggc2.mlp2.', 'qgnni': 'ggc2.mlp.'}
UMAX = 25.0       # |u| = |(G R - 1) - 2 v| <= G R + 1: 25 on BCH(63,45) (G R = 24), 5 on toric codes


def _shipped(name):
    z = np.load(os.path.join(WEIGHTS, name + '.npz'))
    return {k: np.array(z[k]) for k in z.files}


def _kill(w, model, units):
    """Weights with the message-MLP units `units` dead beyond doubt: b1 = -(|W1| 25 + 1)."""
    w = {k: v.copy() for k, v in w.items()}
    W1, b1 = w[MSG[model] + '0.weight'], w[MSG[model] + '0.bias']
    for k in units:
        b1[k] = -(abs(W1[k, 0]) * UMAX + 1)
    return w


def _dead_units(w, model):
    """Dead units by the plain-weight statement of the rule: W1 u + b1 <= 0 at u = +-UMAX, with a
    margin far above fp32 rounding (the cases here are unambiguous by construction, and the
    shipped BCH unit has W1 ~ 1e-5, b1 = -0.75)."""
    W1 = w[MSG[model] + '0.weight'].astype(np.float64)[:, 0]
    b1 = w[MSG[model] + '0.bias'].astype(np.float64)
    return [int(k) for k in np.flatnonzero(np.abs(W1) * UMAX + b1 <= -0.5)]


def _revive(w, model):
    """Weights B: every dead unit replaced by the live unit (W1 = 0, b1 = +1, W2 = 0)."""
    w = {k: v.copy() for k, v in w.items()}
    for k in _dead_units(w, model):
        w[MSG[model] + '0.weight'][k, 0] = 0
        w[MSG[model] + '0.bias'][k] = 1
        w[MSG[model] + '2.weight'][0, k] = 0
    return w


def _model(model, H, T, w):
    import gnndecode as gd
    m = gd.MODELS[model](T, H)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in w.items()})
    return m.to(DEV).eval()


def _assert_native_f32(out, ref):
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=2e-5)
    near = np.abs(ref - 0.5) < 1e-6
    assert ((out > 0.5) == (ref > 0.5))[~near].all()


@pytest.fixture(scope='module')
def bch():
    import gnndecode as gd
    H = gd.codes.bch_63_45()
    x, _ = gd.data.awgn_batch(H, 33, seed=41, device=DEV)
    return H, x.view(33, -1)


@pytest.fixture(scope='module')
def bch_weights(golden):
    """'shipped': the trained BCH(63,45) weights (unit 0 dead).  'rand': the random-init fixture
    of the parity tests (ten live units, second-layer weights of order 0.1, so a unit that landed
    in the wrong slot would show)."""
    return {'shipped': _shipped('cgnni_bch_63_45'),
            'rand': {k: np.array(v) for k, v in weights_of(golden('cgnni_bch_randinit')).items()}}


# (base weights, units killed on top, live units expected)
BCH_CASES = [
    pytest.param('shipped', (), 9, id='shipped-1dead'),
    pytest.param('rand', (0,), 9, id='dead-first'),
    pytest.param('rand', (9,), 9, id='dead-last'),
    pytest.param('rand', (4,), 9, id='dead-middle'),
    pytest.param('rand', (2, 7), 8, id='2dead'),
    pytest.param('rand', (0, 3, 5, 9), 6, id='4dead'),
]


@pytest.mark.parametrize('store', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('base,kill,nlive', BCH_CASES)
def test_cgnni_bch_pruned_equals_ten_live_units(bch, bch_weights, base, kill, nlive, store):
    H, x33 = bch
    wa = _kill(bch_weights[base], 'cgnni', kill)
    assert 10 - len(_dead_units(wa, 'cgnni')) == nlive
    wb = _revive(wa, 'cgnni')
    assert not _dead_units(wb, 'cgnni')
    for T in (1, 3):
        ma, mb = _model('cgnni', H, T, wa), _model('cgnni', H, T, wb)
        for B in (1, 16, 33):       # one codeword, a full 16-codeword tile, three tiles (last partial)
            x = x33[:B].reshape(-1, 1).to(store)
            oa, ob = run_fused(ma, x), run_fused(mb, x)
            assert oa.dtype == store and oa.shape == (B * 63, 1)
            assert torch.equal(oa, ob), (T, B)
            xw = x.float()
            ref = O.decode('cgnni', H, xw.cpu().numpy(), T, wa)
            o32 = run_fused(ma, xw) if store == torch.bfloat16 else oa
            _assert_native_f32(o32.cpu().numpy(), ref)
            if store == torch.bfloat16:
                assert torch.equal(oa, o32.bfloat16()), (T, B)


def test_qgnni_toric5_pruned_equals_ten_live_units():
    """QGNNI (message fma(y, s_c, m)) on the toric-5 plan, two synthetic dead units; fp32 kernel
    against the fp64 oracle."""
    import gnndecode as gd
    H = gd.codes.toric_code(5)
    wa = _kill(_shipped('qgnni_toric_5'), 'qgnni', (1, 6))
    assert _dead_units(wa, 'qgnni') == [1, 6]
    wb = _revive(wa, 'qgnni')
    assert not _dead_units(wb, 'qgnni')
    T = 2
    ma, mb = _model('qgnni', H, T, wa), _model('qgnni', H, T, wb)
    x17, _ = gd.data.toric_batch(H, 17, seed=42, device=DEV, dtype=torch.float64)
    for B in (1, 17):
        x64 = x17.view(17, -1)[:B].reshape(-1, 1)
        oa, ob = run_fused(ma, x64.float()), run_fused(mb, x64.float())
        assert oa.dtype == torch.float32
        assert torch.equal(oa, ob), B
        ref = O.decode('qgnni', H, x64.cpu().numpy(), T, wa)
        out = oa.double().cpu().numpy()
        assert np.abs(out - ref).max() <= 1e-4
        far = np.abs(ref - 0.5) >= 1e-3
        assert ((out > 0.5) == (ref > 0.5))[far].all()


def test_other_paths_unchanged(bch, bch_weights):
    """The per-count loop exists only in the fp32 GNN kernels: plain BP and fp64 CGNNI on
    BCH(63,45) still match the oracle (B = 17: a partial second tile; T = 2)."""
    import gnndecode as gd
    H, x33 = bch
    x = x33[:17].reshape(-1, 1)
    out = run_fused(gd.MODELS['cbp'](2, H).to(DEV).eval(), x).cpu().numpy()
    _assert_native_f32(out, O.decode('cbp', H, x.cpu().numpy(), 2))
    w = bch_weights['shipped']
    x64 = x.double()
    out = run_fused(_model('cgnni', H, 2, w), x64).cpu().numpy()
    assert out.dtype == np.float64
    ref = O.decode('cgnni', H, x64.cpu().numpy(), 2, w)
    np.testing.assert_allclose(out, ref, rtol=1e-10, atol=1e-12)
    near = np.abs(ref - 0.5) < 1e-12
    assert ((out > 0.5) == (ref > 0.5))[~near].all()
