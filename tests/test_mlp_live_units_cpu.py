"""Live units of the CGNNI / QGNNI message MLP (Mlp10Pair::load in gnnd_decode_impl.h), restated
in numpy.

The resident fp32 kernel evaluates the message MLP f(v) = b2 + sum_k W2_k relu(W1_k u + b1_k) of
u = (G R - 1) - 2 v with the affine map folded into the first layer in fp32:
    W1'_k = W1_k * (-2),  b1'_k = fma(W1_k, G R - 1, b1_k),
and v = R_c - r_e lies in [0, G R] (every r in [0, 1], G R slots per check).  A unit is dead when
its pre-activation is <= 0 at both ends of that interval, b1'_k <= 0 and fma(G R, W1'_k, b1'_k)
<= 0: the fp32 fma is monotone in v, so the clamped first layer is +0 on the whole interval and
the unit's layer-2 fma(+0, W2', acc) returns acc.  The kernel evaluates only the live units, in
their original order."""
import os
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = os.path.join(ROOT, 'gnn-decode_amd', 'gnndecode', 'weights')
F32 = np.float32
LOG2E = F32(1.4426950408889634)


def fma32(a, b, c):
    """fp32 fused multiply-add of scalars, rounded once: the exact rational result, then the
    nearest of the fp64-rounded value's fp32 neighbourhood by exact comparison (ties to even)."""
    r = Fraction(float(F32(a))) * Fraction(float(F32(b))) + Fraction(float(F32(c)))
    best = F32(r.numerator / r.denominator)
    for y in (np.nextafter(best, F32(-np.inf)), np.nextafter(best, F32(np.inf))):
        dy, db = abs(Fraction(float(y)) - r), abs(Fraction(float(best)) - r)
        if dy < db or (dy == db and (int(y.view(np.uint32)) & 1) == 0):
            best = y
    return best


def vfma32(a, b, c):
    """fp32 fma of arrays through fp64 (the product of two fp32 values is exact in fp64).  Monotone
    in every argument, which is all the bit-equality property below needs."""
    return (a.astype(np.float64) * np.float64(b) + np.asarray(c, np.float64)).astype(F32)


def resident_slots(H):
    """G R of the resident kernel's check-group plan (gnnd_graph.hip build_plan, larger R on
    ties): R slots per lane, G = 2^k lanes per check, fewest slots."""
    max_dc = int((np.asarray(H) != 0).sum(axis=0).max())      # H: variables x checks
    best = None
    for R in range(1, 5):
        need, G = -(-max_dc // R), 1
        while G < need:
            G <<= 1
        if G <= 64 and (best is None or G * R <= best):
            best = G * R
    return best, max_dc


def fold(W1, b1, W2, b2, GR):
    """The folded, power-of-two scaled weights and the live mask, as Mlp10Pair::load."""
    vmax, in_scale, in_bias = F32(GR), F32(-2), F32(GR - 1)
    w1s, b1s, w2s, live = [], [], [], []
    for k in range(10):
        w1 = F32(W1[k]) * in_scale
        bb = fma32(W1[k], in_bias, b1[k])
        _, e = np.frexp(F32(abs(w1) * vmax + abs(bb)))
        w1s.append(np.ldexp(w1, -int(e)))
        b1s.append(np.ldexp(bb, -int(e)))
        w2s.append(np.ldexp(F32(W2[k]) * LOG2E, int(e)))
        live.append(not (bb <= 0 and fma32(vmax, w1, bb) <= 0))
    return (np.array(w1s, F32), np.array(b1s, F32), np.array(w2s, F32), F32(b2) * LOG2E,
            np.array(live))


def mlp_eval(v, w1s, b1s, w2s, b2s, units):
    """The kernel's operation order: acc = b2', then the units in order, each one clamped fma
    (layer 1 + ReLU, v_pk_fma_f32 clamp: [0, 1]) and one fma (layer 2)."""
    acc = np.full(v.shape, b2s, F32)
    for k in units:
        h = np.clip(vfma32(v, w1s[k], b1s[k]), F32(0), F32(1))
        acc = vfma32(h, w2s[k], acc)
    return acc


def message_mlp(name):
    z = np.load(os.path.join(WEIGHTS, name))
    pre = 'ggc2.mlp2' if 'ggc2.mlp2.0.weight' in z.files else 'ggc2.mlp'
    return (z[f'{pre}.0.weight'].astype(F32).ravel(), z[f'{pre}.0.bias'].astype(F32).ravel(),
            z[f'{pre}.2.weight'].astype(F32).ravel(), z[f'{pre}.2.bias'].astype(F32).ravel()[0])


def code_of(name):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'gnn-decode_amd'))
    from gnndecode import codes
    return {'cgnni_bch_63_45.npz': codes.bch_63_45, 'cgnni_ldpc_648_324.npz': codes.wifi_ldpc_648,
            'qgnni_toric_5.npz': lambda: codes.toric_code(5)}[name]()


SHIPPED = [('cgnni_bch_63_45.npz', 9), ('cgnni_ldpc_648_324.npz', 10), ('qgnni_toric_5.npz', 10)]


def test_fma32_rounds_once():
    # a product whose low bits a separate multiply would lose
    a, b = F32(1 + 2.0 ** -12), F32(1 - 2.0 ** -12)
    assert fma32(a, b, F32(-1)) == F32(-2.0 ** -24)
    assert fma32(F32(3), F32(5), F32(-15)) == 0


@pytest.mark.parametrize('name,nlive', SHIPPED)
def test_shipped_live_counts(name, nlive):
    H = np.asarray(code_of(name))
    GR, max_dc = resident_slots(H)
    assert GR >= max_dc
    live = fold(*message_mlp(name), GR)[4]
    assert int(live.sum()) == nlive


@pytest.mark.parametrize('name,nlive', SHIPPED)
def test_pruned_mlp_is_bit_identical_on_the_reachable_interval(name, nlive):
    GR, _ = resident_slots(np.asarray(code_of(name)))
    w1s, b1s, w2s, b2s, live = fold(*message_mlp(name), GR)
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.uniform(0, GR, 9998), [0.0, float(GR)]]).astype(F32)
    full = mlp_eval(v, w1s, b1s, w2s, b2s, range(10))
    pruned = mlp_eval(v, w1s, b1s, w2s, b2s, np.flatnonzero(live))
    assert np.array_equal(full.view(np.uint32), pruned.view(np.uint32))


@pytest.mark.parametrize('dead', [(0,), (9,), (4,), (2, 7), (0, 3, 5, 9)])
def test_synthetic_dead_units(dead):
    """Units with b1 <= -(|W1| 25 + 1) are dead on BCH(63,45) (|u| <= 25); the rest of a random
    MLP around the shipped one stays live or not as the rule says, and pruning keeps every bit."""
    W1, b1, W2, b2 = message_mlp('cgnni_bch_63_45.npz')
    rng = np.random.default_rng(sum(dead) + len(dead))
    W1 = rng.uniform(-1, 1, 10).astype(F32)
    b1 = rng.uniform(0.5, 3, 10).astype(F32)          # W1 u >= 0 at one end of [-25, 23]: live
    for k in dead:
        b1[k] = -(abs(W1[k]) * F32(25) + F32(1))
    w1s, b1s, w2s, b2s, live = fold(W1, b1, W2, b2, 24)
    assert sorted(np.flatnonzero(~live)) == sorted(dead)
    v = np.random.default_rng(2).uniform(0, 24, 10000).astype(F32)
    full = mlp_eval(v, w1s, b1s, w2s, b2s, range(10))
    pruned = mlp_eval(v, w1s, b1s, w2s, b2s, np.flatnonzero(live))
    assert np.array_equal(full.view(np.uint32), pruned.view(np.uint32))
