#!/bin/bash
# AddressSanitizer + UBSan run of the weighted union-find and belief-find host mirrors
# (gnn-decode_amd/csrc/gnnd_ufw_host.h): a plain host build of tools/ufw_host_check.cpp on toric-5
# and ring-65 (B = 67, both dtypes, llr and priors), on two_comp with two codewords that have no
# solution, compared exactly with the independent statement of tests/ufw_cases.py, and on the
# belief-find batch of that module, compared with the mirrors composed by hand.  No GPU, no Python
# under the sanitizer, nothing preloaded.
# usage: tools/ufw_host_sanitize.sh [OUTDIR]
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-/tmp/gnnd_ufw_hostsan}"
CXX="${CXX:-g++}"
mkdir -p "$OUT"
PYTHONPATH="$ROOT/gnn-decode_amd:$ROOT/tests" python3 - "$OUT" <<'EOF'
import sys
import numpy as np
import uf_cases as uc
import ufw_cases as wc
from gnndecode import ops
from gnndecode.graph import edge_list
out = sys.argv[1]
hx = lambda arr: ' '.join(float(t).hex() for t in np.asarray(arr).reshape(-1))
ints = lambda arr: ' '.join(str(int(t)) for t in np.asarray(arr).reshape(-1))


def head(f, kind, H, B, dtype, has_llr):
    v, c = edge_list(H)
    f.write(f'{kind} {H.shape[0]} {H.shape[1]} {v.size} {B} {int(dtype == "float64")} '
            f'{int(has_llr)} {float(wc.SCALE).hex()} {wc.WMAX}\n')
    f.write('\n'.join(f'{a} {b}' for a, b in zip(v, c)) + '\n')


def write(name, H, x, llr, dtype, ref):
    B = x.size // sum(H.shape)
    with open(f'{out}/{name}_{dtype}_{"llr" if llr is not None else "priors"}.txt', 'w') as f:
        head(f, 0, H, B, dtype, llr is not None)
        f.write(hx(x) + '\n')
        if llr is not None:
            f.write(hx(llr) + '\n')
        for arr in ref:
            f.write(ints(arr) + '\n')


for shape in ('toric_5', 'ring_65'):
    for dtype in ('float32', 'float64'):
        H, x, llr = wc.inputs(shape, wc.B_ALL, dtype)
        for l in (llr, None):
            write(shape, H, x, l, dtype, wc.reference(shape, wc.B_ALL, dtype, l is not None))
H = uc.code_matrix('two_comp')
V, C = H.shape
x = np.ones((3, V + C))
x[0, V + 2] = -1
x[1, V + 1] = x[1, V + 3] = -1
x[2, V + 0] = x[2, V + 1] = x[2, V + 4] = -1
llr = np.random.default_rng(3).normal(1.5, 2.5, 3 * V)
r = wc.ufw_ref(H, x.reshape(-1), llr)
assert r['status'].tolist() == [1, 0, 1]
write('two_comp_unsat', H, x.reshape(-1), llr, 'float64', wc.as_tuple(r, 'float64'))
# belief-find: the expected ehat is the statement's on min-sum's posteriors where min-sum stopped
# unsolved, and min-sum's hard decision elsewhere (the posteriors and the status from minsum_host)
for dtype in ('float32', 'float64'):
    H, x = wc.bf_inputs(dtype)
    V, C = H.shape
    pred, post, its, st = ops.minsum_host(H, x, wc.BF_ITERS, wc.BF_ALPHA, wc.BF_BETA, True)
    assert set(st.tolist()) == {0, 1}
    ehat = np.where((st != 0)[:, None], wc.ufw_ref(H, x, post)['ehat01'],
                    post.reshape(-1, V) < 0)
    with open(f'{out}/belief_find_{dtype}.txt', 'w') as f:
        head(f, 1, H, wc.B_ALL, dtype, False)
        f.write(hx(x) + '\n')
        f.write(f'{float(wc.BF_ALPHA).hex()} {float(wc.BF_BETA).hex()} {wc.BF_ITERS}\n')
        f.write(ints(ehat) + '\n' + ints(st) + '\n')
EOF
"$CXX" -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
  "$ROOT/tools/ufw_host_check.cpp" -o "$OUT/ufw_host_check"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/ufw_host_check" "$OUT"/*.txt
