#!/bin/bash
# AddressSanitizer + UBSan run of the localized-statistics host mirrors
# (gnn-decode_amd/csrc/gnnd_lsd_host.h): a plain host build of tools/lsd_host_check.cpp on toric-5
# (B = 67), syn_c65 and syn_tall (B = 9, the latter with codewords that have no solution), both
# dtypes, both bases, bits_per_step 0, 1 and 3, compared exactly with the independent statement of
# tests/lsd_cases.py, and on the BP+LSD batch of that module, compared with the mirrors composed by
# hand.  No GPU, no Python under the sanitizer, nothing preloaded.
# usage: tools/lsd_host_sanitize.sh [OUTDIR]
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-/tmp/gnnd_lsd_hostsan}"
CXX="${CXX:-g++}"
mkdir -p "$OUT"
PYTHONPATH="$ROOT/gnn-decode_amd:$ROOT/tests" python3 - "$OUT" <<'EOF'
import sys
import numpy as np
import lsd_cases as lc
import osd_cases as oc
from gnndecode import ops
from gnndecode.graph import edge_list
out = sys.argv[1]
hx = lambda arr: ' '.join(float(t).hex() if t == t else 'nan' for t in np.asarray(arr).reshape(-1))
ints = lambda arr: ' '.join(str(int(t)) for t in np.asarray(arr).reshape(-1))


def head(f, kind, H, B, dtype, base, bits):
    v, c = edge_list(H)
    f.write(f'{kind} {H.shape[0]} {H.shape[1]} {v.size} {B} {int(dtype == "float64")} '
            f'{int(base == "hard")} {bits}\n')
    f.write('\n'.join(f'{a} {b}' for a, b in zip(v, c)) + '\n')


for code, B in (('toric_5', 67), ('syn_c65', 9), ('syn_tall', 9)):
    for dtype in ('float32', 'float64'):
        H, x, p = oc.inputs(code, B, dtype)
        for base in ('zero', 'hard'):
            for bits in lc.BITS:
                ref = lc.reference(code, B, dtype, base, bits)
                with open(f'{out}/{code}_{dtype}_{base}_{bits}.txt', 'w') as f:
                    head(f, 0, H, B, dtype, base, bits)
                    f.write(hx(x) + '\n' + hx(p) + '\n')
                    for k in lc.NAMES:
                        f.write(ints(ref[k]) + '\n')
assert lc.reference('syn_tall', 9, 'float64', 'zero', 1)['status'].any()
# BP+LSD: the expected ehat is the statement's on min-sum's soft output where min-sum stopped
# unsolved, and min-sum's hard decision elsewhere (both from bposd_host, whose first stage it is)
for dtype in ('float32', 'float64'):
    H, x, (iters, alpha, beta, early) = lc.bp_inputs(dtype)
    V, C = H.shape
    po = ops.bposd_host(H, x, iters, alpha, beta, early, 'zero', 'osd0', 0)
    st, pred, post = po[4], po[5], po[6]
    assert set(st.tolist()) == {0, 1}
    ehat = np.where((st != 0)[:, None], lc.ref_batch(H, x, pred, False, 1)['ehat'],
                    post.reshape(-1, V) < 0)
    with open(f'{out}/bplsd_{dtype}.txt', 'w') as f:
        head(f, 1, H, lc.BP_B, dtype, 'zero', 1)
        f.write(hx(x) + '\n')
        f.write(f'{float(alpha).hex()} {float(beta).hex()} {iters}\n')
        f.write(ints(ehat) + '\n' + ints(st) + '\n')
EOF
"$CXX" -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
  "$ROOT/tools/lsd_host_check.cpp" -o "$OUT/lsd_host_check"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/lsd_host_check" "$OUT"/*.txt
