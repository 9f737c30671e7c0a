#!/bin/bash
# AddressSanitizer + UBSan run of the union-find host mirror (gnn-decode_amd/csrc/gnnd_uf_host.h):
# a plain host build of tools/uf_host_check.cpp on toric-5 and ring-65 (B = 67, both dtypes) and on
# two_comp with two codewords that have no solution, compared exactly with the independent statement
# of tests/uf_cases.py.  No GPU, no Python under the sanitizer.
# usage: tools/uf_host_sanitize.sh [OUTDIR]
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-/tmp/gnnd_uf_hostsan}"
CXX="${CXX:-g++}"
mkdir -p "$OUT"
PYTHONPATH="$ROOT/gnn-decode_amd:$ROOT/tests" python3 - "$OUT" <<'EOF'
import sys
import numpy as np
import uf_cases as uc
from gnndecode.graph import edge_list
out = sys.argv[1]
hx = lambda arr: ' '.join(float(t).hex() for t in arr.reshape(-1))
ints = lambda arr: ' '.join(str(int(t)) for t in np.asarray(arr).reshape(-1))


def write(name, H, x, dtype, ref):
    v, c = edge_list(H)
    N, ends, _ = uc.matching_ref(H)
    B = x.size // sum(H.shape)
    with open(f'{out}/{name}_{dtype}.txt', 'w') as f:
        f.write(f'{H.shape[0]} {H.shape[1]} {v.size} {B} {int(dtype == "float64")} {N}\n')
        f.write('\n'.join(f'{a} {b}' for a, b in zip(v, c)) + '\n')
        f.write(ints(ends) + '\n' + hx(x) + '\n')
        for arr in ref:
            f.write(ints(arr) + '\n')


for shape in ('toric_5', 'ring_65'):
    for dtype in ('float32', 'float64'):
        H, x = uc.inputs(shape, uc.B_ALL, dtype)
        write(shape, H, x, dtype, uc.reference(shape, uc.B_ALL, dtype))
H = uc.code_matrix('two_comp')
V, C = H.shape
x = np.ones((3, V + C))
x[0, V + 2] = -1
x[1, V + 1] = x[1, V + 3] = -1
x[2, V + 0] = x[2, V + 1] = x[2, V + 4] = -1
r = uc.uf_ref(H, x.reshape(-1))
assert r['status'].tolist() == [1, 0, 1]
write('two_comp_unsat', H, x.reshape(-1), 'float64',
      (r['ehat01'], r['rounds'], r['status'], r['nfull']))
EOF
"$CXX" -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
  "$ROOT/tools/uf_host_check.cpp" -o "$OUT/uf_host_check"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/uf_host_check" "$OUT"/*.txt
