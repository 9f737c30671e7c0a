#!/bin/bash
# AddressSanitizer + UBSan run of the layered min-sum host mirror
# (gnn-decode_amd/csrc/gnnd_minsum_layered_host.h): a plain host build of
# tools/minsum_layered_host_check.cpp on toric-5 and LDPC(648,324), both dtypes, every parameter set
# of tests/minsum_cases.py on toric-5 and the first on LDPC, compared bit for bit with the numpy
# statement of tests/minsum_layered_cases.py.  No GPU, no Python under the sanitizer.
# usage: tools/minsum_layered_host_sanitize.sh [OUTDIR]
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-/tmp/gnnd_minsum_layered_hostsan}"
CXX="${CXX:-g++}"
mkdir -p "$OUT"
PYTHONPATH="$ROOT/gnn-decode_amd:$ROOT/tests" python3 - "$OUT" <<'EOF'
import sys
import minsum_layered_cases as mc
from gnndecode.graph import edge_list
out = sys.argv[1]
CASES = [('toric_5', 9, p) for p in mc.PARAMS] + [('ldpc_648_324', 5, mc.PARAMS[0])]
for k, (code, B, params) in enumerate(CASES):
    for dtype in ('float32', 'float64'):
        H, x = mc.inputs(code, B, dtype)
        v, c = edge_list(H)
        llr, its, st = mc.reference(code, B, dtype, params)
        alpha, beta, iters, early = params
        with open(f'{out}/{code}_{dtype}_{k}.txt', 'w') as f:
            f.write(f'{H.shape[0]} {H.shape[1]} {v.size} {B} {int(dtype == "float64")} '
                    f'{float(alpha).hex()} {float(beta).hex()} {iters} {early}\n')
            f.write('\n'.join(f'{a} {b}' for a, b in zip(v, c)) + '\n')
            f.write(' '.join(float(t).hex() for t in x) + '\n')
            f.write(' '.join(float(t).hex() for t in llr) + '\n')
            f.write(' '.join(str(int(t)) for t in its) + '\n')
            f.write(' '.join(str(int(t)) for t in st) + '\n')
EOF
"$CXX" -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
  "$ROOT/tools/minsum_layered_host_check.cpp" -o "$OUT/minsum_layered_host_check"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/minsum_layered_host_check" "$OUT"/*.txt
