#!/bin/bash
# AddressSanitizer + UBSan run of the OSD host mirror (gnn-decode_amd/csrc/gnnd_osd_host.h):
# a plain host build of tools/osd_host_check.cpp on the rank-deficient BCH graph, toric-7 and
# LDPC(648,324), both bases and dtypes, order 0, combination sweep and exhaustive, compared bit
# for bit with the numpy reference of tests/osd_hi_cases.py.  No GPU, no Python under the
# sanitizer.
# usage: tools/osd_host_sanitize.sh [OUTDIR]
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-/tmp/gnnd_osd_hostsan}"
CXX="${CXX:-g++}"
mkdir -p "$OUT"
PYTHONPATH="$ROOT/gnn-decode_amd:$ROOT/tests" python3 - "$OUT" <<'EOF'
import sys
import numpy as np
import osd_hi_cases as hc
from gnndecode.graph import edge_list
out = sys.argv[1]
METHODS = (('osd0', 0, 0), ('cs', 1, 10), ('cs', 1, 64), ('e', 2, 0), ('e', 2, 8), ('e', 2, 12))
for code, B in (('bch_dup', 4), ('toric_7', 9), ('ldpc_648_324', 3)):
    for dtype in ('float32', 'float64'):
        for base in ('zero', 'hard'):
            H, x, p = hc.inputs(code, B, dtype)
            v, c = edge_list(H)
            for method, mcode, order in METHODS:
                e, s, ch = hc.reference(code, B, dtype, base, method, order)
                with open(f'{out}/{code}_{dtype}_{base}_{method}{order}.txt', 'w') as f:
                    f.write(f'{H.shape[0]} {H.shape[1]} {v.size} {B} {int(base == "hard")} '
                            f'{int(dtype == "float64")} {mcode} {order}\n')
                    f.write('\n'.join(f'{a} {b}' for a, b in zip(v, c)) + '\n')
                    f.write(' '.join(repr(float(t)) for t in x) + '\n')
                    f.write(' '.join(repr(float(t)) for t in p) + '\n')
                    f.write(' '.join(str(int(t)) for t in e.reshape(-1)) + '\n')
                    f.write(' '.join(str(int(t)) for t in s) + '\n')
                    f.write(' '.join(str(int(t)) for t in ch) + '\n')
EOF
"$CXX" -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
  "$ROOT/tools/osd_host_check.cpp" -o "$OUT/osd_host_check"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/osd_host_check" "$OUT"/*.txt
