#!/bin/bash
# AddressSanitizer + UBSan run of the guided-decimation host mirror
# (gnn-decode_amd/csrc/gnnd_bpgd_host.h): a plain host build of tools/bpgd_host_check.cpp on toric-5
# B = 9 under every parameter set of tests/bpgd_cases.py (both picks; the last set asks for V rounds
# of one pick, rounds * per_round >= V, and decimates every variable of some codeword) and on the
# irregular syn_hub under that last set, both dtypes, compared bit for bit with the numpy statement
# of tests/bpgd_cases.py.  No GPU, no Python under the sanitizer.
# usage: tools/bpgd_host_sanitize.sh [OUTDIR]
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-/tmp/gnnd_bpgd_hostsan}"
CXX="${CXX:-g++}"
mkdir -p "$OUT"
PYTHONPATH="$ROOT/gnn-decode_amd:$ROOT/tests" python3 - "$OUT" <<'EOF'
import sys
import bpgd_cases as bc
from gnndecode import _lib
from gnndecode.graph import edge_list
out = sys.argv[1]
CASES = [('toric_5', 9, k) for k in range(4)] + [('syn_hub', 9, 3)]
hx = lambda arr: ' '.join(float(t).hex() for t in arr.reshape(-1))
for code, B, pset in CASES:
    for dtype in ('float32', 'float64'):
        H, x = bc.inputs(code, B, dtype)
        v, c = edge_list(H)
        ref = bc.reference(code, B, dtype, pset)
        iters0, iters_round, rounds, per_round, pick = bc.params(H.shape[0])[pset]
        assert pset != 3 or (rounds * per_round >= H.shape[0] and 'full' in bc.COVERAGE[code, B][3])
        with open(f'{out}/{code}_{dtype}_{pset}.txt', 'w') as f:
            f.write(f'{H.shape[0]} {H.shape[1]} {v.size} {B} {int(dtype == "float64")} {iters0} '
                    f'{iters_round} {rounds} {per_round} {_lib.BPGD_PICK[pick]} '
                    f'{float(bc.CLAMP).hex()} {float(bc.ALPHA).hex()} {float(bc.BETA).hex()}\n')
            f.write('\n'.join(f'{a} {b}' for a, b in zip(v, c)) + '\n')
            f.write(hx(x) + '\n')
            f.write(hx(ref['llr']) + '\n')
            for name in ('iters', 'status', 'ndec'):
                f.write(' '.join(str(int(t)) for t in ref[name]) + '\n')
EOF
"$CXX" -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
  "$ROOT/tools/bpgd_host_check.cpp" -o "$OUT/bpgd_host_check"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/bpgd_host_check" "$OUT"/*.txt
