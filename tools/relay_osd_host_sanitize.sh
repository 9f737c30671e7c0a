#!/bin/bash
# AddressSanitizer + UBSan run of the soft relay and relay+OSD host mirrors
# (gnn-decode_amd/csrc/gnnd_relay_host.h): a plain host build of tools/relay_osd_host_check.cpp on
# toric-5 (every parameter set of tests/relay_cases.py) and on the irregular LDPC(648,324) (the
# short legs that run out), both dtypes and both soft modes, soft / llr / the integers compared bit
# for bit with the numpy statement of tests/relay_osd_cases.py, the OSD stage with its composition
# from the two mirrors.  No GPU, no Python under the sanitizer.
# usage: tools/relay_osd_host_sanitize.sh [OUTDIR]
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-/tmp/gnnd_relay_osd_hostsan}"
CXX="${CXX:-g++}"
mkdir -p "$OUT"
PYTHONPATH="$ROOT/gnn-decode_amd:$ROOT/tests" python3 - "$OUT" <<'EOF'
import sys
import relay_cases as rc
import relay_osd_cases as roc
from gnndecode import _lib
from gnndecode.graph import edge_list
out = sys.argv[1]
CASES = [('toric_5', 9, p) for p in rc.PARAMS] + [('ldpc_648_324', 3, rc.PARAMS[3])]
hx = lambda arr: ' '.join(float(t).hex() for t in arr.reshape(-1))
for k, (code, B, params) in enumerate(CASES):
    for dtype in ('float32', 'float64'):
        H, x = roc.inputs(code, B, dtype, params)
        v, c = edge_list(H)
        ref = roc.reference(code, B, dtype, params)
        legs, iters0, iters_leg, S = params
        for mode in roc.MODES:
            with open(f'{out}/{code}_{dtype}_{mode}_{k}.txt', 'w') as f:
                f.write(f'{H.shape[0]} {H.shape[1]} {v.size} {B} {int(dtype == "float64")} {legs} '
                        f'{iters0} {iters_leg} {S} {float(rc.ALPHA).hex()} {float(rc.BETA).hex()} '
                        f'{_lib.RELAY_SOFT[mode]} {_lib.OSD_BASE[roc.base_of(code)]} '
                        f'{_lib.OSD_METHOD[roc.METHOD]} {roc.ORDER}\n')
                f.write('\n'.join(f'{a} {b}' for a, b in zip(v, c)) + '\n')
                f.write(hx(x) + '\n')
                f.write(hx(rc.gammas(H.shape[0], params, dtype)) + '\n')
                f.write(hx(ref['soft_' + mode]) + '\n')
                f.write(hx(ref['llr']) + '\n')
                for name in ('iters', 'status', 'leg', 'nsol'):
                    f.write(' '.join(str(int(t)) for t in ref[name]) + '\n')
EOF
"$CXX" -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
  "$ROOT/tools/relay_osd_host_check.cpp" -o "$OUT/relay_osd_host_check"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/relay_osd_host_check" "$OUT"/*.txt
