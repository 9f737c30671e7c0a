#!/bin/bash
# AddressSanitizer + UBSan run of the gated-OSD and BP+OSD host mirrors
# (gnn-decode_amd/csrc/gnnd_osd_host.h, gnnd_bposd_host.h): a plain host build of
# tools/bposd_host_check.cpp on toric-5, the rank-deficient BCH graph and LDPC(648,324), both
# dtypes, compared with the numpy statement of tests/bposd_cases.py.  No GPU, no Python under the
# sanitizer.
# usage: tools/bposd_host_sanitize.sh [OUTDIR]
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-/tmp/gnnd_bposd_hostsan}"
CXX="${CXX:-g++}"
mkdir -p "$OUT"
PYTHONPATH="$ROOT/gnn-decode_amd:$ROOT/tests" python3 - "$OUT" <<'EOF'
import sys
import bposd_cases as bc
import minsum_cases as mc
import osd_cases as oc
from gnndecode import _lib
from gnndecode.graph import edge_list
out = sys.argv[1]
hexes = lambda a: ' '.join(float(t).hex() for t in a) + '\n'
ints = lambda a: ' '.join(str(int(t)) for t in a.reshape(-1)) + '\n'
GATED = [('toric_5', 9, 'zero', 'alt'), ('toric_5', 9, 'zero', 'zeros'), ('bch_dup', 4, 'hard', 'ones'),
         ('bch_dup', 4, 'zero', 'alt'), ('ldpc_648_324', 3, 'hard', 'alt')]
for k, (code, B, base, gname) in enumerate(GATED):
    for dtype in ('float32', 'float64'):
        H, x, p = oc.inputs(code, B, dtype)
        v, c = edge_list(H)
        L = bc.llr_input(code, B, dtype)
        g = bc.gate(code, B, dtype, gname)
        for (method, order), with_llr in ((('cs', 10), True), (('e', 8), False)):
            ehat, st, ch = bc.gated_reference(code, B, dtype, base, method, order, gname, with_llr)
            with open(f'{out}/gated_{code}_{dtype}_{k}_{method}.txt', 'w') as f:
                f.write(f'G {H.shape[0]} {H.shape[1]} {v.size} {B} {int(dtype == "float64")} '
                        f'{_lib.OSD_BASE[base]} {_lib.OSD_METHOD[method]} {order} {int(with_llr)}\n')
                f.write('\n'.join(f'{a} {b}' for a, b in zip(v, c)) + '\n')
                f.write(hexes(x) + hexes(p) + (hexes(L) if with_llr else '') + ints(g))
                f.write(ints(ehat) + ints(st) + ints(ch))
for code, B, base in (('toric_5', 9, 'zero'), ('ldpc_648_324', 3, 'hard')):
    for dtype in ('float32', 'float64'):
        H, x = mc.inputs(code, B, dtype)
        v, c = edge_list(H)
        alpha, beta, iters, early = bc.bp_params(code)
        llr, its, st = mc.reference(code, B, dtype, bc.bp_params(code))
        with open(f'{out}/bposd_{code}_{dtype}.txt', 'w') as f:
            f.write(f'P {H.shape[0]} {H.shape[1]} {v.size} {B} {int(dtype == "float64")} '
                    f'{_lib.OSD_BASE[base]} {_lib.OSD_METHOD["cs"]} 10 {float(alpha).hex()} '
                    f'{float(beta).hex()} {iters} {early}\n')
            f.write('\n'.join(f'{a} {b}' for a, b in zip(v, c)) + '\n')
            f.write(hexes(x) + hexes(llr) + ints(its) + ints(st))
EOF
"$CXX" -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
  "$ROOT/tools/bposd_host_check.cpp" -o "$OUT/bposd_host_check"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT/bposd_host_check" "$OUT"/*.txt
