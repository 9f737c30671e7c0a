# usage: tools/torchrun_check.sh OUTDIR
set -o pipefail
OUT="$1"; mkdir -p "$OUT"
export MASTER_ADDR=127.0.0.1
echo "=== torchrun decode $(date +%T)"
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --full --gpus 1 --steps 50 --warmup 5 --cpu-seconds 0 > "$OUT/torchrun_decode.log" 2>&1 && tail -c 600 "$OUT/torchrun_decode.log" &&
echo "=== torchrun train $(date +%T)" &&
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29534 bench.py --full --gpus 1 --mode train --steps 20 --warmup 3 > "$OUT/torchrun_train.log" 2>&1 && tail -c 400 "$OUT/torchrun_train.log" &&
echo "=== default bench $(date +%T)" &&
( time timeout -k 10 400 python bench.py --full > "$OUT/default_bench.log" 2>&1 ) 2> "$OUT/default_bench.time" && cat "$OUT/default_bench.time" && tail -c 300 "$OUT/default_bench.log" &&
echo "=== done $(date +%T)"
