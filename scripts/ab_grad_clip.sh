#!/bin/bash
# Same-box cost of global-norm clipping on the graphed CNN steps, alternated (off / on, twice) to
# cancel drift, plus the kernels' achieved bytes/s.
# A threshold of 1e30 runs the clipped kernels with unchanged math.
set -o pipefail
# Usage: bash scripts/ab_grad_clip.sh [out.jsonl]
out=${1:-grad_clip_ab.jsonl}
mkdir -p "$(dirname "$out")"
for n in 44595786 11689512; do
  r=$(timeout -k 10 120 python -u scripts/bench_grad_clip.py --n $n 2>&1 | tail -1) || { echo "FAIL kernels: $r"; exit 1; }
  echo "{\"kind\": \"kernels\", \"line\": $r}" | tee -a "$out"
done
for rep in 1 2; do
  for cfg in "enhanced_cnn adam" "resnet18 sgd"; do
    set -- $cfg
    for v in "--clip 0" "--clip 1e30"; do
      r=$(timeout -k 10 200 python -u scripts/bench_cnn.py --model $1 --batch 64 --optimizer $2 --graph --no-stock --steps 100 --warmup 20 $v 2>&1 | tail -1) || { echo "FAIL $cfg $v: $r"; exit 1; }
      echo "{\"kind\": \"step\", \"rep\": $rep, \"line\": $r}" | tee -a "$out"
    done
  done
done
