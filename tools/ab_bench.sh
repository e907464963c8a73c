#!/bin/bash
# Same-box A/B of two builds of the library: the output hashes of both (tools/ab_hash.py), then alternating runs of the
# default bench line, the driver's command, one launch sequence at a time and the training step.
#   bash tools/ab_bench.sh OLD [out.txt]
# OLD is a library built from the other sources, loaded by this tree's Python:
#   make -C transcar_amd/csrc -j8 BUILD=../../build/ab_old LIB=../../build/ab_old/libtranscar_old.so EXTRA=-D...
# or, when the two differ in what they export, a built checkout of the other commit (with this tree's tools/ab_hash.py
# copied over its own), run from its own directory.
OLD=${1:-build/ab_old/libtranscar_old.so}
OUT=${2:-gpurun_out/ab.txt}
mkdir -p "$(dirname "$OUT")"
OUT=$(realpath "$OUT")
V='import json,sys; d=json.loads(sys.stdin.read()); print(d[sys.argv[1]])'
# every run under a time limit of its own; the first one that fails ends the script (nothing more is started on the GPU)
new() { timeout -k 10 600 python "$@"; }
old() { if [ -d "$OLD" ]; then (cd "$OLD" && timeout -k 10 600 python "$@"); else TRANSCAR_HIP_LIB=$OLD timeout -k 10 600 python "$@"; fi; }
hashes() { local out; out=$("$1" tools/ab_hash.py 2>&1) || { echo "$out" | tail -5; echo "$1 ab_hash.py failed"; exit 1; }; echo "$out" | grep "^rows"; }
line() {   # label, build, key of the result line, bench.py arguments
  local out
  out=$("$2" bench.py "${@:4}" --main-only --no-cpu-baseline 2>/dev/null) || { echo "$2 $1: bench.py ${*:4} failed"; exit 1; }
  echo "$2 $1: $(echo "$out" | tail -1 | python -c "$V" "$3")"
}
{
echo "== hashes new"; hashes new
echo "== hashes old"; hashes old
for i in 1 2 3; do
  for b in new old; do line default $b value; done
  for b in new old; do line driver $b value --gpus 1 --steps 20 --warmup 5; done
  for b in new old; do line 1lane $b value --lanes 1; done
  for b in new old; do line "train ms_per_step" $b ms_per_step --train; done
done
} > "$OUT" 2>&1
