#!/bin/bash
# ONE parametrised script for the same-box A/B runs of a gpurun call (boxes differ by several percent between calls, so
# every comparison is made inside one call, interleaved):
#   tools/gpu_ab.sh <tag> <rounds> "<configs>" "<label>=<ENV=VAL ENV=VAL ...>" ["<label>=<...>" ...]
#   tools/gpu_ab.sh r03_fuse 2 "2d 3dpart" "base=" "fuse2=HDU_FUSE_BN_BWD=2"
# A label may also name a library: "prev=LIB=tools/libhdu_prev.so" (copied over h-denseunet_amd/libhdu.so for that arm), or a whole
# other checkout with its own built library: "parent=TREE=/path/to/checkout" (that tree's bench.py runs; nothing is copied).
# A bench process that aborts, faults or runs into its time limit ends the script: nothing more is started on that GPU.
# Writes gpurun_out/ab_<tag>.txt: one line per (round, config, label) with ms_per_step.
tag=$1; rounds=$2; configs=$3; shift 3
cd "$(dirname "$0")/.."
mkdir -p gpurun_out
out=gpurun_out/ab_$tag.txt
: > "$out"
cp h-denseunet_amd/libhdu.so /tmp/libhdu_cur.so
for r in $(seq 1 "$rounds"); do
  for cfg in $configs; do
    for arm in "$@"; do
      label=${arm%%=*}; envs=${arm#*=}
      libsel=/tmp/libhdu_cur.so
      cleaned=""
      tree=.
      for kv in $envs; do
        if [ "${kv%%=*}" = LIB ]; then libsel=${kv#LIB=}; elif [ "${kv%%=*}" = TREE ]; then tree=${kv#TREE=}; else cleaned="$cleaned $kv"; fi
      done
      [ "$tree" = . ] && cp "$libsel" h-denseunet_amd/libhdu.so
      env $cleaned timeout -k 10 300 python "$tree/bench.py" --config "$cfg" --steps ${AB_STEPS:-20} --warmup 4 --no-cpu-baseline --no-roofline --extras none >/tmp/ab_line.json 2>>"${out%.txt}.err"
      rc=$?
      ms=$(grep -o '"ms_per_step": [0-9.]*' /tmp/ab_line.json | head -1)
      echo "round $r  $cfg  $label  ${ms:-FAILED rc=$rc}" | tee -a "$out"
      case $rc in 124|134|137|139) cp /tmp/libhdu_cur.so h-denseunet_amd/libhdu.so; echo "bench ended with status $rc: stopping" | tee -a "$out"; exit $rc;; esac
    done
  done
done
cp /tmp/libhdu_cur.so h-denseunet_amd/libhdu.so
