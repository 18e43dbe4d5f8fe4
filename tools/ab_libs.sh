#!/bin/bash
# GPU box: tools/ab_libs.sh "<workloads>" lib1.so lib2.so ...  (paths relative to mujoco-torch_amd/lib/; "base" = libmjhip.so) -- bench digests, base first and last
# AB_REPS=n: n interleaved rounds of (lib1 lib2 ... base) instead (a build against its parent: the difference of the medians against each build's own min-to-max spread);
# AB_STEPS / AB_WARMUP: the timed window (default 100 / 10); AB_RAW=dir: the raw bench lines are kept there, one file per workload and library.
# Every run is its own process under its own time limit, and the first one that fails ends the script.
wl="$1"; shift
steps=${AB_STEPS:-100}; warm=${AB_WARMUP:-10}; reps=${AB_REPS:-0}
[ -n "$AB_RAW" ] && mkdir -p "$AB_RAW"
run() {  # $1 = workload, $2 = library name
  local w=$1 n=$2 lib=mujoco-torch_amd/lib/$2 line
  [ $n = base ] && lib=mujoco-torch_amd/lib/libmjhip.so
  line=$(MJH_LIB=$PWD/$lib timeout -k 10 300 python3 bench.py --workload $w --steps $steps --warmup $warm --no-cpu-baseline --no-other-workloads --no-long-run 2>/dev/null) || { echo "ab_libs: $w $n failed ($?)" >&2; exit 1; }
  [ -n "$AB_RAW" ] && echo "$line" | grep '^{' >> "$AB_RAW/${w}_${n%.so}.jsonl"
  echo "$line" | python3 tools/benchline.py "$n" || exit 1
}
for w in $wl; do
  if [ "$reps" -gt 0 ]; then
    for r in $(seq $reps); do for n in "$@" base; do run $w $n; done; done
  else
    for n in base "$@" base; do run $w $n; done
  fi
done
