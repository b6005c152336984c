#!/bin/bash
# Round profiles: rocprof kernel trace + FETCH_SIZE + WRITE_SIZE passes for the given configs, then bench lines.
#   bash tools/gpu_prof_all.sh <tag> <configs...>
set -o pipefail
cd "$GRAFT_REPO_ROOT"
tag=$1; shift
mkdir -p gpurun_out
for cfg in "$@"; do
    # collect.sh ends with "profiles collected under <directory>": the bench lines go beside that directory
    prof=$(bash profiles/collect.sh "$tag" "$cfg" | tee /dev/stderr | sed -n 's/^profiles collected under //p') || exit 1
    [ -d "$prof" ] || { echo "collect.sh named no profile directory for c$cfg"; exit 1; }
    echo "profiled c$cfg"
done
logs=$(dirname "$prof")
for cfg in "$@"; do
    log=$logs/bench_c$cfg.log
    ACC_BENCH_KERNELS=1 timeout -k 10 600 python -u bench.py --config $cfg --full > "$log" 2>&1 \
        || { echo "bench c$cfg failed"; tail -30 "$log"; exit 1; }
    tail -1 "$log" | cut -c1-300
done
