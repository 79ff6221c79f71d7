#!/bin/bash
# Round evidence in one gpurun call: the PMC traffic passes first (bench.py reads profiles/traffic_latest.json for
# roofline.traffic, so it must come from the SAME build), then the default bench line, then the same command under
# rocprofv3 --kernel-trace --stats. Usage (on the GPU box): bash tools/evidence.sh <tag>; copy gpurun_out/*<tag>* into profiles/.
set -e
TAG=${1:-r01x}
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd "$R"
mkdir -p gpurun_out
bash tools/pmc_traffic.sh > gpurun_out/pmc_${TAG}.log 2>&1
cp gpurun_out/pmc_traffic/traffic.json gpurun_out/traffic_${TAG}.json
cp gpurun_out/pmc_traffic/traffic.json profiles/traffic_latest.json
# the bench lines and their kernel statistics go to $BENCH_OUT (default: bench_out/ in the repository root)
B=${BENCH_OUT:-$R/bench_out}
mkdir -p "$B"
python bench.py --full > "$B/bench_${TAG}.json" 2> "$B/bench_${TAG}.err"
rm -rf "$B/prof_${TAG}"
rocprofv3 --kernel-trace --stats --output-format csv -d "$B/prof_${TAG}" -o p -- python3 bench.py --full --no-cpu-baseline > "$B/bench_${TAG}_prof.json" 2> "$B/bench_${TAG}_prof.err"
tail -c 600 "$B/bench_${TAG}.json"
