#!/bin/bash
# Round-6: the default bench line (every config) and the alltypes profile after the D1 routing change.
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd "$R"
mkdir -p gpurun_out/r06_bench
(cd "$_" && timeout -k 10 600 python "$R/bench.py" --full > bench.json 2> bench.err) || exit 1  # in the directory made above
bash tools/profile.sh alltypes r06_at --variants 0 --pcie 0 --cpu-baseline 0 || exit 1
