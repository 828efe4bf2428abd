#!/bin/bash
# jg_engine_read_chains at 1 M groups x 64 blocks, R = 5: the timed run, then the same run under rocprofv3 (kernel and
# memory-copy traces), summarised into profiles/r07/read_chains_1m_x_64.txt's table.  Each GPU step has its own time limit.
set -euo pipefail  # (a GPU step that fails ends the script: its status is not tee's)
cd "$(dirname "$0")/../.."
OUT=${OUT:-$(mktemp -d -t read_chains_1m.XXXXXX)}  # (the traces: give OUT to keep them somewhere else)
echo "output in $OUT"
mkdir -p "$OUT"
timeout -k 10 600 python profiles/micro/read_chains_1m.py | tee "$OUT/timed.json"
timeout -k 10 900 rocprofv3 --kernel-trace --memory-copy-trace --stats -d "$OUT/prof" -o run -- python profiles/micro/read_chains_1m.py \
  | tee "$OUT/profiled.json"
python profiles/micro/read_chains_1m.py --summarize "$OUT/prof" | tee "$OUT/summary.txt"
