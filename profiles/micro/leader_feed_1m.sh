#!/bin/bash
# jg_engine_watch_leaders / jg_engine_census at 1 M and 16 M slots x R = 3: the timed run, then the same run under rocprofv3
# (kernel trace, --stats), summarised into profiles/r09/leader_feed_1m.txt's table.  Each GPU step has its own time limit.
set -euo pipefail  # (a GPU step that fails ends the script: its status is not tee's)
cd "$(dirname "$0")/../.."
OUT=${OUT:-$(mktemp -d -t leader_feed_1m.XXXXXX)}  # (the traces: give OUT to keep them somewhere else)
echo "output in $OUT"
mkdir -p "$OUT"
timeout -k 10 420 python profiles/micro/leader_feed_1m.py | tee "$OUT/timed.json"
timeout -k 10 540 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python profiles/micro/leader_feed_1m.py \
  | tee "$OUT/profiled.json"
python profiles/micro/leader_feed_1m.py --summarize "$OUT/prof" | tee "$OUT/summary.txt"
