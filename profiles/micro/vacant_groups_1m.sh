#!/bin/bash
# jg_engine_open_groups / jg_engine_close_groups / jg_engine_list_groups at 1 M and 16 M slots x R = 3: the timed run, then
# the same run under rocprofv3 (kernel trace, --stats), summarised into profiles/r07/vacant_groups_1m.txt's table.  Each GPU
# step has its own time limit.
set -euo pipefail  # (a GPU step that fails ends the script: its status is not tee's)
cd "$(dirname "$0")/../.."
OUT=${OUT:-$(mktemp -d -t vacant_groups_1m.XXXXXX)}  # (the traces: give OUT to keep them somewhere else)
echo "output in $OUT"
mkdir -p "$OUT"
timeout -k 10 600 python profiles/micro/vacant_groups_1m.py | tee "$OUT/timed.json"
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python profiles/micro/vacant_groups_1m.py \
  | tee "$OUT/profiled.json"
python profiles/micro/vacant_groups_1m.py --summarize "$OUT/prof" | tee "$OUT/summary.txt"
