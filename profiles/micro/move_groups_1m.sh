#!/bin/bash
# jg_engine_export_groups / jg_engine_import_groups at 1 M groups x R = 5: the timed run, then the same run under rocprofv3
# (kernel and memory-copy traces, --stats), summarised into profiles/r07/move_groups_1m_x_5.txt's table.  Each GPU step has
# its own time limit.
set -euo pipefail  # (a GPU step that fails ends the script: its status is not tee's)
cd "$(dirname "$0")/../.."
OUT=${OUT:-$(mktemp -d -t move_groups_1m.XXXXXX)}  # (the traces: give OUT to keep them somewhere else)
echo "output in $OUT"
mkdir -p "$OUT"
timeout -k 10 600 python profiles/micro/move_groups_1m.py | tee "$OUT/timed.json"
timeout -k 10 900 rocprofv3 --kernel-trace --memory-copy-trace --stats -d "$OUT/prof" -o run -- python profiles/micro/move_groups_1m.py \
  | tee "$OUT/profiled.json"
python profiles/micro/move_groups_1m.py --summarize "$OUT/prof" | tee "$OUT/summary.txt"
