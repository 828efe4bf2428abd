#!/bin/bash
# jg_engine_await_cancel at 1 M slots x R = 5 with 1 M waiters over 100 connections: the timed run (one connection withdrawn with
# 1, 2 048 and 65 536 keys, whole-call ms through the binding, best of three, the watch behind each, and a device-to-device copy
# of the table's bytes), then the kernels of the same script under rocprofv3 (kernel trace, --stats) in a run of its own,
# summarised into profiles/r16/await_cancel_1m.txt.  Each GPU step has its own time limit; a step that fails ends the script.
set -euo pipefail  # (a GPU step that fails ends the script: its status is not tee's)
cd "$(dirname "$0")/../.."
OUT=${OUT:-$(mktemp -d -t await_cancel_1m.XXXXXX)}  # (the traces: give OUT to keep them somewhere else)
echo "output in $OUT"
mkdir -p "$OUT" profiles/r16
timeout -k 10 300 python profiles/micro/await_cancel_1m.py | tee "$OUT/timed.json" &&
timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python profiles/micro/await_cancel_1m.py --kernels-only \
  | tee "$OUT/profiled.json" &&
python profiles/micro/await_cancel_1m.py --summarize "$OUT/prof" | tee "$OUT/summary.txt" &&
{
  echo "# bash profiles/micro/await_cancel_1m.sh on one MI355X: the timed run (ms; three repetitions each), then the kernels of the same script (one repetition) under rocprofv3 --kernel-trace --stats (us)"
  cat "$OUT/timed.json"
  echo
  echo "# the profiled run's own line (one repetition; its copy_table_bytes_ms is the copy timed in that run)"
  cat "$OUT/profiled.json"
  echo
  cat "$OUT/summary.txt"
} > profiles/r16/await_cancel_1m.txt
