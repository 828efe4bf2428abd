#!/bin/bash
# jg_engine_watch_replicas_timed beside jg_engine_watch_replicas at 1 M slots x R = 5: the timed run, then the same run under
# rocprofv3 (kernel trace, --stats), summarised into profiles/r13/isr_clock_1m.txt's table.  Each GPU step has its own time
# limit; a step that fails ends the script.
set -euo pipefail  # (a GPU step that fails ends the script: its status is not tee's)
cd "$(dirname "$0")/../.."
OUT=${OUT:-$(mktemp -d -t isr_clock_1m.XXXXXX)}  # (the traces: give OUT to keep them somewhere else)
echo "output in $OUT"
mkdir -p "$OUT"
timeout -k 10 300 python profiles/micro/isr_clock_1m.py | tee "$OUT/timed.json"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python profiles/micro/isr_clock_1m.py \
  | tee "$OUT/profiled.json"
python profiles/micro/isr_clock_1m.py --summarize "$OUT/prof" | tee "$OUT/summary.txt"
mkdir -p profiles/r13
{
  echo "# bash profiles/micro/isr_clock_1m.sh on one MI355X: the timed run (ms; three repetitions each), then the kernels of the same script under rocprofv3 --kernel-trace --stats (us)"
  cat "$OUT/timed.json"
  echo
  cat "$OUT/summary.txt"
} > profiles/r13/isr_clock_1m.txt
