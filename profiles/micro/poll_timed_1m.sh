#!/bin/bash
# jg_engine_poll carrying the clock against poll(leaders, commits) + jg_engine_watch_replicas_timed at 1 M slots x R = 5, on
# twin engines: the timed run, then the same run under rocprofv3 (kernel trace and --stats, nothing else), summarised into
# profiles/r14/poll_timed_1m.txt's table.  Each GPU step has its own time limit; a step that fails ends the script.
set -o pipefail  # (a GPU step that fails ends the chain: its status is not tee's)
cd "$(dirname "$0")/../.."
OUT=${OUT:-$(mktemp -d -t poll_timed_1m.XXXXXX)}  # (the traces: give OUT to keep them somewhere else)
echo "output in $OUT"
mkdir -p "$OUT" profiles/r14 &&
timeout -k 10 300 python profiles/micro/poll_timed_1m.py | tee "$OUT/timed.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python profiles/micro/poll_timed_1m.py \
  | tee "$OUT/profiled.json" &&
python profiles/micro/poll_timed_1m.py --summarize "$OUT/prof" | tee "$OUT/summary.txt" &&
{
  echo "# bash profiles/micro/poll_timed_1m.sh on one MI355X: the timed run (ms; three repetitions each, all reported), then the count passes of the same script under rocprofv3 --kernel-trace --stats (us)"
  cat "$OUT/timed.json"
  echo
  cat "$OUT/summary.txt"
} > profiles/r14/poll_timed_1m.txt
