#!/bin/bash
# jg_engine_watch_completions at 1 M slots x R = 5 with 1 M and 4 M waiters: the timed run (with the host baseline), then the
# kernels under rocprofv3 (kernel trace, --stats), then - in runs of their own - the counters FETCH_SIZE and WRITE_SIZE, summarised
# into profiles/r14/completion_feed_1m.txt.  Each GPU step has its own time limit; a step that fails ends the script.
set -euo pipefail  # (a GPU step that fails ends the script: its status is not tee's)
cd "$(dirname "$0")/../.."
OUT=${OUT:-$(mktemp -d -t completion_feed_1m.XXXXXX)}  # (the traces: give OUT to keep them somewhere else)
echo "output in $OUT"
mkdir -p "$OUT" profiles/r14
timeout -k 10 540 python profiles/micro/completion_feed_1m.py | tee "$OUT/timed.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python profiles/micro/completion_feed_1m.py --kernels-only \
  | tee "$OUT/profiled.json" &&
python profiles/micro/completion_feed_1m.py --summarize "$OUT/prof" | tee "$OUT/summary.txt" &&
{
  echo "# bash profiles/micro/completion_feed_1m.sh on one MI355X: the timed run (ms; three repetitions each), then the kernels of the same script (one repetition, no host baseline) under rocprofv3 --kernel-trace --stats (us), then FETCH_SIZE / WRITE_SIZE from a counter run of its own"
  cat "$OUT/timed.json"
  echo
  cat "$OUT/summary.txt"
} > profiles/r14/completion_feed_1m.txt &&
timeout -k 10 120 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_fetch" -o run -- python profiles/micro/completion_feed_1m.py --counters-only \
  > "$OUT/pmc_fetch.json" &&
timeout -k 10 120 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_write" -o run -- python profiles/micro/completion_feed_1m.py --counters-only \
  > "$OUT/pmc_write.json" &&
{
  echo
  echo "# counters (W = 1 M, one repetition per done fraction: the timed watch, the flush; one counter per run - the two do not fit one pass)"
  python profiles/micro/completion_feed_1m.py --pmc "$OUT/pmc_fetch"
  python profiles/micro/completion_feed_1m.py --pmc "$OUT/pmc_write"
} >> profiles/r14/completion_feed_1m.txt
