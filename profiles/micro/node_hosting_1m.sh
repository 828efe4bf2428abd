#!/bin/bash
# Hosting behind a kept node step at 1 M x 5, compact bus, two ticks in flight (profiles/micro/node_hosting_1m.py).  Two
# parts, every GPU step under its own time limit, a step that fails ends the script:
#   1. the unchanged paths against the parent commit: PARENT and CONTROL name two checkouts of the parent (built: the
#      library and host/bench_event_loop; node_hosting_1m.py copied into their profiles/micro) - the kept loop without an
#      attachment, the synchronous jg_engine_close_groups / jg_engine_open_groups calls (4096 listed slots, the range of all
#      slots) and the bench's two-ticks-in-flight line, the three trees alternating, RUNS (3) runs each.  Without PARENT the
#      part is skipped.
#   2. the attachment's cost in this tree: (a) the loop without, (b) a close of 4096 listed slots and an open of the 4096
#      closed a tick earlier on every step, (c) the same by a flush and the synchronous calls; and the kept kernels' own times
#      from a rocprofv3 --kernel-trace run of its own.
# Output: $OUT/node_hosting_1m.txt (OUT: profiles/r20 unless set).
set -uo pipefail
cd "$(dirname "$0")/../.."
HERE=$(pwd)
OUT=${OUT:-profiles/r20}
RUNS=${RUNS:-3}
mkdir -p "$OUT"
O=$OUT/node_hosting_1m.txt
TMP=$(mktemp -d -t node_hosting_1m.XXXXXX)
step() {  # step LIMIT COMMAND...: a GPU step of its own, its output in $TMP/out and $TMP/err; its failure ends the script
  local limit=$1
  shift
  timeout -k 10 "$limit" "$@" > "$TMP/out" 2> "$TMP/err"
  local rc=$?
  if [ $rc -ne 0 ]; then
    { echo "FAILED (rc $rc): $*"; tail -5 "$TMP/err"; } | tee -a "$O"
    exit $rc
  fi
}
bench() {  # bench TREE: the event-loop bench's two-ticks-in-flight line of that tree (pipetasks, compact bus)
  local tree=$1
  step 240 env LD_LIBRARY_PATH="$tree/josefine_amd/csrc:${LD_LIBRARY_PATH:-}" JG_BENCH_IN_FLIGHT=2 "$tree/josefine_amd/host/bench_event_loop" 1048576 5 40 10 pipetasks 0 1 4 compact
  tail -1 "$TMP/out" >> "$O"
}
{
  echo "# profiles/micro/node_hosting_1m.sh on an MI355X: 1 M x 5, compact bus, two ticks in flight, steps without inbound rows"
  echo "# loop rows: the median (and quartiles) of the wall time of 80 ticks behind 16 of warm-up, through ctypes; calls: best of three whole calls; each line a process of its own"
} > "$O"
if [ -n "${PARENT:-}" ]; then
  echo "== 1. unchanged paths: parent, control (a second copy of the parent), this - alternating, $RUNS runs each" >> "$O"
  for run in $(seq 1 "$RUNS"); do
    for tree in parent:$PARENT control:${CONTROL:-$PARENT} this:$HERE; do
      name=${tree%%:*} dir=${tree#*:}
      for mode in plain calls; do
        echo -n "$name run $run " >> "$O"
        step 240 python "$dir/profiles/micro/node_hosting_1m.py" $mode
        cat "$TMP/out" >> "$O"
      done
      echo -n "$name run $run bench " >> "$O"
      bench "$dir"
    done
  done
fi
echo "== 2. the attachment's cost (this tree)" >> "$O"
for mode in plain hosted sync; do
  step 240 python profiles/micro/node_hosting_1m.py $mode
  cat "$TMP/out" >> "$O"
done
echo "-- the kernels, under rocprofv3 --kernel-trace (the hosted loop once more, a run of its own; us)" >> "$O"
step 300 rocprofv3 --kernel-trace --stats -d "$TMP/prof" -o run -- python profiles/micro/node_hosting_1m.py hosted
step 60 python profiles/micro/node_hosting_1m.py --summarize "$TMP/prof"
cat "$TMP/out" >> "$O"
[ -n "${PARENT:-}" ] && python profiles/micro/node_hosting_1m.py --table "$O" > "$TMP/table" && cat "$TMP/table" >> "$O"
cat "$O"
