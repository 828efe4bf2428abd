#!/bin/bash
# 1 M x 5, compact bus, two ticks in flight: the loop without an attachment, with a completion request on every step, and
# what a loop can do without it (view, then the synchronous calls) - three medians, each a run of its own
# (profiles/micro/awaited_loop_1m.py).  MODES="awaited cancelled": the awaited loop with and without a 16-key cancel on every step
# (ABI v24), in the same run.  Output: $OUT/awaited_loop_1m.txt (OUT: profiles/r15 unless set)
OUT=${OUT:-profiles/r15}
mkdir -p $OUT
O=$OUT/awaited_loop_1m.txt
{
  echo "# profiles/micro/awaited_loop_1m.sh on an MI355X: 1 M x 5, compact bus, two ticks in flight, steps without inbound rows; 1 M waiters, 1 % fresh and done per tick"
  echo "# ms per tick: the median (and quartiles) of the wall time of 80 ticks behind 16 of warm-up, through ctypes; each mode a process of its own"
  [ -n "${MODES:-}" ] && echo "# MODES=\"$MODES\" (cancelled: the awaited loop with a cancel of 16 exact tokens on every step - 16 waiters marked and delivered per tick beside the 1 %)"
} > $O
for mode in ${MODES:-plain awaited sync}; do
  timeout -k 10 240 python profiles/micro/awaited_loop_1m.py $mode >> $O || { echo "$mode: FAILED (rc $?)" >> $O; break; }
done
cat $O
