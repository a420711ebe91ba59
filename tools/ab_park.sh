#!/bin/bash
# same-box A/B of the parent commit against this tree, with the planner's park hint and with MJPCX_PARK=0 (profiles/r11_park_ab.log):
#   tools/ab_park.sh <parent tree> <out dir>
# <parent tree>: a clean copy of the parent commit, built there (python __graft_entry__.py). First the bit comparison of bench.py --dump-outputs of
# the two, then six alternating rounds of bench.py --steps 20 --warmup 6: parent / this tree (`new`) / this tree with MJPCX_PARK=0 (`nopark`).
# The judged figures are ms_per_step and value: the settling and resume launches lie outside the main kernel's events (kernel_ms).
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PARENT=$(cd "$1" && pwd)
mkdir -p "$2"
OUT=$(cd "$2" && pwd)
LOG=$OUT/r11_park_ab.log
: > $LOG
B="--gpus 1 --steps 20 --warmup 6 --no-cpu-baseline --no-extra"
bench() {  # name, tree, extra environment, extra arguments: one bench line -> $OUT/line_<name>.json; stops the script if the run fails
  local name=$1 tree=$2 e=$3; shift 3
  ( cd $tree && env $e timeout -k 10 120 python bench.py $B "$@" 2>$OUT/err_$name.txt | tail -1 > $OUT/line_$name.json ) || { echo "FAILED $name"; tail -5 $OUT/err_$name.txt; exit 1; }
}
bench dump_parent $PARENT AB=parent --dump-outputs $OUT/dump_parent
bench dump_new $ROOT AB=new --dump-outputs $OUT/dump_new
python $ROOT/tools/ab_report.py compare $OUT >> $LOG || exit 1
for r in 1 2 3 4 5 6; do
  bench parent $PARENT AB=parent; python $ROOT/tools/ab_report.py line parent $OUT/line_parent.json >> $LOG || exit 1
  bench new $ROOT AB=new; python $ROOT/tools/ab_report.py line new $OUT/line_new.json >> $LOG || exit 1
  bench nopark $ROOT MJPCX_PARK=0; python $ROOT/tools/ab_report.py line nopark $OUT/line_nopark.json >> $LOG || exit 1
done
python $ROOT/tools/ab_report.py summary $LOG >> $LOG || exit 1
cat $LOG
