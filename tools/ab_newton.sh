#!/bin/bash
# same-box A/B of the parent commit's library against this tree's, as tools/ab_prune.sh (profiles/r12_newton_ab.log):
#   tools/ab_newton.sh <parent libmjpcx.so> <out dir>
# <parent libmjpcx.so>: built from a clean copy of the parent commit (python __graft_entry__.py there). Only the library differs between the
# two builds, so the two take turns in this tree. First the bit comparison of bench.py --dump-outputs of the two, pruned and with MJPCX_PRUNE=0,
# then six alternating rounds of bench.py --steps 20 --warmup 6: parent / this tree (`new`).
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PARENT=$(cd "$(dirname "$1")" && pwd)/$(basename "$1")
mkdir -p "$2"
OUT=$(cd "$2" && pwd)
LOG=$OUT/r12_newton_ab.log
: > $LOG
LIB=$ROOT/mujoco_mpc_amd/libmjpcx.so
cp $LIB $OUT/new.so || exit 1
trap 'cp $OUT/new.so $LIB' EXIT
B="--gpus 1 --steps 20 --warmup 6 --no-cpu-baseline --no-extra"
bench() {  # name, library, extra environment, extra arguments: one bench line -> $OUT/line_<name>.json; stops the script if the run fails
  local name=$1 lib=$2 e=$3; shift 3
  cp $lib $LIB || exit 1
  ( cd $ROOT && env $e timeout -k 10 150 python bench.py $B "$@" 2>$OUT/err_$name.txt | tail -1 > $OUT/line_$name.json ) || { echo "FAILED $name"; tail -5 $OUT/err_$name.txt; exit 1; }
}
for mode in "AB=pruned" "MJPCX_PRUNE=0"; do
  rm -rf $OUT/dump_parent $OUT/dump_new
  bench dump_parent $PARENT $mode --dump-outputs $OUT/dump_parent
  bench dump_new $OUT/new.so $mode --dump-outputs $OUT/dump_new
  echo "outputs with $mode:" >> $LOG
  python $ROOT/tools/ab_report.py compare $OUT >> $LOG || { cat $LOG; exit 1; }
done
for r in 1 2 3 4 5 6; do
  bench parent $PARENT AB=parent; python $ROOT/tools/ab_report.py line parent $OUT/line_parent.json >> $LOG || exit 1
  bench new $OUT/new.so AB=new; python $ROOT/tools/ab_report.py line new $OUT/line_new.json >> $LOG || exit 1
done
python $ROOT/tools/ab_report.py summary $LOG >> $LOG || exit 1
cat $LOG
