#!/bin/bash
# Parent and new build interleaved, several processes per build and leg, one
# JSON line per process.  Run from the root of the new tree (built):
#   speed_runs.sh <root of a built checkout of the parent commit> <output directory>
set -o pipefail
R=$PWD
P=$(cd "$1" && pwd)
mkdir -p "$2"
O=$(cd "$2" && pwd)
run() {  # leg, build, index, time limit (s), bench.py arguments
    local leg=$1 b=$2 i=$3 lim=$4; shift 4
    local dir=$R; [ $b = parent ] && dir=$P
    ( cd $dir && timeout -k 10 $lim python bench.py --gpus 1 "$@" > $O/${leg}_${b}_$i.json 2> $O/${leg}_${b}_$i.err ) \
        || { echo "FAILED $leg $b $i rc=$?"; tail -5 $O/${leg}_${b}_$i.err; exit 1; }
    echo "$leg $b $i done"
}
for i in 1 2 3 4; do
    run dna272 parent $i 240 --workload dna272 --full --cpu-baseline 0
    run dna272 new $i 240 --workload dna272 --full --cpu-baseline 0
done
for i in 1 2 3; do
    run headline parent $i 240 --steps 3 --warmup 1
    run headline new $i 240 --steps 3 --warmup 1
done
for i in 1 2 3; do
    run config5 parent $i 400 --algo msa --p 0.002 --batch-per-gpu 1000000 --steps 2 --warmup 1
    run config5 new $i 400 --algo msa --p 0.002 --batch-per-gpu 1000000 --steps 2 --warmup 1
done
echo ALL_DONE
