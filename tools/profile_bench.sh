# rocprofv3 kernel-trace summary of a bench workload -> $XFM_PROF_OUT/prof_stats/b_kernel_stats.csv (copy it to profiles/).
# usage: bash tools/profile_bench.sh [workload]   (default: the pre-training step; imagenet | retrieval | vqa | glue)
R=$(cd "$(dirname "$0")/.." && pwd)
export XFM_PROF_OUT=${XFM_PROF_OUT:-$R/profile_out}   # where profiles and logs go
O=$XFM_PROF_OUT
mkdir -p $O
W=${1:-pretrain}
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_stats
cd $R && rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_stats -o b -- python3 bench.py --full --workload $W --steps 5 --warmup 2 --no-cpu-baseline --no-clocks --no-fusion-probe > $O/prof_stats.log 2>&1
find $O/prof_stats -name "*kernel_trace*" -delete
tail -1 $O/prof_stats.log | cut -c1-160
