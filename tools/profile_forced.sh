# rocprofv3 kernel-trace summary of the pre-training step with the N > 1 code path forced in a group of one (XFM_DDP_FORCE=1):
# the RCCL kernel rows and the per-chunk grouped weight gradients -> $XFM_PROF_OUT/prof_forced/b_kernel_stats.csv
R=$(cd "$(dirname "$0")/.." && pwd)
export XFM_PROF_OUT=${XFM_PROF_OUT:-$R/profile_out}   # where profiles and logs go
O=$XFM_PROF_OUT
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_forced
cd $R && XFM_DDP_FORCE=1 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_forced -o b -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-clocks --no-fusion-probe > $O/prof_forced.log 2>&1
find $O/prof_forced -name "*kernel_trace*" -delete
tail -1 $O/prof_forced.log | cut -c1-200
