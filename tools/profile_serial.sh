# rocprofv3 kernel-trace summary of the bench workload with the side streams off (every kernel alone on the GPU: isolated
# per-kernel durations, the measure of machine work) -> $XFM_PROF_OUT/prof_serial/b_kernel_stats.csv
R=$(cd "$(dirname "$0")/.." && pwd)
export XFM_PROF_OUT=${XFM_PROF_OUT:-$R/profile_out}   # where profiles and logs go
O=$XFM_PROF_OUT
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_serial
export XFM_WGRAD_STREAM=0 XFM_TEXT_STREAM=0
cd $R && rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_serial -o b -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-clocks --no-fusion-probe > $O/prof_serial.log 2>&1
find $O/prof_serial -name "*kernel_trace*" -delete
tail -1 $O/prof_serial.log | cut -c1-200
python3 tools/profile_summary.py $O/prof_serial/b_kernel_stats.csv 8 60 > $O/prof_serial_summary.md
