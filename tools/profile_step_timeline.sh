# Per-queue occupancy of the default (multi-stream) bench step: $XFM_PROF_OUT/step_timeline.txt
R=$(cd "$(dirname "$0")/.." && pwd)
export XFM_PROF_OUT=${XFM_PROF_OUT:-$R/profile_out}   # where profiles and logs go
O=$XFM_PROF_OUT
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_tl
cd $R && rocprofv3 --kernel-trace --output-format csv -d $O/prof_tl -o t -- python3 bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-fusion-probe > $O/prof_tl.log 2>&1
T=$(find $O/prof_tl -name "*kernel_trace.csv" | head -1)
LIST=${LIST:-0:2.6} WAKE=${WAKE:-0.5} GANTT=${GANTT:-1} STEP_KERNEL=${STEP_KERNEL:-adamw_kernel:3:4} python3 tools/timeline.py $T 0.45 30 > $O/step_timeline.txt 2>&1
find $O/prof_tl -type f -delete
head -12 $O/step_timeline.txt
