R=$(cd "$(dirname "$0")/.." && pwd)
export XFM_PROF_OUT=${XFM_PROF_OUT:-$R/profile_out}   # where profiles and logs go
O=$XFM_PROF_OUT
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_ft
cd $R && XFM_DDP_FORCE=${FORCE:-1} rocprofv3 --kernel-trace --output-format csv -d $O/prof_ft -o t -- python3 bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-clocks --no-fusion-probe > $O/prof_ft.log 2>&1
T=$(find $O/prof_ft -name "*kernel_trace.csv" | head -1)
python3 tools/queue_map.py $T 2 > $O/queue_map_${FORCE:-1}.txt 2>&1
find $O/prof_ft -type f -delete
