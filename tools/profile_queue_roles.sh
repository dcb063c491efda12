R=$(cd "$(dirname "$0")/.." && pwd)
export XFM_PROF_OUT=${XFM_PROF_OUT:-$R/profile_out}   # where profiles and logs go
O=$XFM_PROF_OUT
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_qr
cd $R && XFM_DDP_FORCE=1 rocprofv3 --kernel-trace --output-format csv -d $O/prof_qr -o t -- python3 bench.py --full --steps 3 --warmup 2 --no-cpu-baseline --no-clocks --no-fusion-probe > $O/prof_qr.log 2>&1
T=$(find $O/prof_qr -name "*kernel_trace.csv" | head -1)
python3 tools/queue_roles.py $T
find $O/prof_qr -type f -delete
