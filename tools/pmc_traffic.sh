# HBM traffic per kernel family: two separate PMC passes (FETCH_SIZE, WRITE_SIZE) over a short bench run, then
# tools/hbm_traffic.py sums them per family into profiles/<round>_hbm_traffic.json.  Run on the GPU box via gpurun.
R=$(cd "$(dirname "$0")/.." && pwd)
export XFM_PROF_OUT=${XFM_PROF_OUT:-$R/profile_out}   # where profiles and logs go
O=$XFM_PROF_OUT
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/pmc_fetch $O/pmc_write
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-clocks --no-fusion-probe > $O/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_write -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-clocks --no-fusion-probe > $O/pmc_write.log 2>&1
cd $R && python3 tools/hbm_traffic.py $O/pmc_fetch $O/pmc_write 4 > $O/hbm_traffic.json
find $O/pmc_fetch $O/pmc_write -type f -delete
cat $O/hbm_traffic.json | head -50
