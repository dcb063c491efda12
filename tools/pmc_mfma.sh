# MFMA pipe utilisation per kernel family from SQ counters (one PMC pass, kernels one at a time) -> $XFM_PROF_OUT/mfma_util.json
R=$(cd "$(dirname "$0")/.." && pwd)
export XFM_PROF_OUT=${XFM_PROF_OUT:-$R/profile_out}   # where profiles and logs go
O=$XFM_PROF_OUT
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/pmc_mfma
export XFM_WGRAD_STREAM=0 XFM_TEXT_STREAM=0
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_BUSY_CYCLES --kernel-trace --output-format csv -d $O/pmc_mfma -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-clocks --no-fusion-probe > $O/pmc_mfma.log 2>&1
cd $R && python3 tools/mfma_util.py $O/pmc_mfma > $O/mfma_util.json
find $O/pmc_mfma -type f -delete
cat $O/mfma_util.json
