# Every tracked artifact of a round in one go (run on the GPU box; copies land in $XFM_PROF_OUT/round/, to be moved into profiles/):
#   bash tools/round_profiles.sh A   -> headline: bench line, kernel stats (default + single stream), gemm shapes
#   bash tools/round_profiles.sh B   -> headline: HBM traffic + MFMA utilisation (PMC passes)
#   bash tools/round_profiles.sh C   -> secondary workloads: bench lines + kernel stats
R=$(cd "$(dirname "$0")/.." && pwd)
export XFM_PROF_OUT=${XFM_PROF_OUT:-$R/profile_out}   # where profiles and logs go
O=$XFM_PROF_OUT/round
mkdir -p $O
case "$1" in
A)
  cd $R && XFM_BENCH_GEMM_SHAPES=$O/gemm_shapes.txt python3 bench.py --full > $O/bench_pretrain.json 2> $O/bench_pretrain.err
  bash tools/profile_bench.sh pretrain && cp $XFM_PROF_OUT/prof_stats/b_kernel_stats.csv $O/bench_kernel_stats.csv
  bash tools/profile_serial.sh && cp $XFM_PROF_OUT/prof_serial/b_kernel_stats.csv $O/bench_kernel_stats_single_stream.csv
  ;;
B)
  cd $R && bash tools/pmc_traffic.sh > /dev/null 2>&1; cp $XFM_PROF_OUT/hbm_traffic.json $O/hbm_traffic.json
  bash tools/pmc_mfma.sh > /dev/null 2>&1; cp $XFM_PROF_OUT/mfma_util.json $O/mfma_util.json
  ;;
C)
  cd $R
  for w in imagenet retrieval vqa glue; do
    python3 bench.py --full --workload $w > $O/bench_$w.json 2> $O/bench_$w.err
    bash tools/profile_bench.sh $w && cp $XFM_PROF_OUT/prof_stats/b_kernel_stats.csv $O/${w}_kernel_stats.csv
  done
  ;;
esac
ls -la $O
