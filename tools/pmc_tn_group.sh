# FETCH_SIZE of the grouped weight-gradient kernel (tools/tn_group_bench.py) -> $XFM_PROF_OUT/pmc_tng.log; needs a GPU.
R=$(cd "$(dirname "$0")/.." && pwd)
export XFM_PROF_OUT=${XFM_PROF_OUT:-$R/profile_out}   # where profiles and logs go
O=$XFM_PROF_OUT
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/pmc_tng
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_tng -- python3 $R/tools/tn_group_bench.py > $O/pmc_tng.log 2>&1
python3 - <<PY
import csv, glob
tot, n = 0.0, 0
for f in glob.glob("$O/pmc_tng/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if r["Counter_Name"] == "FETCH_SIZE" and "gemm_tn_group_kernel" in r["Kernel_Name"]:
            tot += float(r["Counter_Value"]); n += 1
print("gemm_tn_group_kernel launches", n, "read bytes per launch (2 x FETCH_SIZE KB): %.2f GB" % (2 * tot * 1024 / max(n, 1) / 1e9))
PY
find $O/pmc_tng -type f -delete
