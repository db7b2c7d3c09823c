export PYTHONUNBUFFERED=1
R=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${OUT:-/tmp/bench_out}; mkdir -p $OUT      # where the outputs go
cd $R
GLF_STREAMS=0 timeout -k 10 300 python bench.py --steps 8 --warmup 3 --no-config3 --no-exact-f32 --no-cpu-baseline 2>&1 | tail -1 | cut -c100-200
cd /tmp && export TMPDIR=/tmp
GLF_STREAMS=0 timeout -k 10 500 rocprofv3 --kernel-trace --stats -d /tmp/prof -o p --output-format csv -- python3 $R/bench.py --steps 4 --warmup 2 --no-config3 --no-cpu-baseline --no-exact-f32 --full > /tmp/prof.log 2>&1 || tail -5 /tmp/prof.log
f=$(find /tmp/prof -name "*kernel_stats.csv" | head -1)
cp $f $OUT/step_kernel_stats.csv
tail -1 /tmp/prof.log | cut -c100-200
