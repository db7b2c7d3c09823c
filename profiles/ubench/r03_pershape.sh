export PYTHONUNBUFFERED=1
R=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${OUT:-/tmp/bench_out}; mkdir -p $OUT      # where the outputs go
cd $R
GLF_BENCH_DUMP=$OUT/per_shape timeout -k 10 400 python bench.py --steps 4 --warmup 2 --no-config3 --no-cpu-baseline --no-exact-f32 --full $1 > $OUT/bench_dump.json 2> $OUT/bench_dump.err || tail -5 $OUT/bench_dump.err
python - <<'PY'
import csv, json, os
d = json.load(open(os.environ["OUT"] + "/bench_dump.json"))
r = d["roofline"]
print("ms/step", d["ms_per_step"], "frac", r["frac"], "avg_launch_ms", r["avg_launch_ms"], "all frac", r["all_contractions"]["mfma_frac_of_peak"], "contr s/step", r["all_contractions"]["s_per_step"])
rows = list(csv.DictReader(open(os.environ["OUT"] + "/per_shape.f16x3.csv")))
tot = sum(float(x["ms_per_step"]) for x in rows)
print("sum of per-shape ms/step", round(tot, 1))
for x in rows[:45]:
    print(f"{x['kernel']:26s} M={x['M']:>7} N={x['N']:>5} K={x['K']:>6} taps={x['kept_taps']} b={x['batch']:>2} split={x['split']:>3} dil={x['dil']:>2} n={x['launches_per_step']:>3} ms={float(x['ms_per_step']):6.2f} avg={float(x['avg_ms']):.4f} execTF={float(x['executed_TF']):6.1f}")
PY
