export OUT=${OUT:-/tmp/bench_out}; mkdir -p $OUT      # where the outputs go
timeout -k 10 900 python bench.py --full > $OUT/bench_default2.json 2> $OUT/bench_default2.err; echo rc=$?
python - <<'PY'
import json, os
d=json.loads(open(os.environ["OUT"] + "/bench_default2.json").read().strip().splitlines()[-1])
print("main", d["ms_per_step"], "exact", d["exact_f32"]["ms_per_step"], "f16", d["config3_f16"]["ms_per_step"], "bf16", d["config3_bf16"]["ms_per_step"])
PY
grep -v amdgpu $OUT/bench_default2.err | tail -5
