#!/bin/bash
# quick GPU check: parity tests + bench kernel table (files under $OUT, default out/)
export OUT=${OUT:-out}; mkdir -p $OUT
python -m pytest tests -m gpu -q -x 2>&1 | grep -E "passed|failed|FAILED|^E " | head -8 | tee $OUT/pytest_tail.txt
python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/bq.json 2>$OUT/bq.err || tail -5 $OUT/bq.err
python - <<'PY'
import json, os
d=json.load(open(os.path.join(os.environ["OUT"], "bq.json")))
print("graphs/s", d["value"], "ms/step", d["ms_per_step"], "roofline", d["roofline"])
tot=0
for k,v in sorted(d["kernels"].items(), key=lambda kv:-kv[1]["ms_per_step"])[:11]:
    tot+=v["ms_per_step"]; print(f'{k:26s} {v["ms_per_step"]:8.3f} ms  {v.get("tflops","")} TF  {v.get("gbs","")} GB/s')
print("sum top", tot)
PY
