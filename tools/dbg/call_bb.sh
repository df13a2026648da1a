#!/bin/sh
# (files go to $OUT)
: "${OUT:?set OUT to an output directory}"; mkdir -p "$OUT"; export OUT
python -m pytest tests/test_backbone_gpu.py -x -q -m gpu 2>&1 | tail -6
for v in 0 64 128 256; do
  python bench.py --full --no-cpu-baseline --no-extras --bb-set s3_conv3_min_planes=$v 2>"$OUT/bb_err.txt" | tail -1 > "$OUT/bb_$v.json"
  tail -c 200 "$OUT/bb_err.txt"
  python - "$v" <<'PY'
import json, os, sys
d = json.load(open(os.path.join(os.environ["OUT"], "bb_%s.json" % sys.argv[1])))
print("s3_conv3_min_planes", sys.argv[1], d["value"], d["ms_per_step"], str(d["pipeline_check"])[:40])
PY
done
