#!/bin/bash
# the round's closing check on a fresh box: every GPU test, smoke(), and the bench at 20 timed + 5 warm-up steps (--full: the roofline figure)
O=${LOGS:-logs}/r6
mkdir -p $O
timeout 2400 python -m pytest tests -m gpu -x -q > $O/final_tests.log 2>&1; echo "tests rc $?"; tail -2 $O/final_tests.log
timeout 600 python -c 'import __graft_entry__ as g; g.smoke()' > $O/final_smoke.log 2>&1; echo "smoke rc $?"; tail -2 $O/final_smoke.log
timeout 900 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > $O/final_bench.json 2> $O/final_bench.err; echo "bench rc $?"
python - "$O/final_bench.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print({k: d[k] for k in ("metric", "value", "ms_per_step")}, d["roofline"]["frac"], d["roofline"].get("traffic"), d["config"].get("ms_per_step_median"))
PY
