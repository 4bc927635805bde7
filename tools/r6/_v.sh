O=${LOGS:-logs}/r6
mkdir -p $O
timeout 2400 python -m pytest tests -m gpu -x -q > $O/v_tests.log 2>&1; echo "tests rc $?"; tail -1 $O/v_tests.log
bash tools/gpu_check.sh prof > $O/v_prof.log 2>&1; tail -1 $O/v_prof.log
timeout 900 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > $O/final_bench.json 2> $O/final_bench.err; echo "bench rc $?"
python - "$O/final_bench.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["ms_per_step"], d["roofline"]["frac"], d["roofline"].get("traffic"), d["config"].get("ms_per_step_median"))
PY
