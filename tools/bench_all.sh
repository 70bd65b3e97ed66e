# every full benchmark line of one revision: tools/bench_all.sh OUT_DIR   (bench_<name>.json per run, one summary line each)
O=${1:?usage: tools/bench_all.sh OUT_DIR}
mkdir -p "$O"
python bench.py --full --steps 20 --warmup 5 > "$O/bench_drv_b.json" 2> "$O/bench_drv_b.err"
python bench.py --full > "$O/bench_default_b.json" 2>/dev/null
python bench.py --full --n-per-dim 171 > "$O/bench_1e7_b.json" 2>/dev/null
python bench.py --full --nvt --no-cpu-baseline > "$O/bench_nvt_b.json" 2>/dev/null
python bench.py --full --workload ethane > "$O/bench_ethane_b.json" 2>/dev/null
python - "$O" <<PY
import json, sys
for f in ("drv_b","default_b","1e7_b","nvt_b","ethane_b"):
    try:
        d=json.loads(open("%s/bench_%s.json"%(sys.argv[1], f)).read().strip().splitlines()[-1])
        print(f, "%.4g"%d["value"], "%.3f ms"%d["ms_per_step"], "steady", d.get("steady_state_value"), "force", "%.3f"%d["roofline"]["avg_launch_ms"], "frac %.4f"%d["roofline"]["frac"], "traffic", d["roofline"]["traffic"], d["device_ms_per_step"]["list_build_ms_per_build"])
    except Exception as e: print(f, "ERR", e)
PY
