# Counter calibration (tools/calib/fetch_calib) and grid-size sweeps of the bench kernels.
# Output under $OUT (default bench_out/). --full: the summary reads the kernel pass.
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
summ() { python3 -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); r=d['roofline']; print(sys.argv[1], d['value'], 'Mpps step', d['ms_per_step'], 'kern', r['kernel_ms'], 'ms frac', r['frac'])" $1; }
timeout -k 10 120 rocprofv3 -L > "$OUT/counters_list.txt" 2>&1; grep -o 'TCC_EA0_[A-Z0-9_]*' "$OUT/counters_list.txt" | sort -u | tr '\n' ' '; echo
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/calib_fetch" -o run -- ./tools/calib/fetch_calib > "$OUT/calib.log" 2>&1 || exit 4
timeout -k 10 300 rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum --output-format csv -d "$OUT/calib_rdreq" -o run -- ./tools/calib/fetch_calib >> "$OUT/calib.log" 2>&1 || echo rdreq-pass-failed
python3 tools/calib/analyze.py "$OUT/calib_fetch/run_counter_collection.csv"
for gw in 4096 8192 16384 32768; do
  timeout -k 10 200 python bench.py --full --config c2 --steps 20 --warmup 3 --no-cpu --grid-waves $gw > "$OUT/gs_c2_$gw.json" 2>&1 || exit 3
  summ "$OUT/gs_c2_$gw.json"
done
for gw in 4096 8192; do
  for cfg in c3 c4; do
  timeout -k 10 200 python bench.py --full --config $cfg --steps 20 --warmup 3 --no-cpu --grid-waves $gw > "$OUT/gs_${cfg}_$gw.json" 2>&1 || exit 3
  summ "$OUT/gs_${cfg}_$gw.json"
  done
done
