# A/B of two builds of libbeatrice_gpu.so in alternating processes on one box:
#   bash tools/gpu_abx.sh <libA.so> <libB.so> "<configs>" [reps] [extra bench args]
# The lines go to $OUT (default bench_out/). --full: the summary reads the kernel pass.
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
A=$1; B=$2; CFGS=$3; REPS=${4:-3}; shift 4; EXTRA="$@"
summ() { python3 -c "import json,sys; d=json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1]); r=d['roofline']; print(sys.argv[2], sys.argv[3], d['value'], 'Mpps step', d['ms_per_step'], 'kern', r['kernel_ms'])" $1 $2 $3; }
for cfg in $CFGS; do
  for i in $(seq $REPS); do
    for v in A B; do
      L=$A; [ $v = B ] && L=$B
      F="$OUT/ab_${cfg}_${v}_$i.json"
      BT_LIB_PATH=$PWD/$L timeout -k 10 200 python bench.py --full --configs none --config $cfg --steps 20 --warmup 3 --no-cpu $EXTRA > "$F" 2>&1 || { tail -5 "$F"; exit 3; }
      summ "$F" $cfg $v
    done
  done
done
