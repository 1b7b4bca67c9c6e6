# A/B two library builds on one box (GPU box): bash tools/ab_lib.sh libA.so libB.so [reps]
# Results in $OUT/ab_lib.txt (OUT: a fresh temporary directory unless set).
A=$1; B=$2; R=${3:-2}
OUT=${OUT:-$(mktemp -d)}
mkdir -p "$OUT"; : > "$OUT/ab_lib.txt"
for rep in $(seq 1 $R); do for L in $A $B; do
  MIRT_LIB=distributed_raytracer_amd/$L timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-parity --steps 300 > "$OUT/ab.log" 2>&1 || exit 1
  python -c "
import json; t=open('$OUT/ab.log').read(); d=json.loads(t[t.index('{'):].splitlines()[0]); print($rep, '$L', 'bench', d['ms_per_step'], d['frame_latency_ms'])" >> "$OUT/ab_lib.txt"
  MIRT_LIB=distributed_raytracer_amd/$L timeout -k 10 100 python tools/inflight_probe.py --view away --world 1 --inflight 4 --maxwg 256 --repeat 1 | grep world | sed "s/^/$rep $L away /" >> "$OUT/ab_lib.txt"
done; done
cat "$OUT/ab_lib.txt"
