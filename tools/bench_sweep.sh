# bench.py over frames in flight x hardware queues (GPU box): bash tools/bench_sweep.sh
# Results in $OUT/sweep.txt (OUT: a fresh temporary directory unless set).
OUT=${OUT:-$(mktemp -d)}
mkdir -p "$OUT"
: > "$OUT/sweep.txt"
for rep in 1 2; do
for q in ${QS:-8 16}; do for f in ${FS:-4 6 8}; do
  GPU_MAX_HW_QUEUES=$q timeout -k 10 100 python bench.py --full --no-cpu-baseline --no-parity --steps 300 --inflight $f > "$OUT/sw.log" 2>&1 || exit 1
  python -c "
import json; t=open('$OUT/sw.log').read(); d=json.loads(t[t.index('{'):].splitlines()[0]); print($rep, 'q$q', 'F$f', d['ms_per_step'], d['frame_latency_ms'])" >> "$OUT/sweep.txt"
done; done; done
cat "$OUT/sweep.txt"
