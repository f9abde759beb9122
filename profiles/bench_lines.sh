set -e
# usage: profiles/bench_lines.sh OUTDIR -- the full bench.py line (sub-records, parity) of every single-GPU workload, one file each
OUT=${1:?usage: profiles/bench_lines.sh OUTDIR}
mkdir -p "$OUT"
for wl in cfg2 cfg2nc cfg1 cfg1c cfg3; do
  python3 bench.py --full --workload $wl > "$OUT/bench_$wl.json" 2> "$OUT/bench_$wl.err"
  tail -c 300 "$OUT/bench_$wl.json"
done
python3 bench.py --full --weights bf16 > "$OUT/bench_cfg2_weights_bf16.json" 2>/dev/null
