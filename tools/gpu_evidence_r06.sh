#!/bin/bash
# Round-6 evidence on the shipped kernels, written to OUTDIR (copy OUTDIR/r06_* into profiles/ afterwards):
#   r06_bench.json                       the full bench line (cfg2, B=128, extras, cpu_baseline: bench.py --full)
#   r06_cfg2_b{128,512,1000}_kernel_stats.csv   rocprofv3 --kernel-trace --stats of a plain bench run at that batch
#   r06_step_trace.txt                   start times of the step's kernels inside the real captured step (trace build)
#   r06_bench_<cfg>.json + r06_<cfg>_kernel_stats.csv   the other BASELINE workloads (CFGS=... to choose)
OUT=${1:?usage: tools/gpu_evidence_r06.sh OUTDIR}
cd "${GRAFT_REPO_ROOT:-.}" || exit 1
mkdir -p "$OUT"; export TMPDIR=/tmp
python3 bench.py --full --steps 200 --warmup 20 > "$OUT/r06_bench.json" 2> "$OUT/r06_bench.err"; echo "bench rc=$?"; cut -c1-400 "$OUT/r06_bench.json"
for B in ${BATCHES:-128 512 1000}; do
  rm -rf "$OUT/prof_b$B"
  rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_b$B" -- python3 bench.py --batch $B --steps 30 --warmup 5 > /dev/null 2> "$OUT/prof_b$B.err"; echo "prof B=$B rc=$?"
  f=$(find "$OUT/prof_b$B" -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp "$f" "$OUT/r06_cfg2_b${B}_kernel_stats.csv"
  rm -rf "$OUT/prof_b$B"
done
[ -f tools/probe/libmmvae_trace.so ] && MMVAE_HIP_LIB=$PWD/tools/probe/libmmvae_trace.so python3 tools/probe/trace_step.py > "$OUT/r06_step_trace.txt" 2>/dev/null; cat "$OUT/r06_step_trace.txt"
for c in ${CFGS:-}; do
  python3 bench.py --full --config $c --steps 50 --warmup 10 > "$OUT/r06_bench_$c.json" 2> "$OUT/r06_bench_$c.err"; echo "$c bench rc=$?"
  cut -c1-260 "$OUT/r06_bench_$c.json"
  rm -rf "$OUT/prof_$c"
  rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$c" -- python3 bench.py --config $c --steps 20 --warmup 5 > /dev/null 2> "$OUT/prof_$c.err"; echo "$c prof rc=$?"
  f=$(find "$OUT/prof_$c" -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp "$f" "$OUT/r06_${c}_kernel_stats.csv"
  rm -rf "$OUT/prof_$c"
done
