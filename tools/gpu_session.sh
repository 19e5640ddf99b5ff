#!/bin/bash
# One GPU-box session: gpu tests -> smoke -> bench -> rocprof kernel summary.
# Test failures (exit 1) do not stop the session; faults, aborts and time limits do.
# Outputs under $OUT_DIR (default: evidence_out/ in the repository root).
set -u
cd "$(dirname "$0")/.."
R=$PWD
O="${OUT_DIR:-$R/evidence_out}"
mkdir -p "$O"
export TMPDIR=/tmp
stop_if_fatal() {  # $1 = exit code, $2 = step name
  local rc=$1
  echo "[$2] exit $rc" | tee -a "$O/session.log"
  if [ "$rc" -ne 0 ] && [ "$rc" -ne 1 ]; then echo "fatal exit in $2; stopping" | tee -a "$O/session.log"; exit "$rc"; fi
}
STEPS="${STEPS:-tests smoke bench prof}"
for s in $STEPS; do
  case $s in
    tests) timeout -k 10 900 python -m pytest tests -m gpu -q -rf ${PYTEST_ARGS:-} > "$O/pytest_gpu.log" 2>&1; stop_if_fatal $? tests; tail -30 "$O/pytest_gpu.log" ;;
    smoke) timeout -k 10 300 python -c "import __graft_entry__ as g; g.build(); g.smoke()" > "$O/smoke.log" 2>&1; stop_if_fatal $? smoke; tail -3 "$O/smoke.log" ;;
    lab)   timeout -k 10 600 python tools/gemm_lab.py > "$O/gemm_lab.log" 2>&1; stop_if_fatal $? lab; grep -v "^\[\|amdgpu.ids" "$O/gemm_lab.log" | tail -20 ;;
    dwlab) timeout -k 10 300 python tools/dw_lab.py > "$O/dw_lab.log" 2>&1; stop_if_fatal $? dwlab; grep -v "^\[\|amdgpu.ids" "$O/dw_lab.log" | tail -8 ;;
    cfgs)  timeout -k 10 600 python tools/bench_configs.py > "$O/bench_configs.log" 2>&1; stop_if_fatal $? cfgs; grep "^{" "$O/bench_configs.log" ;;
    convbf) timeout -k 10 300 python tools/conv_bf16_bench.py > "$O/conv_bf16.log" 2>&1; stop_if_fatal $? convbf; grep -v "^\[" "$O/conv_bf16.log" | tail -20 ;;
    profcfg) (cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$O/prof_${CFG}" -o run --output-format csv -- python3 "$R/tools/bench_configs.py" --only ${CFG} --steps 5 > "$O/prof_${CFG}.log" 2>&1); stop_if_fatal $? profcfg ;;
    pmcg)  timeout -k 10 900 bash tools/pmc_generic.sh > "$O/pmcg.log" 2>&1; stop_if_fatal $? pmcg; tail -60 "$O/pmcg.log" ;;
    gemm)  timeout -k 10 300 python tools/gemm_bench.py > "$O/gemm_bench.log" 2>&1; stop_if_fatal $? gemm; grep -v "^\[" "$O/gemm_bench.log" | tail -20 ;;
    bench) timeout -k 10 600 python bench.py --full ${BENCH_ARGS:-} > "$O/bench.log" 2>&1; stop_if_fatal $? bench; tail -3 "$O/bench.log" ;;
    prof)  (cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$O/prof" -o run --output-format csv -- python3 "$R/bench.py" --full --steps 10 --warmup 3 --no-cpu-baseline > "$O/prof.log" 2>&1); stop_if_fatal $? prof; find "$O/prof" -name "*stats*" | head ;;
    pmc)   timeout -k 10 900 bash tools/pmc.sh > "$O/pmc.log" 2>&1; stop_if_fatal $? pmc; tail -25 "$O/pmc.log" ;;
    fold)  timeout -k 10 180 python tools/fold_bench.py > "$O/fold_bench.txt" 2>&1; stop_if_fatal $? fold; tail -1 "$O/fold_bench.txt" ;;
    bf16lab) LAB_ABL=${LAB_ABL:-0,2,32,34,-1} LAB_SHAPES=${LAB_SHAPES:-sq4096,sq8192,l3c1,l4c1,l4ds,l3c3} timeout -k 10 600 python tools/bf16_lab.py > "$O/bf16_lab.log" 2>&1; stop_if_fatal $? bf16lab; grep -v "^\[\|amdgpu.ids" "$O/bf16_lab.log" | tail -20 ;;
  esac
done
exit 0
