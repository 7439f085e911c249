#!/bin/bash
# One parameterised script for every GPU-box job of a round (replaces the per-experiment one-offs):
#   bash tools/gpu.sh <task> [args] [-- <task> [args] ...]
# Logs, traces and counter summaries go to $SE3DS_OUT (default: out/ in the repository root).
# tasks:
#   tests [pytest args]         GPU suite (default: whole suite), log in $OUT/pytest_gpu.log
#   smoke                       __graft_entry__.smoke()
#   bench [bench.py args]       bench line (--full: with everything beyond the headline) -> $OUT/bench_default.log
#   ab 'ENV=v ENV=v' ...        A/B of the gan_step bench under env settings (baseline first), 2 reps
#   abwarp 'ENV=v' ...          the same for --workload warp (random and room depth; WARP_H=512 in the environment: at that height)
#   prof_step TAG [ENV=v ...]   rocprofv3 kernel stats of the default bench -> $OUT/TAG_kernel_stats.csv
#   prof_warp TAG [ENV=v ...]   kernel stats of the warp bench, random + room depth
#   pmc_conv TAG "SHAPE"        MFMA-busy / FETCH / WRITE counters of tools/one_conv.py SHAPE (3 passes)
#   pmc_warp TAG                FETCH / WRITE counters of the warp kernels (2 passes)
#   pmc_warp_valu TAG           VALU / LDS counters of the warp kernels (1 pass) -> $OUT/TAG_warp_valu_pmc.json
#   pmc_step TAG [ENV=v ...]    MFMA-busy + shader clock of every kernel inside the step (1 pass, tools/pmc_step.py)
#   prof_py TAG <file.py> [args] rocprofv3 kernel stats of any python tool -> $OUT/TAG_kernel_stats.csv
#   pmc_py TAG "PMC ..." REGEX <file.py> [args]   one --pmc pass over any python tool -> $OUT/TAG_pmc.json
#   video_input [args]          tools/video_input_bench.py (fused evaluation input transform vs op by op) -> $OUT/video_input_bench.json
#   py <file.py> [args]         any python tool
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
ulimit -c 0
OUT=${SE3DS_OUT:-out}
mkdir -p "$OUT"
line() { python -c "import json,sys
d=json.loads(sys.stdin.readline()); r=d['roofline']
print('ms/step %.2f value %.3f frac %.4f' % (d['ms_per_step'], d['value'], r['frac']), 'in_step %.4f' % r['frac_in_step'] if 'frac_in_step' in r else '')"; }
task_tests() {
  SECONDS=0
  if [ $# -eq 0 ]; then set -- tests; fi
  timeout 3000 python -m pytest "$@" -m gpu -x -q --durations=10 > $OUT/pytest_gpu.log 2>&1
  echo "pytest rc=$? elapsed $SECONDS s"; tail -22 $OUT/pytest_gpu.log | cut -c1-200
}
task_smoke() {
  timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
  echo "smoke rc=$?"; tail -3 $OUT/smoke.log
}
task_bench() {
  SECONDS=0
  timeout 1200 python bench.py "$@" > $OUT/bench_default.log 2> $OUT/bench_default.err
  echo "bench rc=$? elapsed $SECONDS s"; tail -1 $OUT/bench_default.log | cut -c1-7000; tail -3 $OUT/bench_default.err | cut -c1-300
}
task_ab() {
  for rep in 1 2; do
    for v in "SE3DS_NOP=1" "$@"; do
      echo "== $v"
      env $v timeout 600 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-batch-max --no-warp --no-shipped --no-fp32 2>$OUT/ab.err | line || tail -5 $OUT/ab.err
    done
  done
}
task_abwarp() {
  for rep in 1 2; do
    for v in "SE3DS_NOP=1" "$@"; do
      for d in random room; do
        echo "== $v ($d)"
        env $v timeout 300 python bench.py --full --workload warp --warp-height ${WARP_H:-1024} --warp-depth $d --steps 200 --warmup 20 --no-cpu-baseline 2>$OUT/ab.err | python -c "import json,sys
d=json.loads(sys.stdin.readline()); r=d['roofline']
print('us/render %.1f frac %.4f step_ms %.4f' % (1e3*r['ms_per_launch'], r['frac'], d['ms_per_step']))" || tail -5 $OUT/ab.err
      done
    done
  done
}
task_prof_step() {
  local tag=$1; shift
  rm -rf $OUT/prof_tmp
  local note="$* rocprofv3 --kernel-trace --stats -- python bench.py --full --no-cpu-baseline --no-batch-max --no-warp --no-shipped --no-fp32   (3 warm-up + 10 timed + 2 instrumented train_g_d steps = 15 steps; model build kernels included)"
  ( for v in "$@"; do export "$v"; done
    rocprofv3 --kernel-trace --stats -d $OUT/prof_tmp -o gan -- python bench.py --full --no-cpu-baseline --no-batch-max --no-warp --no-shipped --no-fp32 > $OUT/prof_$tag.log 2>&1 )
  python tools/rocpd_summary.py $OUT/prof_tmp/gan_results.db $OUT/${tag}_kernel_stats.csv "$note"
  python tools/step_trace.py $OUT/prof_tmp/gan_results.db $OUT/${tag}_per_step.csv 4 11 "$note"
  grep '^#' $OUT/${tag}_per_step.csv | cut -c1-200
  tail -1 $OUT/prof_$tag.log | cut -c1-400
  head -24 $OUT/${tag}_kernel_stats.csv | cut -c1-160; tail -1 $OUT/${tag}_kernel_stats.csv
  rm -rf $OUT/prof_tmp
}
task_prof_warp() {
  local tag=$1; shift
  for v in "$@"; do export "$v"; done
  for d in random room; do
    rm -rf $OUT/prof_tmp
    rocprofv3 --kernel-trace --stats -d $OUT/prof_tmp -o warp -- python bench.py --full --workload warp --warp-height ${WARP_H:-1024} --warp-depth $d --steps 200 --warmup 20 --no-cpu-baseline > /dev/null 2>&1
    python tools/rocpd_summary.py $OUT/prof_tmp/warp_results.db $OUT/${tag}_warp_${d}_kernel_stats.csv "rocprofv3 --kernel-trace --stats -- python bench.py --full --workload warp --warp-height ${WARP_H:-1024} --warp-depth $d --steps 200 --warmup 20 --no-cpu-baseline"
    head -9 $OUT/${tag}_warp_${d}_kernel_stats.csv | cut -c1-150
  done
  rm -rf $OUT/prof_tmp
}
task_pmc_conv() {
  local tag=$1 shape="$2"
  local st=$(echo $shape | tr ' ' '_')
  rm -rf $OUT/pmc_tmp_*
  rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d $OUT/pmc_tmp_a -o pmc -- python tools/one_conv.py $shape > /dev/null 2>&1
  rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_tmp_f -o pmc -- python tools/one_conv.py $shape > /dev/null 2>&1
  rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_tmp_w -o pmc -- python tools/one_conv.py $shape > /dev/null 2>&1
  python tools/pmc_summary.py $OUT/${tag}_conv_pmc_$st.json --source=se3ds_amd/csrc/conv.hip "$OUT/pmc_tmp_a/*.db" "$OUT/pmc_tmp_f/*.db" "$OUT/pmc_tmp_w/*.db" 'igemm|wgrad'
  rm -rf $OUT/pmc_tmp_*
}
task_pmc_warp() {
  local tag=$1
  rm -rf $OUT/pmc_tmp_*
  rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_tmp_f -o pmc -- python bench.py --full --workload warp --steps 20 --warmup 3 --no-cpu-baseline > /dev/null 2>&1
  rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_tmp_w -o pmc -- python bench.py --full --workload warp --steps 20 --warmup 3 --no-cpu-baseline > /dev/null 2>&1
  python tools/pmc_summary.py $OUT/${tag}_warp_pmc.json --source=se3ds_amd/csrc/geom.hip "$OUT/pmc_tmp_f/*.db" "$OUT/pmc_tmp_w/*.db" 'splat|unproject'
  rm -rf $OUT/pmc_tmp_*
}
task_pmc_warp_valu() {
  # VALU / LDS counters of the warp kernels (one pass): is the splat VALU-bound?
  local tag=$1
  rm -rf $OUT/pmc_tmp_v
  rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE -d $OUT/pmc_tmp_v -o pmc -- python bench.py --full --workload warp --steps 20 --warmup 3 --no-cpu-baseline > /dev/null 2>&1
  python tools/pmc_summary.py $OUT/${tag}_warp_valu_pmc.json --source=se3ds_amd/csrc/geom.hip "$OUT/pmc_tmp_v/*.db" 'splat|unproject'
  rm -rf $OUT/pmc_tmp_v
}
task_pmc_step() {
  local tag=$1; shift
  rm -rf $OUT/pmc_tmp_s
  ( for v in "$@"; do export "$v"; done
    rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE -d $OUT/pmc_tmp_s -o pmc -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-batch-max --no-warp --no-shipped --no-fp32 > $OUT/pmc_step_$tag.log 2>&1 )
  tail -1 $OUT/pmc_step_$tag.log | cut -c1-300
  python tools/pmc_step.py "$OUT/pmc_tmp_s/*.db" $OUT/${tag}_step_pmc.json 40
  rm -rf $OUT/pmc_tmp_s
}
task_prof_py() {
  local tag=$1; shift
  rm -rf $OUT/prof_tmp
  rocprofv3 --kernel-trace --stats -d $OUT/prof_tmp -o run -- python "$@" > $OUT/prof_$tag.log 2>&1
  python tools/rocpd_summary.py $OUT/prof_tmp/run_results.db $OUT/${tag}_kernel_stats.csv "rocprofv3 --kernel-trace --stats -- python $*"
  head -${PROF_HEAD:-16} $OUT/${tag}_kernel_stats.csv | cut -c1-160
  rm -rf $OUT/prof_tmp
}
task_pmc_py() {
  local tag=$1 pmc="$2" re="$3"; shift; shift; shift
  rm -rf $OUT/pmc_tmp_g
  rocprofv3 --kernel-trace --pmc $pmc -d $OUT/pmc_tmp_g -o pmc -- python "$@" > /dev/null 2>&1
  python tools/pmc_summary.py $OUT/${tag}_pmc.json "$OUT/pmc_tmp_g/*.db" "$re"
  python - $OUT/${tag}_pmc.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
for k, v in d.items():
  if k.startswith('_'): continue
  print(k[:60], ' '.join('%s=%.4g' % (a, (b['avg'] if isinstance(b, dict) and 'avg' in b else b)) for a, b in v.items() if not isinstance(b, dict) or 'avg' in b))
PY
  rm -rf $OUT/pmc_tmp_g
}
task_video_input() {
  timeout 600 python tools/video_input_bench.py --out $OUT/video_input_bench.json "$@" > $OUT/video_input_bench.log 2>&1
  echo "video_input rc=$?"; grep -v '^{' $OUT/video_input_bench.log | tail -9 | cut -c1-300
}
task_py() { timeout 1500 python "$@"; }
args=()
run_task() { if [ ${#args[@]} -gt 0 ]; then local t=${args[0]}; echo "##### $t ${args[*]:1}"; "task_$t" "${args[@]:1}"; fi; args=(); }
for a in "$@"; do
  if [ "$a" == "--" ]; then run_task; else args+=("$a"); fi
done
run_task
du -sh $OUT | cut -c1-40
