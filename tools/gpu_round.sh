#!/bin/bash
# One GPU-box session.  Usage (from the repo root on the GPU box): bash tools/gpu_round.sh <tag> [steps...]
# steps (default: all): smoke tests gemm bench sweep prof pmc
# Every step runs under its own `timeout`, so a hung kernel cannot eat the whole box allowance.
TAG=${1:-r01}; shift
STEPS=${*:-smoke tests gemm bench sweep prof pmc}
OUT=gpurun_out/$TAG
mkdir -p $OUT
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$(pwd)}
has() { [[ " $STEPS " == *" $1 "* ]]; }
echo "== rocminfo =="; /opt/rocm/bin/rocminfo 2>/dev/null | grep -E "Marketing Name|gfx9|Compute Unit" | head -4; nproc

if has smoke; then
  echo "== smoke =="; timeout 600 python __graft_entry__.py smoke 2>&1 | tail -5
fi
if has pair; then
  echo "== pair kernel: occupancy, bit-identity tests, same-process A/B =="
  python - <<'PY'
from tokenpacker_amd import _capi
print("pair kernel workgroups per CU (needs 2):", _capi.load_test_library().tp_test_pair_occupancy())
PY
  timeout 900 python -m pytest tests/test_gpu_pair.py -m gpu -x -q -p no:cacheprovider > $OUT/pytest_pair.log 2>&1
  echo "pytest exit $?"; tail -30 $OUT/pytest_pair.log
  timeout 600 python tools/pair_ab.py --batches 256 128 64 32 --out $OUT/pair_ab.json > $OUT/pair_ab.log 2>&1; echo "pair_ab exit $?"; cat $OUT/pair_ab.log | cut -c1-600
fi
if has ktests; then
  echo "== pytest gpu (kernels only) =="
  timeout 900 python -m pytest tests/test_gpu_kernels.py -m gpu -x -q -p no:cacheprovider > $OUT/pytest_kernels.log 2>&1
  echo "pytest exit $?"; tail -25 $OUT/pytest_kernels.log
fi
if has tests; then
  echo "== pytest gpu =="
  # (exactly the driver's command plus the 25 slowest tests: the whole suite must stay far below the driver's 1200 s limit — VERDICT r4)
  T0=$(date +%s); timeout 1500 python -m pytest tests -m gpu -q -s -p no:cacheprovider --durations=25 > $OUT/pytest_gpu.log 2>&1
  echo "pytest exit $? wall $(( $(date +%s) - T0 )) s"; grep -E "passed|failed|error" $OUT/pytest_gpu.log | tail -5; grep -E "^\[parity\]|^\[eager|^\[e2e\]|^\[adv\]|^\[grad\].*worst" $OUT/pytest_gpu.log | tail -120; grep -E "^(FAILED|ERROR)" $OUT/pytest_gpu.log | head -40
  cp gpurun_out/eager_rocm_s*.json $OUT/ 2>/dev/null
fi
if has gemm; then
  echo "== gemm bench =="; timeout 600 python tools/gemm_bench.py --out $OUT/gemm_bench.json > $OUT/gemm_bench.log 2>&1; echo "exit $?"; tail -30 $OUT/gemm_bench.log
fi
if has kfit; then
  echo "== per-tile fixed cost fit =="; timeout 600 python tools/ktile_fit.py > $OUT/ktile_fit.txt 2>&1; echo "exit $?"; cat $OUT/ktile_fit.txt
fi
if has btests; then
  echo "== pytest gpu (backward only) =="
  timeout 900 python -m pytest tests/test_gpu_backward.py -m gpu -x -q -s -p no:cacheprovider > $OUT/pytest_bwd.log 2>&1
  echo "pytest exit $?"; tail -8 $OUT/pytest_bwd.log
fi
if has train; then
  echo "== train bench =="; timeout 900 python tools/train_bench.py --out $OUT/train_bench.json > $OUT/train_bench.log 2>&1; echo "exit $?"; tail -6 $OUT/train_bench.log
fi
if has trainprof; then
  echo "== rocprof kernel trace of the training step =="
  ( cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/rocprof_train -o train -- python $R/tools/train_bench.py --batches 256 --hip-only --out $R/$OUT/train_bench_prof.json > $R/$OUT/rocprof_train.log 2>&1 ); echo "rocprof exit $?"
  F=$(find $OUT/rocprof_train -name "*kernel_stats.csv" | head -1); [ -n "$F" ] && head -16 "$F" | cut -c1-200
  find $OUT/rocprof_train -name "*kernel_trace.csv" -size +20M -delete
fi
if has bench; then
  echo "== bench =="; timeout 600 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; echo "bench exit $?"; cat $OUT/bench.json; tail -5 $OUT/bench.err
fi
if has sweep; then
  echo "== sweep (scale_factor 3, 4; HD 36 crops/GPU; fp16) =="
  for sf in 3 4; do timeout 300 python bench.py --full --scale-factor $sf --no-cpu-baseline --no-extras > $OUT/bench_s$sf.json 2>> $OUT/bench.err; cat $OUT/bench_s$sf.json; done
  timeout 300 python bench.py --full --batch 36 --no-cpu-baseline --no-extras > $OUT/bench_hd36.json 2>> $OUT/bench.err; cat $OUT/bench_hd36.json
  timeout 300 python bench.py --full --dtype fp16 --no-cpu-baseline --no-extras > $OUT/bench_fp16.json 2>> $OUT/bench.err; cat $OUT/bench_fp16.json
fi
if has small; then
  echo "== small batches (strong-scaling shards: 256/8 = 32 images, B = 1, 8, 64, 128) and the HD workload on one GPU =="
  for b in 1 8 10 32 64 128; do timeout 300 python bench.py --full --batch $b --no-cpu-baseline --no-extras --steps 100 --warmup 20 > $OUT/bench_b$b.json 2>> $OUT/bench.err; python - "$OUT/bench_b$b.json" <<'PY'
import json,sys
d=json.load(open(sys.argv[1])); print("B=%d: %.1f img/s  %.4f ms/step  whole-path %.0f TFLOP/s" % (d["config"]["global_batch"], d["value"], d["ms_per_step"], d["whole_path"]["achieved_tflops"]))
PY
  done
  timeout 300 python bench.py --full --hd --no-cpu-baseline > $OUT/bench_hd288.json 2>> $OUT/bench.err; cat $OUT/bench_hd288.json
fi
if has absorb; then
  echo "== absorbed K/V schedule A/B (s = 2 forced on; s = 3, 4 forced off) =="
  timeout 300 python bench.py --full --tune ABSORB_KV=2 --no-cpu-baseline > $OUT/bench_s2_absorb.json 2>> $OUT/bench.err; cat $OUT/bench_s2_absorb.json
  for sf in 3 4; do timeout 300 python bench.py --full --scale-factor $sf --tune ABSORB_KV=1 --no-cpu-baseline > $OUT/bench_s${sf}_plain.json 2>> $OUT/bench.err; cat $OUT/bench_s${sf}_plain.json; done
fi
if has e2e; then
  echo "== encode_images + 7B-shaped prefill (BASELINE configs[4], B=64 on one GPU) =="
  timeout 600 python bench.py --full --e2e --steps 5 --warmup 2 > $OUT/bench_e2e.json 2>> $OUT/bench.err; cat $OUT/bench_e2e.json; tail -3 $OUT/bench.err
fi
if has prof; then
  echo "== rocprof kernel trace =="
  ( cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/rocprof -o bench -- python $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extras --min-seconds 0 > $R/$OUT/rocprof_bench.log 2>&1 ); echo "rocprof exit $?"
  F=$(find $OUT/rocprof -name "*kernel_stats.csv" | head -1); [ -n "$F" ] && head -16 "$F"
  find $OUT/rocprof -name "*kernel_trace.csv" -size +20M -delete
fi
if has prof3; then
  echo "== rocprof kernel trace, scale_factor 3 (absorbed K/V schedule) =="
  ( cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/rocprof_s3 -o bench -- python $R/bench.py --full --scale-factor 3 --steps 10 --warmup 3 --no-cpu-baseline --no-extras --min-seconds 0 > $R/$OUT/rocprof_bench_s3.log 2>&1 ); echo "rocprof exit $?"
  F=$(find $OUT/rocprof_s3 -name "*kernel_stats.csv" | head -1); [ -n "$F" ] && head -16 "$F" | cut -c1-220
  find $OUT/rocprof_s3 -name "*kernel_trace.csv" -size +20M -delete
  for C in "FETCH_SIZE" "WRITE_SIZE"; do
    ( cd /tmp && timeout 600 rocprofv3 --kernel-trace --pmc $C --output-format csv -d $R/$OUT/pmc3_$C -o pmc -- python $R/bench.py --full --scale-factor 3 --steps 3 --warmup 2 --no-cpu-baseline --no-extras --min-seconds 0 > $R/$OUT/pmc3_$C.log 2>&1 ); echo "pmc3 $C exit $?"
  done
  mkdir -p $OUT/s3 && for C in FETCH_SIZE WRITE_SIZE; do mv $OUT/pmc3_$C $OUT/s3/pmc_$C; done
  python tools/pmc_summary.py $OUT/s3 > $OUT/pmc_summary_s3.json 2> $OUT/pmc_summary.err; python - "$OUT/pmc_summary_s3.json" <<'PY'
import json,sys
d=json.load(open(sys.argv[1]))
for k,v in d.items():
    if "attention" in k: print(k, {x: v.get(x) for x in ("dispatches","duration_ns","hbm_read_bytes_corrected","hbm_write_bytes_uncalibrated")})
PY
  find $OUT -name "*kernel_trace.csv" -size +20M -delete
fi
if has pmc; then
  echo "== rocprof PMC passes (own runs, kernel-trace only) =="
  for C in "FETCH_SIZE" "WRITE_SIZE" "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"; do
    N=$(echo $C | tr ' ' '_' | cut -c1-24)
    ( cd /tmp && timeout 600 rocprofv3 --kernel-trace --pmc $C --output-format csv -d $R/$OUT/pmc_$N -o pmc -- python $R/bench.py --full --steps 3 --warmup 2 --no-cpu-baseline --no-extras --min-seconds 0 > $R/$OUT/pmc_$N.log 2>&1 ); echo "pmc $N exit $?"
  done
  python tools/pmc_summary.py $OUT > $OUT/pmc_summary.json 2> $OUT/pmc_summary.err; cat $OUT/pmc_summary.json | head -60; tail -3 $OUT/pmc_summary.err
  python tools/make_traffic.py $OUT/pmc_summary.json $TAG && cp profiles/traffic.json $OUT/traffic.json
  find $OUT -name "*kernel_trace.csv" -size +20M -delete
fi
if has gemmpmc; then
  echo "== GEMM variants under PMC (two passes) =="
  i=0
  for C in "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE" \
           "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_INST_CYCLES_VMEM SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_MFMA GRBM_GUI_ACTIVE"; do
    i=$((i+1))
    ( cd /tmp && timeout 600 rocprofv3 --kernel-trace --pmc $C --output-format csv -d $R/$OUT/pmc_gemm$i -o pmc -- python $R/tools/gemm_bench.py --rounds 1 --iters 2 --out $R/$OUT/gemm_bench_pmc.json > $R/$OUT/pmc_gemm$i.log 2>&1 ); echo "pmc gemm pass $i exit $?"
  done
  python tools/pmc_summary.py $OUT --all > $OUT/pmc_gemm_summary.json 2> $OUT/pmc_summary.err; tail -3 $OUT/pmc_summary.err
  find $OUT -name "*kernel_trace.csv" -size +20M -delete
fi
du -sh $OUT
