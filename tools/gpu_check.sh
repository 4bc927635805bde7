#!/bin/bash
# Run on the GPU box: kernel unit tests, parity tests, smoke, bench (+ optional profile).
# Everything is logged under $LOGS (default logs/ in the repository root).
LOGS=${LOGS:-logs}
mkdir -p $LOGS
export PYTHONUNBUFFERED=1
STAGE=${1:-all}
if [ "$STAGE" = "all" ] || [ "$STAGE" = "tests" ]; then
  timeout 900 python -m pytest tests/test_gpu_kernels.py -m gpu -q -s -p no:cacheprovider > $LOGS/kernels.log 2>&1
  echo "kernels exit $?" | tee -a $LOGS/summary.txt
  timeout -k 10 900 python -m pytest tests/test_gpu_block_kernels.py -m gpu -q -s -p no:cacheprovider > $LOGS/block_kernels.log 2>&1
  rc=$?
  echo "block kernels exit $rc" | tee -a $LOGS/summary.txt
  # a time limit, an abort or a segmentation fault in a kernel test: nothing more is started on this card
  case $rc in 124|134|137|139) echo "stopping: see $LOGS/block_kernels.log" | tee -a $LOGS/summary.txt; exit $rc ;; esac
  timeout -k 10 600 python -m pytest tests/test_gpu_wgrad_kernels.py -m gpu -q -s -p no:cacheprovider > $LOGS/wgrad_kernels.log 2>&1
  rc=$?
  echo "wgrad kernels exit $rc" | tee -a $LOGS/summary.txt
  case $rc in 124|134|137|139) echo "stopping: see $LOGS/wgrad_kernels.log" | tee -a $LOGS/summary.txt; exit $rc ;; esac
  timeout 1200 python -m pytest tests/test_gpu_parity.py -m gpu -q -s -p no:cacheprovider > $LOGS/parity.log 2>&1
  echo "parity exit $?" | tee -a $LOGS/summary.txt
  timeout -k 10 900 python -m pytest tests/test_gpu_decode_cond.py -m gpu -q -s -p no:cacheprovider > $LOGS/decode_cond.log 2>&1
  rc=$?
  echo "conditioned decode exit $rc" | tee -a $LOGS/summary.txt
  case $rc in 124|134|137|139) echo "stopping: see $LOGS/decode_cond.log" | tee -a $LOGS/summary.txt; exit $rc ;; esac
  timeout 600 python __graft_entry__.py smoke > $LOGS/smoke.log 2>&1
  echo "smoke exit $?" | tee -a $LOGS/summary.txt
fi
if [ "$STAGE" = "all" ] || [ "$STAGE" = "bench" ]; then
  timeout 900 python bench.py --steps 10 --warmup 3 --full --phases > $LOGS/bench.log 2> $LOGS/bench.err
  echo "bench exit $?" | tee -a $LOGS/summary.txt
fi
tail -n 60 $LOGS/kernels.log $LOGS/block_kernels.log $LOGS/wgrad_kernels.log $LOGS/parity.log $LOGS/smoke.log $LOGS/bench.log $LOGS/bench.err 2>/dev/null | tail -n 150
if [ "$STAGE" = "all" ] || [ "$STAGE" = "prof" ]; then
  REPO=$(pwd)
  case $LOGS in /*) L=$LOGS ;; *) L=$REPO/$LOGS ;; esac
  export TMPDIR=/tmp
  rm -rf $LOGS/prof $LOGS/pmc_fetch $LOGS/pmc_write
  # --full: the profiled command is the whole line's (tools/prof_summary.py counts its phase-table and per-kernel steps)
  (cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $L/prof -- python3 $REPO/bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-extras > $L/prof.log 2>&1)
  echo "prof exit $?" | tee -a $LOGS/summary.txt
  (cd /tmp && timeout 900 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $L/pmc_fetch -- python3 $REPO/bench.py --steps 2 --warmup 1 --settle 0 --full --no-cpu-baseline --no-extras > $L/pmc_fetch.log 2>&1)
  echo "pmc fetch exit $?" | tee -a $LOGS/summary.txt
  (cd /tmp && timeout 900 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $L/pmc_write -- python3 $REPO/bench.py --steps 2 --warmup 1 --settle 0 --full --no-cpu-baseline --no-extras > $L/pmc_write.log 2>&1)
  echo "pmc write exit $?" | tee -a $LOGS/summary.txt
  # config 4's stack kernels (conditioned decoder blocks, encoder blocks): the same two passes over its step
  rm -rf $LOGS/pmc_fetch_ae $LOGS/pmc_write_ae
  (cd /tmp && timeout 900 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $L/pmc_fetch_ae -- python3 $REPO/tools/ae_phases.py > $L/pmc_fetch_ae.log 2>&1)
  echo "pmc fetch (config 4) exit $?" | tee -a $LOGS/summary.txt
  (cd /tmp && timeout 900 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $L/pmc_write_ae -- python3 $REPO/tools/ae_phases.py > $L/pmc_write_ae.log 2>&1)
  echo "pmc write (config 4) exit $?" | tee -a $LOGS/summary.txt
  python3 tools/prof_summary.py $LOGS > $LOGS/prof_summary.md 2>&1
  # keep only the small files (the raw traces can be large)
  find $LOGS/prof $LOGS/pmc_fetch $LOGS/pmc_write $LOGS/pmc_fetch_ae $LOGS/pmc_write_ae -type f -size +3M -delete 2>/dev/null
  cat $LOGS/prof_summary.md | head -60
fi
