#!/bin/bash
# full verification of the tree on one GPU: the GPU test suite, smoke(), the headline bench with its self-check
# logs go to $LWC_OUT (default: out/ in the repository root)
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${LWC_OUT:-out}
mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 900 python -u -m pytest tests/ -x -q -m gpu --timeout 120 --timeout-method thread \
  > "$OUT/suite.log" 2>&1 || { tail -30 "$OUT/suite.log"; exit 1; }
tail -2 "$OUT/suite.log"
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('SMOKE OK')" > "$OUT/smoke.log" 2>&1 \
  || { tail -30 "$OUT/smoke.log"; exit 1; }
tail -1 "$OUT/smoke.log"
timeout -k 10 600 python -u bench.py --gpus 1 --steps 20 --warmup 5 --full > "$OUT/bench.log" 2>&1 \
  || { tail -30 "$OUT/bench.log"; exit 1; }
grep '"metric"' "$OUT/bench.log"
