# conv_first5: parity tests, then the layer inside ProDCoNN-synth (+ knock-outs named on the command line)
#   gpurun --timeout 900 -- 'bash tools/jobs/first5.sh [TH_FIRST_DBG=1 ...]'
timeout 300 python -m pytest tests/test_gpu_conv_first5.py -q -x 2>&1 | tail -3
# TH_*_DBG rows run on the knock-out library (tools/build_knockouts.py; results wrong by design), every other row on the product
KNOCK=$(python tools/build_knockouts.py | grep '^TIMED_HIP_LIB=') || exit 1
for v in "" "$@"; do
  echo "VAR=$v"
  case "$v" in *_DBG=*) lib=$KNOCK ;; *) lib= ;; esac;
  env TH_GUARD=0 $lib $v timeout 200 python tools/plan_report.py --measure prodconn 2>/dev/null | grep -E "measured:|conv3d|dense"
done
