# rate of the split 10^3 layer under the knobs given as arguments:  gpurun -- 'bash tools/jobs/wfs_var.sh TH_WF_DBG=64 TH_WF_DBG=128'
mkdir -p gpurun_out/wfs
# TH_*_DBG rows run on the knock-out library (tools/build_knockouts.py; results wrong by design), every other row on the product
KNOCK=$(python tools/build_knockouts.py | grep '^TIMED_HIP_LIB=') || exit 1
for v in "TH_WF_SPLIT=1" "$@"; do
  echo "== $v"; case "$v" in *_DBG=*) lib=$KNOCK ;; *) lib= ;; esac; env $lib $v TH_GUARD=0 timeout 120 python tools/bench_layer.py 10 32 64 3 8192 1 2>&1 | grep -o '"ms_per_4096": [0-9.]*' | tr '\n' ' '; echo
done 2>&1 | tee -a gpurun_out/wfs/layer_rate_var.txt
