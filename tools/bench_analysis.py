"""Rate of th_analyse_probs (predict.py --output_analysis) and th_analyse_classes (analyse_rotamers.py, predict.py --output_auc;
with and without the AUC sweep): wall time of the call on 1 M x 338 and 1 M x 20 float16 matrices (host arrays, staged in blocks),
and the wall time --output_analysis adds to a predict.py run of a synthetic TIMED model over a uint8 frame pack.

    python tools/bench_analysis.py [--rows 1000000] [--reps 5] [--predict-frames 100000] [--kernel-stats kernel_stats.csv]

The kernel's own time comes from a profiler run of this script (rocprofv3 --kernel-trace --stats -- python tools/bench_analysis.py
--predict-frames 0): pass the kernel_stats.csv it writes to --kernel-stats and the k_analyse, k_class_rows and k_pair_sweep rows are
reported as GB/s of matrix read, the other kernels of th_analyse_classes (the radix sort, k_positives) as time per call.  One JSON
line per measurement."""
import argparse
import csv
import json
import os
import sys
import tempfile
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _matrix(rng, n, k):
    out = np.empty((n, k), np.float16)
    for lo in range(0, n, 65536):
        z = rng.standard_normal((min(65536, n - lo), k)).astype(np.float32) * 2.5
        p = np.exp(z - z.max(axis=1, keepdims=True))
        out[lo:lo + len(z)] = p / p.sum(axis=1, keepdims=True)
    return out


def bench_call(n, reps, device, ks=(338, 20)):
    from design_utils import utils
    from timed_hip import analysis
    rng = np.random.default_rng(0)
    rows = []
    for k in ks:
        x = _matrix(rng, n, k)
        t = rng.integers(0, 20, n).astype(np.int8)
        col = analysis.rotamer_columns(utils.get_rotamer_codec()[1]) if k == 338 else analysis.identity_columns()
        analysis.analyse_probs(x, t, col, device=device)              # warm-up (module load, first allocations)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            analysis.analyse_probs(x, t, col, device=device)
            times.append(time.perf_counter() - t0)
        best = min(times)
        rows.append(dict(what="th_analyse_probs", n=n, k=k, dtype="f16", best_s=round(best, 5), median_s=round(float(np.median(times)), 5),
                         host_GBps=round(x.nbytes / best / 1e9, 2)))
        print(json.dumps(rows[-1]), flush=True)
        tc = rng.integers(0, k, n).astype(np.int16)
        for auc in (False, True):
            analysis.analyse_classes(x, tc, device=device, auc=auc)      # warm-up
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                analysis.analyse_classes(x, tc, device=device, auc=auc)
                times.append(time.perf_counter() - t0)
            best = min(times)
            rows.append(dict(what="th_analyse_classes", pair_u2=auc, n=n, k=k, dtype="f16", best_s=round(best, 5),
                             median_s=round(float(np.median(times)), 5), host_GBps=round(x.nbytes / best / 1e9, 2)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def bench_kernel_stats(path, rows, calls_per_k, ks=(338, 20)):
    """k_analyse rows of a rocprofv3 kernel_stats.csv (a run of this script with --predict-frames 0: ``calls_per_k`` calls of
    th_analyse_probs per k, warm-up included) -> kernel time per call and GB/s of matrix read.  k = 338 runs on the 64-lane
    instantiation, k = 20 on the 4-lane one."""
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "") or r.get("KernelName", "")
            launches, total_ns = int(r["Calls"]), float(r["TotalDurationNs"])
            if "k_analyse" in name or "k_class_rows" in name:
                # th_analyse_classes runs twice per k (without and with the AUC sweep), the row pass in both
                calls = calls_per_k * (2 if "k_class_rows" in name else 1)
                k = 338 if ("64>" in name or "Li64E" in name) else 20 if ("4>" in name or "Li4E" in name) else None
                per_call_s = total_ns / 1e9 / calls
                row = dict(what=("k_analyse" if "k_analyse" in name else "k_class_rows") + " kernel", name=name[:60], launches=launches,
                           kernel_ms_per_call=round(per_call_s * 1e3, 4))
                if k:
                    row.update(k=k, rows=rows, GBps=round(rows * k * 2 / per_call_s / 1e9, 1))
            elif "k_pair_sweep" in name:
                # one instantiation serves every k: the total is over the calls with the AUC sweep of all the matrices of the run
                # (profile one k at a time with --k to separate them)
                per_call_s = total_ns / 1e9 / calls_per_k
                row = dict(what="k_pair_sweep kernel", k=list(ks), name=name[:60], launches=launches,
                           kernel_ms_per_call=round(per_call_s * 1e3, 4), rows=rows,
                           GBps=round(rows * sum(ks) * 2 / per_call_s / 1e9, 1))
            elif "radix" in name or "onesweep" in name or "k_positives" in name or "histogram" in name:
                row = dict(what="sort step of th_analyse_classes", k=list(ks), name=name[:60], launches=launches,
                           kernel_ms_per_call=round(total_ns / 1e6 / calls_per_k, 4))
            else:
                continue
            print(json.dumps(row), flush=True)


def bench_predict(frames, device):
    import bench_legs
    import predict
    from design_utils import utils as du
    from timed_hip import pack, synth
    cfg, w = synth.timed_synth(20)
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        mp = d / "TIMED.pack"
        mp.write_bytes(pack.keras_to_pack(cfg, w))
        stem = str(d / "frames")
        bench_legs.make_frame_pack(stem, frames, gaussian=False)
        walls = {}
        for rep in range(2):
            for flag in (False, True):
                out = d / f"out_{int(flag)}_{rep}"
                out.mkdir()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    t0 = time.perf_counter()
                    predict.load_dataset_and_predict([mp], stem + ".framepack", batch_size=500, dataset_map_path=out / "datasetmap.txt",
                                                     path_to_output=out, device=device, output_analysis=flag)
                    walls.setdefault(flag, []).append(time.perf_counter() - t0)
        du.release_device_memory()
    off, on = min(walls[False]), min(walls[True])
    row = dict(what="predict.py --output_analysis", frames=frames, wall_s_without=round(off, 3), wall_s_with=round(on, 3),
               added_s=round(on - off, 3), added_pct=round(100 * (on - off) / off, 2))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--predict-frames", type=int, default=100_000)
    ap.add_argument("--k", type=int, nargs="+", default=[338, 20], help="column counts to measure (default: 338 20)")
    ap.add_argument("--kernel-stats", type=str, default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run")
    a = ap.parse_args()
    if a.kernel_stats:
        bench_kernel_stats(a.kernel_stats, a.rows, a.reps + 1, tuple(a.k))
        return
    bench_call(a.rows, a.reps, a.device, tuple(a.k))
    if a.predict_frames > 0:
        bench_predict(a.predict_frames, a.device)


if __name__ == "__main__":
    main()
