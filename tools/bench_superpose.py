"""Rate of th_superpose (analyse_models.py) on N pairs of L positions in ONE submission — models x temperatures x samples x AlphaFold2
outputs against their natives are this shape: (a) the kernel alone (events inside the call), (b) the call on flat arrays (device
allocation and copies included) — and beside them a NumPy loop on THIS host that does the cycle-0 fit alone, one np.linalg.svd
Kabsch per pair (on --numpy-pairs of them, scaled to all: its cost per pair is constant; the GPU figure includes up to --cycles
refinement fits per pair, the NumPy one none).  rmsd_fit_all of the pairs the NumPy loop covers is checked against it.

    python tools/bench_superpose.py [--pairs 10000] [--length 300] [--reps 5] [--numpy-pairs 500]

One JSON line.  No rate is a pass condition."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--numpy-pairs", type=int, default=500)
    a = ap.parse_args()
    import superpose_restatement as sr
    from timed_hip import superpose
    rng = np.random.default_rng(0)
    n, length = a.pairs, a.length
    distinct = [sr.synthetic_pair(length, rng) for _ in range(min(n, 64))]         # 64 different pairs, repeated: the kernel cannot tell
    pairs = [distinct[k % len(distinct)] for k in range(n)]
    ref, mob, offsets = sr.flatten(pairs)

    superpose.superpose_arrays(ref[:2 * length], mob[:2 * length], offsets[:3], cycles=a.cycles, device=a.device)   # warm-up: module load
    walls, kernels = [], []
    for _ in range(a.reps):
        timing = {}
        t0 = time.perf_counter()
        got = superpose.superpose_arrays(ref, mob, offsets, cycles=a.cycles, device=a.device, timing=timing)
        walls.append(time.perf_counter() - t0)
        kernels.append(timing["kernel_ms"] / 1e3)

    m = max(1, min(a.numpy_pairs, n))
    t0 = time.perf_counter()
    host = [sr.kabsch_rmsd(r, q) for r, q in pairs[:m]]
    numpy_s = (time.perf_counter() - t0) / m * n
    assert np.abs(got.rmsd[:m, 2] - np.array(host)).max() < 1e-9

    wall, kern = float(np.median(walls)), float(np.median(kernels))
    fits = int(n + got.counts[:, 2].sum())
    print(json.dumps(dict(what=f"{n} pairs of {length} positions, cycles={a.cycles}", pairs=n, positions=n * length, submissions=1, reps=a.reps,
                          fits_made=fits, kernel_s_median=round(kern, 6), kernel_s_min=round(min(kernels), 6), call_s_median=round(wall, 6),
                          call_s_min=round(min(walls), 6), pairs_per_s_kernel=float(f"{n / kern:.4g}") if kern > 0 else None,
                          pairs_per_s_call=float(f"{n / wall:.4g}"), numpy_svd_loop_s_scaled=round(numpy_s, 3), numpy_pairs_timed=m,
                          ratio_numpy_over_call=round(numpy_s / wall, 1))), flush=True)


if __name__ == "__main__":
    main()
