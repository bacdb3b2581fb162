"""Rate of th_tmscore (analyse_models.py --tmscore) on N pairs of L positions in ONE submission — a sampling campaign scored against
its natives is this shape: (a) the two kernels alone (events inside the call), (b) the call on flat arrays (compaction on the host,
device allocation and copies included) — for 10 000 pairs of 300 and for a batch of 76-position pairs.  Beside each: th_superpose's
kernel time on the same batch with cycles = 0, the yardstick of "one fit per pair", and the NumPy restatement
(tests/tmscore_restatement.py) on THIS host on --numpy-pairs of the pairs, scaled to all; the GPU's counts of those pairs are checked
against it.

    python tools/bench_tmscore.py [--pairs 10000] [--lengths 300 76] [--reps 3] [--numpy-pairs 2] [--rounds 20]

One JSON line per length.  No rate is a pass condition."""
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
    ap.add_argument("--lengths", type=int, nargs="+", default=[300, 76])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--numpy-pairs", type=int, default=2)
    a = ap.parse_args()
    import superpose_restatement as sr
    import tmscore_restatement as tr
    from timed_hip import superpose, tmscore
    for length in a.lengths:
        rng = np.random.default_rng(0)
        n = a.pairs
        distinct = [sr.synthetic_pair(length, rng) for _ in range(min(n, 64))]     # 64 different pairs, repeated: the kernel cannot tell
        pairs = [distinct[k % len(distinct)] for k in range(n)]
        ref, mob, offsets = sr.flatten(pairs)

        tmscore.tmscore_arrays(ref[:2 * length], mob[:2 * length], offsets[:3], rounds=a.rounds, device=a.device)     # warm-up: module load
        walls, kernels = [], []
        for _ in range(a.reps):
            timing = {}
            t0 = time.perf_counter()
            got = tmscore.tmscore_arrays(ref, mob, offsets, rounds=a.rounds, device=a.device, timing=timing)
            walls.append(time.perf_counter() - t0)
            kernels.append(timing["kernel_ms"] / 1e3)
        one_fit = []
        for _ in range(a.reps):
            timing = {}
            superpose.superpose_arrays(ref, mob, offsets, cycles=0, device=a.device, timing=timing)
            one_fit.append(timing["kernel_ms"] / 1e3)

        m = max(0, min(a.numpy_pairs, n))
        t0 = time.perf_counter()
        host = [tr.restate(r, q, rounds=a.rounds) for r, q in pairs[:m]]
        numpy_s = (time.perf_counter() - t0) / m * n if m else None
        for k, h in enumerate(host):
            assert got.counts[k].tolist() == h["counts"].tolist() and abs(got.tm[k, 0] - float(h["tm"])) < 1e-12, (k, got.counts[k], h["counts"])

        wall, kern, fit = float(np.median(walls)), float(np.median(kernels)), float(np.median(one_fit))
        seeds, fits = int(got.counts[:, 2].sum()), int(got.counts[:, 3].sum())
        print(json.dumps(dict(what=f"{n} pairs of {length} positions, rounds={a.rounds}", pairs=n, positions=n * length, submissions=1, reps=a.reps,
                              seeds=seeds, fits_made=fits, fits_per_pair=round(fits / n, 1), tm_mean=round(float(got.tm[:, 0].mean()), 4),
                              kernel_ms_median=round(kern * 1e3, 3), kernel_ms_min=round(min(kernels) * 1e3, 3), call_ms_median=round(wall * 1e3, 3),
                              call_ms_min=round(min(walls) * 1e3, 3), pairs_per_s_kernel=float(f"{n / kern:.4g}"), pairs_per_s_call=float(f"{n / wall:.4g}"),
                              fits_per_s_kernel=float(f"{fits / kern:.4g}"), superpose_cycles0_kernel_ms=round(fit * 1e3, 3),
                              superpose_fits_per_s_kernel=float(f"{n / fit:.4g}"), numpy_restatement_s_scaled=None if numpy_s is None else round(numpy_s, 1),
                              numpy_pairs_timed=m, checked_against_numpy=m > 0,
                              ratio_numpy_over_call=None if numpy_s is None else round(numpy_s / wall, 1))), flush=True)


if __name__ == "__main__":
    main()
