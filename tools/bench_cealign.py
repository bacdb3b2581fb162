"""Rate of th_cealign (analyse_models.py --cealign) on N pairs of L positions in ONE submission: (a) the four kernels alone (events
inside the call), (b) the call on flat arrays (compaction on the host, device allocation and copies included) — by default for 1000
pairs of 76 and for 100 pairs of 300.  A pair is a random-walk chain against a copy in another frame with sigma = 0.3 Angstrom noise
that lacks six residues in the middle.  Beside each: the NumPy restatement (tests/cealign_restatement.py) on THIS host on
--numpy-pairs of the pairs, scaled to all; the GPU's counts and alignments of those pairs are checked against it.

    python tools/bench_cealign.py [--shapes 1000x76 100x300] [--reps 3] [--numpy-pairs 1]

One JSON line per shape.  No rate is a pass condition."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def chain_pair(length, rng, rotation):
    steps = rng.normal(size=(length, 3))
    steps *= 3.8 / np.linalg.norm(steps, axis=1, keepdims=True)
    ref = np.cumsum(steps, axis=0)
    cut = length // 2
    model = np.concatenate([ref[:cut - 3], ref[cut + 3:]]) + rng.normal(0, 0.3, (length - 6, 3))
    return ref, model @ rotation(rng).T + rng.uniform(-30, 30, 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", type=str, nargs="+", default=["1000x76", "100x300"], help="PAIRSxPOSITIONS")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--numpy-pairs", type=int, default=1)
    a = ap.parse_args()
    import cealign_restatement as cr
    import superpose_restatement as sr
    from timed_hip import cealign
    for shape in a.shapes:
        n, length = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(0)
        distinct = [chain_pair(length, rng, sr.rotation) for _ in range(min(n, 32))]      # 32 different pairs, repeated: the kernel cannot tell
        pairs = [distinct[k % len(distinct)] for k in range(n)]
        ref, ro, mob, mo = cr.flatten(pairs)
        cealign.cealign_arrays(ref[:ro[1]], ro[:2], mob[:mo[1]], mo[:2], device=a.device)                    # warm-up: module load
        walls, kernels = [], []
        for _ in range(a.reps):
            timing = {}
            t0 = time.perf_counter()
            got = cealign.cealign_arrays(ref, ro, mob, mo, device=a.device, timing=timing)
            walls.append(time.perf_counter() - t0)
            kernels.append(timing["kernel_ms"] / 1e3)
        m = max(0, min(a.numpy_pairs, n))
        t0 = time.perf_counter()
        host = [cr.restate(r, q) for r, q in pairs[:m]]
        numpy_s = (time.perf_counter() - t0) / m * n if m else None
        agree = all(np.array_equal(got.counts[k], h["counts"]) and np.array_equal(got.align[ro[k]:ro[k + 1]], h["align"]) for k, h in enumerate(host))
        kernel, wall = float(np.median(kernels)), float(np.median(walls))
        starts = int(got.counts[:, 2].sum())
        print(json.dumps({"pairs": n, "positions": length, "model_positions": length - 6, "window_pairs": int((length - 7) * (length - 13)) * n,
                          "starts": starts, "afps_mean": float(got.counts[:, 3].mean()), "aligned_mean": float(got.counts[:, 4].mean()),
                          "rmsd_mean": float(np.nanmean(got.scores[:, 0])), "kernel_ms": kernel * 1e3, "call_ms": wall * 1e3,
                          "pairs_per_s_kernel": n / kernel, "pairs_per_s_call": n / wall, "starts_per_s_kernel": starts / kernel,
                          "numpy_s_scaled": numpy_s, "numpy_pairs": m, "agrees_with_numpy": bool(agree), "reps": a.reps}))


if __name__ == "__main__":
    main()
