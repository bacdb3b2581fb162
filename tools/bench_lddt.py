"""Rate of th_lddt (analyse_models.py --lddt) on N pairs of L positions in ONE submission — models x temperatures x samples x AlphaFold2
outputs against their natives are this shape — and then on one very long pair: (a) the kernels alone (events inside the call), (b) the
call on flat arrays (device allocation and copies included), and the ordered pairs (i, j) of positions tested per second (L^2 per
pair; the model's distance is computed for the included ones only) — and beside them the NumPy restatement on THIS host, on
--numpy-pairs of the pairs, scaled to all (its cost per pair is constant).  The integers of the pairs the restatement covers are
checked against it when no decision of theirs sits within 1e-9 of a tie.

Two geometries, the extremes between which a protein lies: ``walk``, a random-walk chain of 3.8 Angstrom steps (neighbours along the
chain are neighbours in space, so the lanes of a wavefront agree about which j are included), and ``globule``, positions uniform in a
sphere at a protein's CA density in random order (compact, no agreement between lanes).

    python tools/bench_lddt.py [--pairs 10000] [--length 300] [--long 50000] [--reps 5] [--numpy-pairs 50]

One JSON line per run.  No rate is a pass condition."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def globule(n, rng):
    """n positions uniform in a sphere with one position per 140 cubic Angstrom, in random order, against a noisy rotated copy"""
    import superpose_restatement as sr
    radius = (n * 140.0 * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0)
    v = rng.normal(size=(n, 3))
    ref = v / np.linalg.norm(v, axis=1, keepdims=True) * radius * rng.random((n, 1)) ** (1.0 / 3.0)
    return ref, (ref + rng.normal(0, 1.0, (n, 3))) @ sr.rotation(rng).T + rng.uniform(-30, 30, 3)


def timed(lddt, ref, mob, offsets, a):
    walls, kernels = [], []
    for _ in range(a.reps):
        timing = {}
        t0 = time.perf_counter()
        got = lddt.lddt_arrays(ref, mob, offsets, radius=a.radius, device=a.device, timing=timing)
        walls.append(time.perf_counter() - t0)
        kernels.append(timing["kernel_ms"] / 1e3)
    return got, walls, kernels


def report(what, got, offsets, walls, kernels, a, **more):
    sizes = np.diff(offsets).astype(np.float64)
    tested = float((sizes * sizes).sum())
    wall, kern = float(np.median(walls)), float(np.median(kernels))
    print(json.dumps(dict(what=what, pairs=len(sizes), positions=int(sizes.sum()), radius=a.radius, submissions=1, reps=a.reps,
                          ordered_pairs_tested=tested, included_fraction=round(float(got.pair[:, 1].sum()) / tested, 4),
                          lddt_mean=round(float(np.nanmean([s[2:].sum() / (4.0 * s[1]) if s[1] else np.nan for s in got.pair.astype(np.float64)])), 4),
                          kernel_ms_median=round(kern * 1e3, 3), kernel_ms_min=round(min(kernels) * 1e3, 3), call_ms_median=round(wall * 1e3, 3),
                          call_ms_min=round(min(walls) * 1e3, 3), pair_distances_per_s_kernel=float(f"{tested / kern:.4g}") if kern > 0 else None,
                          pair_distances_per_s_call=float(f"{tested / wall:.4g}"), **more)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--long", type=int, default=50000, help="positions of the one very long pair (0: skip it)")
    ap.add_argument("--radius", type=float, default=15.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--numpy-pairs", type=int, default=50)
    a = ap.parse_args()
    import lddt_restatement as lr
    import superpose_restatement as sr
    from timed_hip import lddt
    rng = np.random.default_rng(0)
    n, length = a.pairs, a.length
    warm = sr.flatten([sr.synthetic_pair(8, rng)] * 2)
    lddt.lddt_arrays(*warm, device=a.device)                                     # warm-up: module load
    for name, make in (("walk", lambda: sr.synthetic_pair(length, rng)), ("globule", lambda: globule(length, rng))):
        distinct = [make() for _ in range(min(n, 64))]                           # 64 different pairs, repeated: the kernel cannot tell
        pairs = [distinct[k % len(distinct)] for k in range(n)]
        ref, mob, offsets = sr.flatten(pairs)
        got, walls, kernels = timed(lddt, ref, mob, offsets, a)
        m = max(1, min(a.numpy_pairs, n))
        t0 = time.perf_counter()
        residue, pair, edge = lr.restate_batch(ref[:offsets[m]], mob[:offsets[m]], offsets[:m + 1], radius=a.radius)
        numpy_s = (time.perf_counter() - t0) / m * n
        if edge > 1e-9:
            assert np.array_equal(got.residue[:offsets[m]], residue) and np.array_equal(got.pair[:m], pair), "GPU and restatement disagree"
        report(f"{n} pairs of {length} positions, {name}", got, offsets, walls, kernels, a, numpy_restatement_s_scaled=round(numpy_s, 3),
               numpy_pairs_timed=m, numpy_edge=float(f"{edge:.3g}"), checked_against_numpy=bool(edge > 1e-9),
               ratio_numpy_over_call=round(numpy_s / float(np.median(walls)), 1))
    if a.long > 0:
        ref, mob = sr.synthetic_pair(a.long, rng)
        offsets = np.array([0, a.long], np.int64)
        got, walls, kernels = timed(lddt, ref, mob, offsets, a)
        assert got.pair[0, 1:].tolist() == got.residue.astype(np.int64).sum(axis=0).tolist() and got.pair[0, 0] == a.long
        report(f"one pair of {a.long} positions, walk", got, offsets, walls, kernels, a)


if __name__ == "__main__":
    main()
