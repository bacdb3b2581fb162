"""Rate of th_sasa (analyse_properties.py / analyse_models.py --sasa) on ONE submission of N structures of 602 atoms — models x
temperatures x samples x AlphaFold2 outputs are this shape — at 96 and at 960 points per atom, and on one of a few very long
structures: the device time of each kernel span from the events inside the call (occlusion; totals) and the call on flat arrays
(device allocation and copies included), each as median, minimum and maximum over --reps timed calls after --warmup untimed ones; and
the point-neighbour tests per second of the occlusion span — points x near atoms summed over the atoms, what the kernel does without
its early exit, counted by the NumPy restatement's pre-filter.

The structures are copies of the heavy atoms of tests/golden/1ubq.pdb1.gz with seeded 0.2 Angstrom noise — 64 different ones,
repeated: the kernel cannot tell; a long structure is such copies 50 Angstrom apart along x, truncated to the length.  The first
--numpy-structures structures of every workload are checked as bytes against the NumPy restatement, whose wall time is reported.

    python tools/bench_sasa.py [--structures 1000 10000] [--points 96 960] [--long-structures 100] [--long 8192] [--reps 7] [--warmup 2]
                               [--out profiles/sasa_raw.txt]

TIMED_HIP_LIB=<library built with -DTH_SASA_EARLY_EXIT=0> runs the same on the kernel without the early exit: the same bytes, so the
check stays on.  One JSON line per workload (also appended to --out).  No rate is a pass condition."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SPANS = ("points_ms", "totals_ms", "kernel_ms")


def spread(values):
    return dict(median=round(float(np.median(values)), 3), min=round(float(min(values)), 3), max=round(float(max(values)), 3))


def noisy_structure(sr, length, rng, sigma=0.2, shift=50.0):
    xyz, radius = sr.ubq_atoms()[:2]
    copies = -(-length // len(xyz))
    parts = [xyz + rng.normal(0.0, sigma, xyz.shape) + np.array([k * shift, 0.0, 0.0]) for k in range(copies)]
    return np.concatenate(parts)[:length], np.tile(radius, copies)[:length]


def workload(sr, sasa, n, length, n_points, a, distinct_count):
    rng = np.random.default_rng(0)
    points = sasa.sphere_points(n_points)
    distinct = [noisy_structure(sr, length, rng) for _ in range(min(n, distinct_count))]
    flat = sr.flatten([distinct[k % len(distinct)] for k in range(n)])
    walls, spans, got = [], {k: [] for k in SPANS}, None
    for rep in range(a.warmup + a.reps):
        timing = {}
        t0 = time.perf_counter()
        got = sasa.sasa_arrays(*flat, probe=sr.PROBE, points=points, device=a.device, timing=timing)
        wall = (time.perf_counter() - t0) * 1e3
        if rep >= a.warmup:
            walls.append(wall)
            for k in SPANS:
                spans[k].append(timing[k])
    for k in range(len(distinct), n):                                            # a repeated structure: the same bytes wherever it sits
        assert np.array_equal(got.structure[k], got.structure[k % len(distinct)])
    checked, numpy_s = 0, 0.0
    for k in range(min(a.numpy_structures, n)):
        t0 = time.perf_counter()
        want = sr.restate(*distinct[k], sr.PROBE, points)
        numpy_s += time.perf_counter() - t0
        lo, hi = int(flat[2][k]), int(flat[2][k + 1])
        assert got.exposed[lo:hi].tobytes() == want["exposed"].tobytes() and got.structure[k].tobytes() == want["totals"].tobytes(), "GPU and restatement disagree"
        checked += 1
    near = [float(sr.near_pairs(xyz, radius + sr.PROBE, np.ones(len(xyz), bool))[0].size) for xyz, radius in distinct]
    tests = float(sum(near[k % len(distinct)] for k in range(n))) * n_points
    occlusion = float(np.median(spans["points_ms"])) / 1e3
    area = float(sr.atom_areas(got.exposed[:length], flat[1][:length], sr.PROBE, n_points).sum())
    line = dict(what=f"{n} structures of {length} atoms at {n_points} points", structures=n, atoms=n * length, points=n_points, reps=a.reps,
                warmup=a.warmup, near_per_atom=round(sum(near) / (len(distinct) * length), 1), first_structure_area=round(area, 1),
                buried_atoms_share=round(float(got.structure[:, 1].sum()) / max(1.0, float(got.structure[:, 0].sum())), 3), call_ms=spread(walls),
                point_neighbour_tests=tests, tests_per_s_occlusion=float(f"{tests / occlusion:.4g}") if occlusion > 0 else None,
                checked_against_numpy=checked, numpy_s_per_structure=round(numpy_s / checked, 3) if checked else None,
                library=os.path.basename(os.environ.get("TIMED_HIP_LIB", "libtimedhip.so")), **{k: spread(v) for k, v in spans.items()})
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--structures", type=int, nargs="*", default=[1000, 10000])
    ap.add_argument("--length", type=int, default=602)
    ap.add_argument("--points", type=int, nargs="*", default=[96, 960])
    ap.add_argument("--long-structures", type=int, default=100)
    ap.add_argument("--long", type=int, default=8192, help="atoms of the long structures (0: skip them)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--numpy-structures", type=int, default=3)
    ap.add_argument("--out", type=str, default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import sasa_restatement as sr
    from timed_hip import sasa
    for n in a.structures:
        for n_points in a.points:
            workload(sr, sasa, n, a.length, n_points, a, 64)
    if a.long > 0:
        workload(sr, sasa, a.long_structures, a.long, 96, a, 4)


if __name__ == "__main__":
    main()
