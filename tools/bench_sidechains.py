"""Rate of th_build_sidechains (build_sidechains.py) on N structures of L residues in ONE submission — a design campaign whose
predicted rotamers are built and checked for clashes is this shape: (a) the kernels alone (events inside the call: building, the
deviation from the native, the all-pairs clash count), (b) the call on flat arrays (device allocation and copies included), and
(c) the building kernel alone (clashes=False) — for 10 000 structures of 300 and for a batch of 76-residue structures.  Beside
each: the NumPy restatement (tests/sidechain_restatement.py) on THIS host on --numpy-structures of the structures, scaled to all;
the GPU's counts of those structures are checked against it.

    python tools/bench_sidechains.py [--structures 10000] [--lengths 300 76] [--reps 3] [--numpy-structures 1]

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
    ap.add_argument("--structures", type=int, default=10000)
    ap.add_argument("--lengths", type=int, nargs="+", default=[300, 76])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--numpy-structures", type=int, default=1)
    a = ap.parse_args()
    import rotamer_restatement as rr
    import sidechain_restatement as sr
    from timed_hip import sidechains
    for length in a.lengths:
        rng = np.random.default_rng(0)
        n = a.structures
        distinct = [sr.compact_structure(rng, length, spacing=5.5) for _ in range(min(n, 16))]     # 16 different structures, repeated: the kernel cannot tell
        backbone = np.array([[r[1] for r in s] for s in distinct])                                  # [16, L, 4, 3]
        types = np.array([[sr.type_index(r[0]) for r in s] for s in distinct], dtype=np.int8)
        chi = np.array([[r[2] for r in s] for s in distinct])
        built = [sr.restate_build(s)[0] for s in distinct]
        native = [[(res, [(row[0], xyz[k, j]) for j, row in enumerate(sr.TREE[res])]) for k, (res, _, _) in enumerate(s)] for s, xyz in zip(distinct, built)]
        pick = np.arange(n) % len(distinct)
        flat = [rr.flatten(nat) for nat in native]
        atoms = np.array([len(f[0]) for f in flat])
        atom_lo = np.concatenate([[0], np.cumsum(atoms[pick])])
        nat = (np.concatenate([flat[k][0] for k in pick]), np.concatenate([flat[k][1] for k in pick]),
               np.concatenate([flat[k][2][:-1] + atom_lo[i] for i, k in enumerate(pick)] + [atom_lo[-1:]]), types[pick].reshape(-1))
        args = (backbone[pick].reshape(-1, 4, 3), types[pick].reshape(-1), chi[pick].reshape(-1, 4))
        offsets = np.arange(n + 1, dtype=np.int64) * length
        chain = np.zeros(n * length, np.int32)

        sidechains.build_arrays(args[0][:length], args[1][:length], args[2][:length], device=a.device)       # warm-up: module load
        walls, kernels, build_only = [], [], []
        for _ in range(a.reps):
            timing = {}
            t0 = time.perf_counter()
            got = sidechains.build_arrays(*args, struct_offsets=offsets, chain_id=chain, native=nat, device=a.device, timing=timing)
            walls.append(time.perf_counter() - t0)
            kernels.append(timing["kernel_ms"] / 1e3)
            timing = {}
            sidechains.build_arrays(*args, struct_offsets=offsets, clashes=False, device=a.device, timing=timing)
            build_only.append(timing["kernel_ms"] / 1e3)

        m = max(0, min(a.numpy_structures, n))
        t0 = time.perf_counter()
        host = []
        for k in range(m):
            s = distinct[pick[k]]
            xyz, n_built = sr.restate_build(s)
            n_matched, _ = sr.restate_match(s, xyz, n_built, native[pick[k]])
            host.append((n_built, n_matched) + sr.restate_clashes(s, xyz, np.zeros(length, np.int32), np.array([0, length]))[:2])
        numpy_s = (time.perf_counter() - t0) / m * n if m else None
        for k, (n_built, n_matched, clashes, pairs) in enumerate(host):
            lo, hi = k * length, (k + 1) * length
            assert np.array_equal(got.n_built[lo:hi], n_built) and np.array_equal(got.n_matched[lo:hi], n_matched), k
            assert np.array_equal(got.clashes[lo:hi], clashes) and got.pairs[k] == pairs[0], (k, int(got.pairs[k]), int(pairs[0]))

        wall, kern, only = float(np.median(walls)), float(np.median(kernels)), float(np.median(build_only))
        n_atoms = int(got.n_built.sum())
        print(json.dumps(dict(what=f"{n} structures of {length} residues", structures=n, residues=n * length, atoms_built=n_atoms, submissions=1, reps=a.reps,
                              clashing_pairs=int(got.pairs.sum()), rmsd_to_own_float64_build=float(f"{np.sqrt(got.sum_sq.sum() / max(1, got.n_matched.sum())):.3g}"),
                              kernel_ms_median=round(kern * 1e3, 3), kernel_ms_min=round(min(kernels) * 1e3, 3), build_kernel_ms_median=round(only * 1e3, 3),
                              call_ms_median=round(wall * 1e3, 3), call_ms_min=round(min(walls) * 1e3, 3),
                              structures_per_s_kernel=float(f"{n / kern:.4g}"), structures_per_s_call=float(f"{n / wall:.4g}"),
                              atoms_per_s_build_kernel=float(f"{n_atoms / only:.4g}"),
                              numpy_restatement_s_scaled=None if numpy_s is None else round(numpy_s, 1), numpy_structures_timed=m,
                              checked_against_numpy=m > 0, ratio_numpy_over_call=None if numpy_s is None else round(numpy_s / wall, 1))), flush=True)


if __name__ == "__main__":
    main()
