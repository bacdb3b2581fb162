"""Rate of th_packing_density (analyse_properties.py): (a) 2 000 structures of about 2 500 atoms in ONE submission, (b) one
100 000-atom structure, (c) 1ubq alone (660 atoms: the fixed cost of a call).  Per workload: wall time of the call through the C
ABI with host arrays (copies, allocation and the per-residue reduction included), the device time of the two kernels (events
inside the call), pair tests per second from each — and beside them the reference's per-atom NumPy loop
(design_utils/analyse_utils.py tag_packing_density, restated line for line below) timed on THIS host on a subsample of atoms and
EXTRAPOLATED to all atoms (the loop's cost per atom is constant within a structure, so the extrapolation is a multiplication; it
is still not a measurement of the whole run).

    python tools/bench_packdensity.py [--reps 5] [--structures 2000] [--atoms 2500] [--big 100000] [--numpy-atoms 64]

One JSON line per workload."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))


def random_structure(rng, n):
    """protein-like density: one atom per 20 cubic Angstrom, three-decimal coordinates"""
    half = max(3.0, (n * 20.0) ** (1 / 3) / 2)
    return np.round(rng.uniform(-half, half, (n, 3)), 3)


def residues_of(sizes, per_residue=8):
    """every atom reported, residues of 8 consecutive atoms, all selected"""
    group, n_groups = [], 0
    for n in sizes:
        k = (n + per_residue - 1) // per_residue
        group.append(np.repeat(np.arange(n_groups, n_groups + k, dtype=np.int32), per_residue)[:n])
        n_groups += k
    group = np.concatenate(group) if group else np.zeros(0, np.int32)
    return group, np.ones(len(group), np.uint8), n_groups


def numpy_loop_seconds(xyz, offsets, radius, sample_atoms, rng):
    """the reference's loop body for ``sample_atoms`` atoms of each of up to 3 structures -> seconds for all atoms, extrapolated"""
    total_s, n_structures = 0.0, len(offsets) - 1
    picked = rng.choice(n_structures, min(3, n_structures), replace=False)
    per_atom = []
    for s in picked:
        coords = xyz[offsets[s]:offsets[s + 1]]
        if not len(coords):
            continue
        idx = rng.choice(len(coords), min(sample_atoms, len(coords)), replace=False)
        t0 = time.perf_counter()
        for index in idx:
            distances = np.sqrt(np.square(coords[:, :] - coords[index, :]).sum(axis=1))
            _ = np.sum(distances < radius) - 1
        per_atom.append((time.perf_counter() - t0) / len(idx) / len(coords))       # seconds per pair
    per_pair = float(np.median(per_atom))
    sizes = np.diff(offsets).astype(np.float64)
    total_s = per_pair * float((sizes * sizes).sum())
    return total_s, per_pair


def bench(name, xyz, offsets, reps, device, sample_atoms, rng, radius=7.0):
    from timed_hip import structure
    sizes = np.diff(offsets)
    group, selected, n_groups = residues_of(sizes)
    pairs = float((sizes.astype(np.float64) ** 2).sum())
    structure.contact_numbers(xyz, offsets, radius, group, selected, n_groups, device=device)        # warm-up: module load, first allocation
    walls, kernels = [], []
    for _ in range(reps):
        timing = {}
        t0 = time.perf_counter()
        structure.contact_numbers(xyz, offsets, radius, group, selected, n_groups, device=device, timing=timing)
        walls.append(time.perf_counter() - t0)
        kernels.append(timing["kernel_ms"] / 1e3)
    wall, kern = float(np.median(walls)), float(np.median(kernels))
    numpy_s, per_pair = numpy_loop_seconds(xyz, offsets, radius, sample_atoms, rng)
    row = dict(what=name, structures=len(sizes), atoms=int(sizes.sum()), pair_tests=pairs, reps=reps,
               wall_s_median=round(wall, 6), wall_s_min=round(min(walls), 6), kernel_s_median=round(kern, 6), kernel_s_min=round(min(kernels), 6),
               pair_tests_per_s_wall=float(f"{pairs / wall:.4g}"), pair_tests_per_s_kernel=float(f"{pairs / kern:.4g}") if kern > 0 else None,
               numpy_loop_s_extrapolated=round(numpy_s, 3), numpy_ns_per_pair=round(per_pair * 1e9, 3), numpy_sample_atoms_per_structure=sample_atoms,
               wall_ratio_numpy_over_gpu=round(numpy_s / wall, 1))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--structures", type=int, default=2000)
    ap.add_argument("--atoms", type=int, default=2500)
    ap.add_argument("--big", type=int, default=100000)
    ap.add_argument("--numpy-atoms", type=int, default=64, help="atoms per sampled structure the NumPy loop is timed on")
    a = ap.parse_args()
    from timed_hip import pdbio, structure
    rng = np.random.default_rng(0)
    sizes = rng.integers(int(a.atoms * 0.8), int(a.atoms * 1.2) + 1, a.structures)
    xyz = np.concatenate([random_structure(rng, int(n)) for n in sizes])
    bench(f"(a) {a.structures} structures of ~{a.atoms} atoms", xyz, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), a.reps,
          a.device, a.numpy_atoms, rng)
    bench(f"(b) one structure of {a.big} atoms", random_structure(rng, a.big), np.array([0, a.big], np.int64), a.reps, a.device,
          a.numpy_atoms, rng)
    lay = structure.layout(pdbio.read_pdb(os.path.join(ROOT, "tests", "golden", "1ubq.pdb1.gz"))[0], "all")
    bench("(c) 1ubq alone", lay.xyz, np.array([0, len(lay.xyz)], np.int64), max(a.reps, 20), a.device, a.numpy_atoms, rng)


if __name__ == "__main__":
    main()
