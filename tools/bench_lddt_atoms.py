"""Rate of th_lddt_atoms (analyse_models.py --lddt_all_atom, build_sidechains.py / pack_sidechains.py --lddt) in ONE submission: N noisy
copies of the 601 heavy atoms of tests/golden/1ubq.pdb1.gz against the native — every second copy with its symmetric names exchanged,
so the resolution has swaps to make — and then structures of --big-atoms atoms (copies of 1ubq side by side, cut at that length):
(a) all kernels (events inside the call) and of those the symmetry resolution alone (k_lddt_resolve + k_lddt_decide), (b) the call on
flat arrays (device allocation and copies included), the ordered pairs (i, j) of atoms tested per second (n^2 per structure) and the
INCLUDED pairs per second of the counting kernels — the figure to hold beside k_lddt's in profiles/lddt.txt — and the NumPy
restatement on THIS host per structure.  The integers of the structures the restatement covers are checked against it when no
decision of theirs sits within 1e-9 of a tie and no symmetric residue is tied.

    python tools/bench_lddt_atoms.py [--copies 1000 10000] [--big 100] [--big-atoms 8192] [--reps 5] [--numpy-structures 3]

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


def noisy_copies(base, n, rng, sigma=0.3, distinct=64):
    """n structures: `distinct` different noisy models of `base`, repeated (the kernel cannot tell); every second one exchanged"""
    import lddt_atoms_restatement as ar
    models = []
    for k in range(min(n, distinct)):
        mob = base["ref"] + rng.normal(0.0, sigma, base["ref"].shape)
        models.append(dict(base, mob=ar.exchanged(mob, base["partner"]) if k % 2 else mob))
    return [models[k % len(models)] for k in range(n)]


def side_by_side(base, atoms):
    """copies of `base` on a grid of 30 Angstrom, as one structure cut at `atoms` atoms (a partner beyond the cut is dropped)"""
    n = len(base["ref"])
    copies = -(-atoms // n)
    grid = np.array([[x, y, z] for z in range(8) for y in range(8) for x in range(8)], np.float64)[:copies] * 30.0
    ref = np.concatenate([base["ref"] + shift for shift in grid])[:atoms]
    per = int(base["residue"][-1]) + 1
    residue = np.concatenate([base["residue"] + k * per for k in range(copies)])[:atoms].astype(np.int32)
    partner = np.concatenate([np.where(base["partner"] >= 0, base["partner"] + k * n, -1) for k in range(copies)])[:atoms].astype(np.int32)
    partner[partner >= atoms] = -1
    partner[(partner >= 0) & (partner[np.maximum(partner, 0)] != np.arange(atoms))] = -1
    return dict(ref=ref, residue=residue, partner=partner)


def timed(module, flat, a):
    walls, kernels, resolves = [], [], []
    for _ in range(a.reps):
        timing = {}
        t0 = time.perf_counter()
        got = module.lddt_atoms_arrays(*flat, radius=a.radius, device=a.device, timing=timing)
        walls.append(time.perf_counter() - t0)
        kernels.append(timing["kernel_ms"] / 1e3)
        resolves.append(timing["resolve_ms"] / 1e3)
    return got, walls, kernels, resolves


def report(what, got, flat, walls, kernels, resolves, a, **more):
    sizes = np.diff(flat[4]).astype(np.float64)
    tested, included = float((sizes * sizes).sum()), float(got.pair[:, 2].sum())
    wall, kern, res = float(np.median(walls)), float(np.median(kernels)), float(np.median(resolves))
    score = got.pair[:, 3:7].sum(axis=1) / np.maximum(4.0 * got.pair[:, 2], 1.0)
    print(json.dumps(dict(what=what, structures=len(sizes), atoms=int(sizes.sum()), partnered_atoms=int((flat[3] >= 0).sum()), radius=a.radius,
                          submissions=1, reps=a.reps, ordered_pairs_tested=tested, included_pairs=included,
                          included_fraction=round(included / tested, 4), swapped_residues=int(got.pair[:, 7].sum()),
                          lddt_mean=round(float(score.mean()), 4), kernel_ms_median=round(kern * 1e3, 3), kernel_ms_min=round(min(kernels) * 1e3, 3),
                          resolve_ms_median=round(res * 1e3, 3), resolve_share=round(res / kern, 3) if kern > 0 else None,
                          call_ms_median=round(wall * 1e3, 3), call_ms_min=round(min(walls) * 1e3, 3),
                          pairs_tested_per_s_kernel=float(f"{tested / kern:.4g}") if kern > 0 else None,
                          included_pairs_per_s_counting_kernels=float(f"{included / (kern - res):.4g}") if kern > res else None,
                          pairs_tested_per_s_call=float(f"{tested / wall:.4g}"), **more)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--copies", type=int, nargs="*", default=[1000, 10000])
    ap.add_argument("--big", type=int, default=100, help="structures of --big-atoms atoms (0: skip them)")
    ap.add_argument("--big-atoms", type=int, default=8192)
    ap.add_argument("--radius", type=float, default=15.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--numpy-structures", type=int, default=3)
    a = ap.parse_args()
    import lddt_atoms_restatement as ar
    from timed_hip import lddt_atoms
    rng = np.random.default_rng(0)
    golden = np.load(ar.GOLDEN)
    base = {key: golden[f"self_{key}"] for key in ("ref", "residue", "partner")}
    lddt_atoms.lddt_atoms_arrays(*ar.flatten([dict(base, mob=base["ref"])]), device=a.device)        # warm-up: module load
    for n in a.copies:
        cases = noisy_copies(base, n, rng)
        flat = ar.flatten(cases)
        got, walls, kernels, resolves = timed(lddt_atoms, flat, a)
        m = max(1, min(a.numpy_structures, n))
        t0 = time.perf_counter()
        restated = [ar.restate(*(case[key] for key in ar.INPUTS), radius=a.radius) for case in cases[:m]]
        numpy_s = (time.perf_counter() - t0) / m
        fair = all(r["edge"] > 1e-9 and r["margin"] > 0 for r in restated)
        if fair:
            for k, r in enumerate(restated):
                lo, hi = int(flat[4][k]), int(flat[4][k + 1])
                assert np.array_equal(got.atom[lo:hi], r["atom"]) and np.array_equal(got.swapped[lo:hi], r["swapped"]), "GPU and restatement disagree"
                assert np.array_equal(got.pair[k], r["pair"]), "GPU and restatement disagree"
        report(f"{n} noisy copies of 1ubq (601 atoms)", got, flat, walls, kernels, resolves, a, numpy_restatement_s_per_structure=round(numpy_s, 4),
               numpy_structures_timed=m, checked_against_numpy=bool(fair), ratio_numpy_all_over_call=round(numpy_s * n / float(np.median(walls)), 1))
    if a.big > 0:
        big = side_by_side(base, a.big_atoms)
        cases = noisy_copies(big, a.big, rng, distinct=8)
        flat = ar.flatten(cases)
        got, walls, kernels, resolves = timed(lddt_atoms, flat, a)
        assert got.pair[:, 2:7].sum(axis=0).tolist() == got.atom.astype(np.int64).sum(axis=0).tolist() and (got.pair[:, 0] == a.big_atoms).all()
        report(f"{a.big} structures of {a.big_atoms} atoms (copies of 1ubq side by side)", got, flat, walls, kernels, resolves, a)


if __name__ == "__main__":
    main()
