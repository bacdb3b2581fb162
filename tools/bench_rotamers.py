"""Rate of th_tag_rotamers (tag_rotamers.py, analyse_rotamers.py --path_to_pdb) on N replicas of 1ubq (76 residues, 602 atoms each):
(a) the kernel alone (events inside the call), (b) timed_hip.structure.tag_rotamers on parsed layouts (batching in Python, device allocation and copies included),
(c) end to end from the file: parsing with timed_hip.pdbio on --workers host threads, flattening, the call — and beside them
the NumPy restatement of the same rule (tests/rotamer_restatement.py: a dict lookup and the float64 formula per residue) timed on
THIS host on the same residues (on --numpy-structures of them, scaled to all: its cost per structure is constant).  Classes of
every replica are checked against the restatement's.

    python tools/bench_rotamers.py [--structures 4000] [--reps 5] [--workers 16] [--numpy-structures 20]

One JSON line."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--structures", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--numpy-structures", type=int, default=20)
    a = ap.parse_args()
    import rotamer_restatement as rr
    from timed_hip import pdbio, structure
    n = a.structures
    model = pdbio.read_pdb(rr.UBQ)[0]
    lay = structure.rotamer_layout(model)
    layouts = [lay] * n
    residues = rr.residues_of_model(model)
    want, _ = rr.restate(residues)

    structure.tag_rotamers(layouts[:2], device=a.device)                                  # warm-up: module load, first allocation
    walls, kernels, subs = [], [], 0
    for _ in range(a.reps):
        stats = {}
        t0 = time.perf_counter()
        tagged = structure.tag_rotamers(layouts, device=a.device, stats=stats)
        walls.append(time.perf_counter() - t0)
        kernels.append(stats["kernel_ms"] / 1e3)
        subs = stats["submissions"]
    assert all(np.array_equal(t.cls, want) for t in tagged)

    e2e = []
    for _ in range(max(1, a.reps // 2)):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=a.workers) as pool:
            parsed = list(pool.map(lambda _k: structure.rotamer_layout(structure.first_model(rr.UBQ)), range(n)))
        t_parse = time.perf_counter() - t0
        structure.tag_rotamers(parsed, device=a.device)
        e2e.append((time.perf_counter() - t0, t_parse))

    m = max(1, min(a.numpy_structures, n))
    t0 = time.perf_counter()
    for _ in range(m):
        got, _ = rr.restate(residues)
    numpy_s = (time.perf_counter() - t0) / m * n
    assert np.array_equal(got, want)

    wall, kern = float(np.median(walls)), float(np.median(kernels))
    end, parse = min(e2e)
    n_res, n_atoms = n * len(lay.residues), n * len(lay.xyz)
    print(json.dumps(dict(what=f"{n} replicas of 1ubq", structures=n, residues=n_res, atoms=n_atoms, submissions=subs, reps=a.reps,
                          kernel_s_median=round(kern, 6), kernel_s_min=round(min(kernels), 6), call_s_median=round(wall, 6), call_s_min=round(min(walls), 6),
                          residues_per_s_kernel=float(f"{n_res / kern:.4g}") if kern > 0 else None, residues_per_s_call=float(f"{n_res / wall:.4g}"),
                          end_to_end_s=round(end, 3), of_which_parsing_s=round(parse, 3), parse_workers=a.workers,
                          numpy_restatement_s_scaled=round(numpy_s, 3), numpy_structures_timed=m,
                          ratio_numpy_over_call=round(numpy_s / wall, 1))), flush=True)


if __name__ == "__main__":
    main()
