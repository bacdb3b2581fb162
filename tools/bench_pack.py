"""Time of th_pack_sidechains (pack_sidechains.py) per kernel, in ONE submission each: 1000 copies of 1ubq and 100 structures of 300
residues (a jittered 5.5 Angstrom lattice, random types, 4 distinct structures repeated: the kernel cannot tell) — candidates,
backbone penalties, search; sweeps to convergence; the call on flat arrays (device allocation and copies included).  Beside each:
the wall time of the NumPy restatement (tests/pack_restatement.py) on ONE of the structures on this host — a CPU RESTATEMENT
written for clarity, NOT a baseline — whose outputs the GPU's are checked against.  Then the 1ubq table of the README, measured by
the restatement (tests/golden/make_pack_golden.py).

    python tools/bench_pack.py [--output profiles/pack_sidechains.txt] [--reps 3]

Writes the report to --output and prints it.  Nothing here is a pass condition, and there is no packer in the parent commit, and none
where this is measured, to compare against: SCWRL4 was not run, no CPU packer was timed, and the rates are the rates measured."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def workload(pr, name, distinct, copies, reps, device, packer):
    structures = [distinct[k % len(distinct)] for k in range(copies)]
    backbone, types, offsets, chain, prior = pr.flat(structures)
    packer.pack_arrays(backbone[:offsets[1]], types[:offsets[1]], device=device)                        # warm-up: module load
    rows, walls = [], []
    for _ in range(reps):
        timing = {}
        t0 = time.perf_counter()
        got = packer.pack_arrays(backbone, types, offsets, chain, prior, device=device, timing=timing)
        walls.append(time.perf_counter() - t0)
        rows.append([timing[k] for k in ("pack_candidates_ms", "pack_backbone_ms", "pack_search_ms")])
    t0 = time.perf_counter()
    want = pr.restate_pack(*structures[0][:2])
    cpu_s = time.perf_counter() - t0
    n0 = int(offsets[1])
    assert np.array_equal(got.cls[:n0], want["cls"]) and int(got.energy_final[0]) == want["energy_final"] and int(got.n_sweeps[0]) == want["n_sweeps"]
    assert want["margin"] > pr.MARGIN_BOUND
    med = np.median(np.array(rows), axis=0)
    return dict(what=name, structures=copies, residues=int(offsets[-1]), candidates=int(packer.candidate_counts(types).sum()), reps=reps,
                candidates_kernel_ms=round(float(med[0]), 3), backbone_kernel_ms=round(float(med[1]), 3), search_kernel_ms=round(float(med[2]), 3),
                kernels_ms=round(float(med.sum()), 3), call_ms_median=round(float(np.median(walls)) * 1e3, 3),
                sweeps_min=int(got.n_sweeps.min()), sweeps_max=int(got.n_sweeps.max()), moves=int(got.n_moves.sum()), converged=int(got.converged.sum()),
                energy_initial=int(got.energy_initial.sum()), energy_final=int(got.energy_final.sum()),
                structures_per_s_kernels=float(f"{copies / (med.sum() / 1e3):.4g}"),
                cpu_restatement_s_one_structure=round(cpu_s, 2), checked_against_restatement=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "pack_sidechains.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import make_pack_golden
    import pack_restatement as pr
    from timed_hip import packer
    ubq, _, _ = pr.ubq_structure()
    lines = [workload(pr, "1000 copies of 1ubq (76 residues)", [(ubq, None, None)], 1000, a.reps, a.device, packer),
             workload(pr, "100 structures of 300 residues", [(pr.compact(100 + k, 300, spacing=5.5), None, None) for k in range(4)], 100, a.reps, a.device, packer)]
    table = io.StringIO()
    with contextlib.redirect_stdout(table):
        make_pack_golden.table()
    report = ["th_pack_sidechains (csrc/pack_sidechains.hip) — measurements of tools/bench_pack.py", "",
              "Default ladder (2.0, 2.5, 3.0, 3.5), clash_weight 2000, no prior, max_sweeps 10; kernel times from events inside the call, median of",
              f"{a.reps}; the call includes device allocation and copies.  cpu_restatement_s_one_structure is the wall time of the NumPy restatement",
              "(tests/pack_restatement.py) on ONE structure of the workload on the host of this run: a restatement written for clarity and labelled",
              "as such, NOT a baseline.  The GPU's classes, final energy and sweeps of that structure are checked against it.",
              "Not measured: SCWRL4 (not available), any tuned CPU packer, the prior's effect with a real model (none is available).", ""]
    report += [json.dumps(line) for line in lines]
    report += ["", "1ubq, 68 residues with a chi angle, measured by the restatement (tests/golden/make_pack_golden.py):", ""] + table.getvalue().splitlines()
    text = "\n".join(report) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
