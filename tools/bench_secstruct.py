"""Rate of th_secondary_structure (analyse_properties.py / analyse_models.py --secondary_structure) on ONE submission of N structures
of L residues — models x temperatures x samples x AlphaFold2 outputs are this shape — and on one of a few very long structures: the
device time of each kernel span from the events inside the call (hydrogen bonds with the per-residue preparation; assignment; totals)
and the call on flat arrays (device allocation and copies included), each as median, minimum and maximum over --reps timed calls
after --warmup untimed ones; and the ordered (acceptor, donor) pairs tested per second of the hydrogen-bond span (L^2 per structure).

The structures are copies of the backbone of tests/golden/1ubq.pdb1.gz with seeded 0.2 Angstrom noise, shifted 40 Angstrom apart under
different chain ids and truncated to the length (tests/secstruct_restatement.py: tiled_ubq) — 64 different ones, repeated: the kernel
cannot tell.  The first --numpy-structures structures of the first workload are checked as bytes against the NumPy restatement.

    python tools/bench_secstruct.py [--structures 10000] [--length 300] [--long-structures 100] [--long 4096] [--reps 7] [--warmup 2]
                                    [--out profiles/secstruct_raw.txt]

One JSON line per workload (also appended to --out).  No rate is a pass condition."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SPANS = ("hbonds_ms", "assign_ms", "totals_ms", "kernel_ms")


def spread(values):
    return dict(median=round(float(np.median(values)), 3), min=round(float(min(values)), 3), max=round(float(max(values)), 3))


def run(secstruct, flat, a, bits=False):
    walls, spans = [], {k: [] for k in SPANS}
    got = None
    for rep in range(a.warmup + a.reps):
        timing = {}
        t0 = time.perf_counter()
        got = secstruct.secondary_structure_arrays(*flat, device=a.device, bits=bits, timing=timing)
        wall = (time.perf_counter() - t0) * 1e3
        if rep >= a.warmup:
            walls.append(wall)
            for k in SPANS:
                spans[k].append(timing[k])
    return got, walls, spans


def workload(ss, secstruct, n, length, a, check):
    rng = np.random.default_rng(0)
    distinct = [ss.tiled_ubq(length, rng) for _ in range(min(n, 64))]
    flat = ss.flatten([distinct[k % len(distinct)] for k in range(n)])
    got, walls, spans = run(secstruct, flat, a)
    if a.timing_build:
        check = 0
    else:
        assert got.structure[:, 1].sum() == got.residue[:, 3].astype(np.int64).sum() == got.residue[:, 4].astype(np.int64).sum()      # every bond: one acceptor, one donor
        for k in range(len(distinct), n):                                        # a repeated structure: the same bytes wherever it sits
            assert np.array_equal(got.structure[k], got.structure[k % len(distinct)])
    checked = 0
    for k in range(min(check, n)):
        want = ss.restate(*distinct[k])
        lo, hi = int(flat[3][k]), int(flat[3][k + 1])
        assert got.cls[lo:hi].tobytes() == want["cls"].tobytes() and got.residue[lo:hi].tobytes() == want["residue"].tobytes(), "GPU and restatement disagree"
        assert got.structure[k].tobytes() == want["totals"].tobytes()
        checked += 1
    tested = float(n) * length * length
    hb = float(np.median(spans["hbonds_ms"])) / 1e3
    line = dict(what=f"{n} structures of {length} residues", structures=n, residues=n * length, reps=a.reps, warmup=a.warmup,
                bitmap_mb=round(float(secstruct.bitmap_words(np.diff(flat[3])).sum()) * 8 / 2 ** 20, 1), n_hbonds_per_structure=round(float(got.structure[:, 1].mean()), 1),
                classes="".join(f"{letter}{int(c)} " for letter, c in zip(secstruct.LETTERS, got.structure[:, 2:].sum(axis=0))).strip(),
                call_ms=spread(walls), pairs_tested=tested, pairs_per_s_hbonds=float(f"{tested / hb:.4g}") if hb > 0 else None,
                checked_against_numpy=checked, library=os.path.basename(os.environ.get("TIMED_HIP_LIB", "libtimedhip.so")), **{k: spread(v) for k, v in spans.items()})
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--structures", type=int, default=10000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--long-structures", type=int, default=100)
    ap.add_argument("--long", type=int, default=4096, help="residues of the long structures (0: skip them)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--numpy-structures", type=int, default=3)
    ap.add_argument("--timing-build", action="store_true", help="the library (TIMED_HIP_LIB) is a timing build whose output is wrong by design: check nothing")
    ap.add_argument("--out", type=str, default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import secstruct_restatement as ss
    from timed_hip import secstruct
    workload(ss, secstruct, a.structures, a.length, a, a.numpy_structures)
    if a.long > 0:
        workload(ss, secstruct, a.long_structures, a.long, a, 0)


if __name__ == "__main__":
    main()
