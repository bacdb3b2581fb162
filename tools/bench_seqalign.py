"""Rate of th_seqalign (analyse_models.py --seqalign) on ONE submission of P pairs of n x m residues: the device time of k_seqalign_fill
and of k_seqalign_trace from the events inside the call, their sum, and the call on flat arrays (device allocation and copies
included), each as median, minimum and maximum over --reps timed calls after --warmup untimed ones; and the cell updates per second,
P n m over the fill and over both kernels.

A pair is a random sequence and a copy of it with every residue substituted with probability --mutate and a stretch of 6 cut out of its
middle — 8 different pairs, repeated: the kernel cannot tell, and a repeated pair is checked to give the same bytes.  The first pair
of every workload is checked as bytes against the restatement (tests/seqalign_restatement.py), whose wall time for that ONE pair on
this host is reported: the only other implementation there is, a ratio, not a target.

    python tools/bench_seqalign.py [--shapes 10000x76x76 1000x300x300 100x2048x2048] [--reps 7] [--warmup 2] [--out profiles/seqalign_raw.txt]

One JSON line per workload (also appended to --out); profiles/seqalign.txt is written up from them.  No rate is a pass condition."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SPANS = ("fill_ms", "trace_ms", "kernel_ms")


def spread(values):
    return dict(median=round(float(np.median(values)), 3), min=round(float(min(values)), 3), max=round(float(max(values)), 3))


def make_pair(rng, n, m, mutate):
    base = rng.integers(0, 20, max(n, m) + 6).astype(np.uint8)
    model = np.concatenate([base[:m // 2], base[m // 2 + 6:]])[:m].copy()
    hit = rng.random(m) < mutate
    model[hit] = rng.integers(0, 20, int(hit.sum())).astype(np.uint8)
    return base[:n].copy(), model


def workload(ar, seqalign, shape, a):
    n_pairs, n, m = shape
    rng = np.random.default_rng(0)
    distinct = [make_pair(rng, n, m, a.mutate) for _ in range(min(n_pairs, 8))]
    pairs = [distinct[k % len(distinct)] for k in range(n_pairs)]
    ref, ro, mob, mo = ar.flatten(pairs)
    walls, spans, got = [], {k: [] for k in SPANS}, None
    for rep in range(a.warmup + a.reps):
        timing = {}
        t0 = time.perf_counter()
        got = seqalign.seqalign_arrays(ref, ro, mob, mo, free_ends=not a.charged_ends, device=a.device, timing=timing)
        wall = (time.perf_counter() - t0) * 1e3
        if rep >= a.warmup:
            walls.append(wall)
            for k in SPANS:
                spans[k].append(timing[k])
    for k in range(len(distinct), n_pairs):                                      # a repeated pair: the same bytes wherever it sits
        j = k % len(distinct)
        assert np.array_equal(got.counts[k], got.counts[j]) and np.array_equal(got.align[ro[k]:ro[k + 1]], got.align[ro[j]:ro[j + 1]])
    numpy_s = None
    if not a.no_check:
        t0 = time.perf_counter()
        want = ar.restate(*pairs[0], free_ends=int(not a.charged_ends))
        numpy_s = time.perf_counter() - t0
        assert got.counts[0].tobytes() == want["counts"].tobytes() and got.align[:n].tobytes() == want["align"].tobytes(), "GPU and restatement disagree"
    cells = float(n_pairs) * n * m
    fill_s, kernel_ms = float(np.median(spans["fill_ms"])) / 1e3, float(np.median(spans["kernel_ms"]))
    line = dict(what=f"{n_pairs} pair(s) of {n} x {m}", pairs=n_pairs, n=n, m=m, reps=a.reps, warmup=a.warmup, mutate=a.mutate,
                free_ends=not a.charged_ends, first_pair_counts=got.counts[0].tolist(), cells=cells,
                trace_bytes_per_pair=seqalign.trace_bytes(n, m), cells_per_s_fill=float(f"{cells / fill_s:.4g}") if fill_s > 0 else None,
                cells_per_s_kernels=float(f"{cells / (kernel_ms / 1e3):.4g}") if kernel_ms > 0 else None,
                trace_share=round(float(np.median(spans["trace_ms"])) / kernel_ms, 4) if kernel_ms > 0 else None, call_ms=spread(walls),
                restatement_s_per_pair=None if numpy_s is None else round(numpy_s, 4),
                restatement_all_pairs_over_kernels=None if numpy_s is None or kernel_ms <= 0 else round(numpy_s * n_pairs * 1e3 / kernel_ms, 0),
                library=os.path.basename(os.environ.get("TIMED_HIP_LIB", "libtimedhip.so")), **{k: spread(v) for k, v in spans.items()})
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", type=str, nargs="*", default=["10000x76x76", "1000x300x300", "100x2048x2048"], help="PAIRSxNxM")
    ap.add_argument("--mutate", type=float, default=0.3)
    ap.add_argument("--charged-ends", action="store_true", help="free_ends = 0")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-check", action="store_true", help="skip the restatement of the first pair")
    ap.add_argument("--out", type=str, default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import seqalign_restatement as ar
    from timed_hip import seqalign
    for shape in a.shapes:
        workload(ar, seqalign, tuple(int(v) for v in shape.split("x")), a)


if __name__ == "__main__":
    main()
