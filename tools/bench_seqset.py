"""Rate of th_seqset (analyse_samples.py) on ONE submission of S sets of N draws of L residues — what sample.py writes for S structures:
the device time of the kernels before the clustering (pack, pairs, native, columns), of k_seqset_cluster and of all kernels from the
events inside the call, and the call on flat arrays (device allocation and copies included), each as median, minimum and maximum over
--reps timed calls after --warmup untimed ones; and the residue comparisons per second, S N^2 L over the time before the clustering.

A set is a random native and N draws of it, every position redrawn with probability --mutate (0.5: draws about 28 % identical to one
another, so that at --cluster_identity 0.9 nearly every draw is a representative — the most the cluster kernel can be given) — 8
different sets, repeated: the kernel cannot tell.  The first workload is checked as bytes against the NumPy restatement
(tests/seqset_restatement.py), whose wall time on this host is reported: the only other implementation there is, a ratio, not a target.

    python tools/bench_seqset.py [--shapes 1x1000x300 1x10000x300 100x1000x300 1x1000x3000] [--reps 7] [--warmup 2] [--out profiles/seqset_raw.txt]
    python tools/bench_seqset.py --build-variant bytes -DTH_SEQSET_PACKED=0      # the same sources with the flag(s) into a library of its own
    python tools/bench_seqset.py --build-variant chunk512 -DTH_SEQSET_CHUNK=512  # (timed_hip/libtimedhip_seqset_<name>.so); prints its path

TIMED_HIP_LIB=<that library> runs the same on that build — the kernel that compares byte by byte, or another chunk of positions: the
same bytes, so the check stays on.  One JSON
line per workload (also appended to --out).  No rate is a pass condition."""
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

SPANS = ("pairs_ms", "cluster_ms", "kernel_ms")


def spread(values):
    return dict(median=round(float(np.median(values)), 3), min=round(float(min(values)), 3), max=round(float(max(values)), 3))


def build_variant(name, flags):
    """csrc/seqset.hip alone with the flags (no other source reads them), linked with the product's objects of everything else"""
    import __graft_entry__ as entry
    entry.build_lib()
    objdir = os.path.join(entry.CSRC, f"build_seqset_{name}")
    os.makedirs(objdir, exist_ok=True)
    mine = os.path.join(objdir, "seqset.o")
    entry._run([entry.HIPCC, *entry.HIP_FLAGS, *flags, "-c", os.path.join(entry.CSRC, "seqset.hip"), "-o", mine])
    objs = [mine if src == "seqset.hip" else os.path.join(entry.CSRC, "build", src.replace(".hip", ".o")) for src in entry.HIP_SOURCES]
    lib = os.path.join(entry.PKG, "timed_hip", f"libtimedhip_seqset_{name}.so")
    entry._run([entry.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", lib, "-ldl", "-lz"])
    print(f"TIMED_HIP_LIB={lib}")


def make_set(rng, n, length, mutate):
    native = rng.integers(0, 20, length).astype(np.uint8)
    draws = np.tile(native, (n, 1))
    change = rng.random(draws.shape) < mutate
    draws[change] = rng.integers(0, 20, int(change.sum())).astype(np.uint8)
    return draws, native


def workload(qr, seqset, shape, a, check):
    n_sets, n, length = shape
    rng = np.random.default_rng(0)
    distinct = [make_set(rng, n, length, a.mutate) for _ in range(min(n_sets, 8))]
    threshold = seqset.min_matches_of(a.cluster_identity, length)
    parts = [distinct[k % len(distinct)] + (threshold,) for k in range(n_sets)]
    codes, offsets, lengths, native, thresholds = qr.flatten(parts)
    walls, spans, got = [], {k: [] for k in SPANS}, None
    for rep in range(a.warmup + a.reps):
        timing = {}
        t0 = time.perf_counter()
        got = seqset.seqset_arrays(codes, offsets, lengths, native, thresholds, device=a.device, timing=timing)
        wall = (time.perf_counter() - t0) * 1e3
        if rep >= a.warmup:
            walls.append(wall)
            for k in SPANS:
                spans[k].append(timing[k])
    for k in range(len(distinct), n_sets):                                       # a repeated set: the same bytes wherever it sits
        assert np.array_equal(got.sets[k], got.sets[k % len(distinct)])
    numpy_s = None
    if check:
        t0 = time.perf_counter()
        want = qr.restate(*parts[0])
        numpy_s = time.perf_counter() - t0
        assert got.seq[:n].tobytes() == want["seq"].tobytes() and got.profile[:length].tobytes() == want["profile"].tobytes(), "GPU and restatement disagree"
        assert got.sets[0].tobytes() == want["set"].tobytes()
    comparisons = float(n_sets) * n * n * length
    pairs_s, kernel = float(np.median(spans["pairs_ms"])) / 1e3, float(np.median(spans["kernel_ms"]))
    line = dict(what=f"{n_sets} set(s) of {n} x {length}", sets=n_sets, n=n, length=length, reps=a.reps, warmup=a.warmup, mutate=a.mutate,
                min_matches=threshold, clusters_first_set=int(got.sets[0, 2]), distinct_first_set=int(got.sets[0, 1]),
                mean_pairwise_identity=round(float(got.sets[0, 0]) / (n * (n - 1) / 2 * length), 4), residue_comparisons=comparisons,
                comparisons_per_s=float(f"{comparisons / pairs_s:.4g}") if pairs_s > 0 else None,
                cluster_share=round(float(np.median(spans["cluster_ms"])) / kernel, 4) if kernel > 0 else None, call_ms=spread(walls),
                numpy_restatement_s=None if numpy_s is None else round(numpy_s, 2),
                numpy_over_kernel=None if numpy_s is None or kernel <= 0 else round(numpy_s * 1e3 / kernel, 0),
                library=os.path.basename(os.environ.get("TIMED_HIP_LIB", "libtimedhip.so")), **{k: spread(v) for k, v in spans.items()})
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", type=str, nargs="*", default=["1x1000x300", "1x10000x300", "100x1000x300", "1x1000x3000"], help="SETSxNxL")
    ap.add_argument("--mutate", type=float, default=0.5)
    ap.add_argument("--cluster_identity", type=float, default=0.9)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-check", action="store_true", help="skip the NumPy restatement of the first workload")
    ap.add_argument("--build-variant", type=str, nargs="+", default=None, metavar=("NAME", "FLAG"), help="build a library with these compiler flags and leave")
    ap.add_argument("--out", type=str, default=None, help="append the JSON lines to this file")
    a, flags = ap.parse_known_args()
    if a.build_variant:
        return build_variant(a.build_variant[0], a.build_variant[1:] + flags)
    if flags:
        ap.error(f"unknown arguments {flags}")
    import seqset_restatement as qr
    from timed_hip import seqset
    for k, shape in enumerate(a.shapes):
        workload(qr, seqset, tuple(int(v) for v in shape.split("x")), a, check=k == 0 and not a.no_check)


if __name__ == "__main__":
    main()
