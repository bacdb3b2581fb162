"""The host-side batch driver (timed_hip/batching.py) and the parse-once entry of the pair scorers (superpose.prepare), without a
GPU: the greedy cut at an explicit cost per unit, the runner's submissions and stats, the thread-pool map, and both scorers on one
prepared set with the kernel calls replaced by the restatements the other host tests use."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lddt_restatement as lr  # noqa: E402
import superpose_restatement as sr  # noqa: E402
from timed_hip import _lib, analysis, batching, lddt, structure, superpose  # noqa: E402

PER = structure._ATOM_BYTES
CUT_CASES = [([], 100, []), ([10, 10, 10], 1 << 20, [(0, 3)]), ([10, 10, 10], 20 * PER, [(0, 2), (2, 3)]),
             ([50, 1, 1, 50, 0], 10 * PER, [(0, 1), (1, 3), (3, 4), (4, 5)]), ([0, 0, 0], 1, [(0, 3)])]


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restated_superposition(ref_xyz, mob_xyz, offsets, cycles=5, cutoff=2.0, device=0, transform=False, timing=None):
    """superpose.superpose_arrays with the GPU call replaced by its restatement, as in test_superpose_host.py"""
    dist, kept, rmsd, counts, moves, _, _ = sr.restate_batch(ref_xyz, mob_xyz, np.asarray(offsets), cycles, cutoff)
    return superpose.Superposed(dist, kept, rmsd, counts, moves.reshape(-1, 3, 4) if transform else None)


def restated_lddt(ref_xyz, mob_xyz, offsets, radius=15.0, thresholds=lr.THRESHOLDS, device=0, timing=None):
    """lddt.lddt_arrays with the GPU call replaced by its restatement, as in test_lddt_host.py"""
    residue, pair, _ = lr.restate_batch(ref_xyz, mob_xyz, offsets, radius, thresholds)
    return lddt.LddtTables(residue, pair)


def labels(residues):
    return [(r.chain, r.number, r.name) for r in residues]


def test_cut_batches_takes_the_cost_per_unit_as_an_argument():
    assert PER == 3 * 8 + 4 + 1 + 4 and structure.BATCH_BYTES == batching.BATCH_BYTES == 256 << 20
    for sizes, budget, runs in CUT_CASES:
        assert batching.cut_batches(sizes, budget, PER) == runs
        assert structure.cut_batches(sizes, budget) == runs
    rng = np.random.default_rng(11)
    sizes = rng.integers(0, 40, 200).tolist()
    sizes[17], sizes[60], sizes[61], sizes[140] = 0, 0, 0, 500                  # zeros, and one size above the budget
    budget = 100 * PER
    runs = batching.cut_batches(sizes, budget, PER)
    assert structure.cut_batches(sizes, budget) == runs and (140, 141) in runs
    assert [lo for lo, _ in runs] == [0] + [hi for _, hi in runs[:-1]] and runs[-1][1] == 200          # consecutive, complete
    for k, (lo, hi) in enumerate(runs):
        assert sum(sizes[lo:hi]) * PER <= budget or hi == lo + 1
        if k + 1 < len(runs):
            assert (sum(sizes[lo:hi]) + sizes[hi]) * PER > budget                                      # greedy: the next one did not fit
    # the cost is in bytes: the same sizes at another cost per unit are the same cuts at the scaled budget
    assert batching.cut_batches(sizes, 100 * 68, 68) == runs
    assert batching.cut_batches([30] * 5, 2 * 30 * 68 + 100, 68) == [(0, 2), (2, 4), (4, 5)]


def test_run_batches_submits_the_runs_in_order_and_adds_up_the_stats():
    items = [f"item{k}" for k in range(7)]
    sizes = [3, 3, 3, 9, 0, 1, 1]
    seen = []

    def submit(part, timing):
        seen.append(list(part))
        if timing is not None:
            timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + 0.25
    stats = {}
    assert batching.run_batches(items, sizes, 6 * PER, PER, submit, stats) is None
    runs = batching.cut_batches(sizes, 6 * PER, PER)
    assert runs == [(0, 2), (2, 3), (3, 4), (4, 7)] and seen == [items[lo:hi] for lo, hi in runs]
    assert stats == {"submissions": 4, "kernel_ms": 1.0}
    batching.run_batches(items, sizes, 1 << 20, PER, submit, stats)             # the same dict again: the values add up
    assert seen[4:] == [items] and stats == {"submissions": 5, "kernel_ms": 1.25}
    del seen[:]
    batching.run_batches(items, sizes, 6 * PER, PER, submit, None)              # nobody asks: no timing dict either
    assert len(seen) == 4
    del seen[:]
    batching.run_batches([], [], 100, PER, submit, stats)
    assert seen == [] and stats == {"submissions": 5, "kernel_ms": 1.25}
    empty = {}
    batching.run_batches([], [], 100, PER, submit, empty)
    assert empty == {"submissions": 0, "kernel_ms": 0.0}


def test_parse_each_keeps_order_on_at_most_sixteen_threads(monkeypatch):
    gate = threading.Barrier(16, timeout=20)
    pool, sized = batching.ThreadPoolExecutor, []
    monkeypatch.setattr(batching, "ThreadPoolExecutor", lambda max_workers: sized.append(max_workers) or pool(max_workers=max_workers))

    def fn(k):
        if k < 16:
            gate.wait()                                                        # sixteen calls are in flight at once ...
        return threading.get_ident(), k * k
    got = batching.parse_each(fn, range(64), 1000)
    assert [v for _, v in got] == [k * k for k in range(64)]
    assert len({ident for ident, _ in got}) == 16 and sized == [16]            # ... and never a seventeenth thread
    main = threading.get_ident()
    alone = batching.parse_each(lambda k: (threading.get_ident(), -k), [3, 1, 2], 0)
    assert [v for _, v in alone] == [-3, -1, -2] and len({ident for ident, _ in alone}) == 1 and alone[0][0] != main
    assert sized == [16, 1]
    assert batching.parse_each(fn, [], 8) == [] and batching.parse_each(fn, iter(()), 8) == [] and sized == [16, 1]      # no pool for nothing

    def broken(k):
        if k == 2:
            raise KeyError("two")
        return k
    with pytest.raises(KeyError, match="two"):
        batching.parse_each(broken, range(4), 4)


def test_prepare_reads_and_pairs_once_for_both_scores(tmp_path, monkeypatch):
    monkeypatch.setattr(superpose, "superpose_arrays", restated_superposition)
    monkeypatch.setattr(lddt, "lddt_arrays", restated_lddt)
    cases = sr.ubq_cases()
    ref, hinge = cases["hinge"]
    (tmp_path / "native.pdb").write_text(sr.pdb_text(ref))
    (tmp_path / "hinge.pdb").write_text(sr.pdb_text(hinge))
    (tmp_path / "noise.pdb").write_text(sr.pdb_text(cases["noise"][1]))
    (tmp_path / "short.pdb").write_text(sr.pdb_text(hinge[:70]))
    names = ["hinge.pdb", "short.pdb", "absent.pdb", "noise.pdb", "hinge.pdb"]
    pairs = [(tmp_path / "native.pdb", tmp_path / name) for name in names]
    for pair_by in superpose.PAIR_BY:
        raw_fit, raw_score = superpose.superpose(pairs, pair_by=pair_by), lddt.lddt(pairs, pair_by=pair_by)
        reads, pairings = [], []
        first_model, pair_positions = structure.first_model, superpose.pair_positions
        with monkeypatch.context() as m:
            m.setattr(structure, "first_model", lambda path: reads.append(str(path)) or first_model(path))
            m.setattr(superpose, "pair_positions", lambda *a: pairings.append(a[2]) or pair_positions(*a))
            prepared = superpose.prepare(pairs, pair_by, "CA", 4)
            stats = {}
            fit = superpose.superpose(prepared, stats=stats)
            assert stats["files_parsed"] == 5 and stats["submissions"] == 1
            score = lddt.lddt(prepared, stats=stats)
        assert sorted(reads) == sorted(str(tmp_path / name) for name in set(names) | {"native.pdb"})     # every file once, the absent one tried once
        assert pairings == [pair_by] * 4                                           # once per pair that has both its files
        assert prepared.files == 5 and stats["files_parsed"] == 5 and stats["submissions"] == 2 and "kernel_ms" in stats
        other = {}
        lddt.lddt(prepared, stats=other)                                           # another dict has not counted them yet
        assert other["files_parsed"] == 5 and other["submissions"] == 1
        assert superpose.prepare(prepared) is prepared
        for a, b in zip(raw_fit, fit):
            assert a.error == b.error and same_bytes(a.dist, b.dist) and same_bytes(a.kept, b.kept) and labels(a.residues) == labels(b.residues)
            assert repr((a.n_valid, a.n_kept, a.cycles_run, a.rmsd_kept, a.rmsd_all, a.rmsd_fit_all, a.gdt, a.mean_gdt, a.sequence_identity)) == \
                repr((b.n_valid, b.n_kept, b.cycles_run, b.rmsd_kept, b.rmsd_all, b.rmsd_fit_all, b.gdt, b.mean_gdt, b.sequence_identity))
            assert (a.unpaired_reference, a.unpaired_model) == (b.unpaired_reference, b.unpaired_model)
        for a, b in zip(raw_score, score):
            assert a.error == b.error and same_bytes(a.lddt_i, b.lddt_i) and same_bytes(a.n_i, b.n_i) and same_bytes(a.model_bfactor, b.model_bfactor)
            assert repr((a.n_valid, a.n_included, a.preserved, a.lddt)) == repr((b.n_valid, b.n_included, b.preserved, b.lddt))
            assert labels(a.residues) == labels(b.residues) and (a.unpaired_reference, a.unpaired_model) == (b.unpaired_reference, b.unpaired_model)
        assert [r.error is None for r in fit] == [True, pair_by == "number", False, True, True]
        assert "absent.pdb" in fit[2].error and "absent.pdb" in score[2].error
    with pytest.raises(ValueError):
        superpose.prepare(pairs, "alignment")


def test_one_pointer_helper():
    assert _lib.ptr(None) is None
    a = np.arange(3.0)
    assert _lib.ptr(a).value == a.ctypes.data
    for module in (analysis, structure, superpose, lddt):
        assert module.ptr is _lib.ptr
