"""th_superpose on the GPU against the NumPy restatement (tests/superpose_restatement.py) and the committed fixture: the five cases on
the CA atoms of 1ubq, a ragged batch of every size at which the kernel's lane layout changes, degenerate geometry, cycles = 0 and the
optional transform, ABI errors, and superpose() / analyse_models.py / calculate_RMSD_and_gdt end to end.

Integer outputs — the kept bytes and the counts — must be exact.  That is fair only if no decision sits on an edge, so each test first
asserts ON THE RESTATEMENT that no d_i lies within 1e-9 Angstrom of 1, 2, 4, 8 or of a cycle's cutoff * rms, and that the two largest
eigenvalues of Horn's matrix differ by more than 1e-6 of the largest.  The distances and RMSDs have a MEASURED tolerance: the float64
restatement's own worst error against the same rule in np.longdouble is measured on the data of the test, and the GPU is allowed 64
times that (the margin covers a device sqrt or division a few ulp off, the wave's summation order and a different but converged
Jacobi sweep).  Each test prints its figures before it asserts; profiles/superpose.txt records them.
"""
import csv
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import superpose_restatement as sr  # noqa: E402
from timed_hip import _lib, superpose  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 64
EDGE, GAP = 1e-9, 1e-6


@pytest.fixture(scope="module")
def golden():
    return np.load(sr.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return sr.ubq_cases()


@pytest.fixture(scope="module")
def ragged():
    """the ragged batch, its float64 and long double restatements pair by pair: computed once, shared, never changed"""
    pairs = sr.ragged_batch()
    return pairs, [sr.restate(r, m) for r, m in pairs], [sr.restate(r, m, dtype=np.longdouble) for r, m in pairs]


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_result(a, b):
    return all((x is None and y is None) or same_bytes(x, y) for x, y in zip(a, b))


def worst(a, b):
    """largest |a - b| over the entries where b is a number (NaN must sit in the same places)"""
    a, b = np.asarray(a, dtype=np.longdouble).ravel(), np.asarray(b, dtype=np.longdouble).ravel()
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.nanmax(np.abs(a - b))) if np.isfinite(b).any() else 0.0


def check(what, got, float64, exact):
    """``got`` / ``float64`` / ``exact``: (dist, rmsd) of the GPU, the float64 and the long double restatement.  ONE tolerance for
    the data of a test: 64 times the float64 restatement's worst error in any d_i or RMSD of it."""
    own = max(worst(f, e) for f, e in zip(float64, exact))
    mine = [worst(g, e) for g, e in zip(got, exact)]
    print(f"{what}: float64 restatement vs long double {own:.3e} Angstrom; GPU vs long double: d_i {mine[0]:.3e}, RMSD {mine[1]:.3e}; "
          f"allowed {MARGIN * own:.3e}")
    assert own > 0 and max(mine) <= MARGIN * own, (what, own, mine)


def test_ubq_cases_equal_the_fixture(gpu, golden, cases):
    assert str(golden["sha256"]) == sr.inputs_sha256(cases)
    exact = {name: sr.restate(*cases[name], cycles=sr.CASE_CYCLES[name], dtype=np.longdouble) for name in sr.CASES}
    for name in sr.CASES:                                                       # the condition on the inputs
        res = sr.restate(*cases[name], cycles=sr.CASE_CYCLES[name])
        assert res["edge"] > EDGE and res["gap"] > GAP, (name, res["edge"], res["gap"])
        assert same_bytes(res["kept"], exact[name]["kept"]) and same_bytes(res["counts"], exact[name]["counts"])
    refined = [name for name in sr.CASES if sr.CASE_CYCLES[name] == 5]
    ref, mob, offsets = sr.flatten([cases[name] for name in refined])
    got = superpose.superpose_arrays(ref, mob, offsets, device=gpu)
    rigid = superpose.superpose_arrays(*cases["rigid"], [0, 76], cycles=0, device=gpu)
    results = {name: (got.dist[76 * k:76 * k + 76], got.kept[76 * k:76 * k + 76], got.rmsd[k], got.counts[k]) for k, name in enumerate(refined)}
    results["rigid"] = (rigid.dist, rigid.kept, rigid.rmsd[0], rigid.counts[0])
    for name in sr.CASES:
        dist, kept, rmsd, counts = results[name]
        print(name, "rmsd kept / all / fit_all", rmsd.tolist(), "counts", counts.tolist())
        assert same_bytes(kept, golden[f"{name}_kept"]) and same_bytes(counts, golden[f"{name}_counts"]), name
    cat = lambda pick: np.concatenate([pick(name).ravel() for name in sr.CASES])                                  # noqa: E731
    check("1ubq cases", (cat(lambda n: results[n][0]), cat(lambda n: results[n][2])), (cat(lambda n: golden[f"{n}_dist"]), cat(lambda n: golden[f"{n}_rmsd"])),
          (cat(lambda n: exact[n]["dist"]), cat(lambda n: exact[n]["rmsd"])))
    assert results["rigid"][2][2] < 1e-12
    assert results["noise"][3][:3].tolist() == [76, 76, 0]                      # sigma = 0.5: nothing is rejected
    assert results["hinge"][3][2] >= 2 and results["hinge"][2][0] < 0.6 and results["hinge"][2][2] > 2.0
    mirror = results["mirror"][2][2]
    assert 10.6 < mirror < 10.8 and abs(mirror - sr.kabsch_rmsd(*cases["mirror"])) < 1e-9           # a proper rotation: not 0
    dist, kept, _, counts = results["invalid"]
    assert counts[0] == 73 and np.isnan(dist[[3, 11, 40]]).all() and not kept[[3, 11, 40]].any() and np.isfinite(np.delete(dist, [3, 11, 40])).all()
    nothing = superpose.superpose_arrays(np.full((5, 3), np.nan), np.ones((5, 3)), [0, 5, 5], device=gpu, transform=True)
    assert np.isnan(nothing.rmsd).all() and not nothing.counts.any() and np.isnan(nothing.dist).all() and not nothing.kept.any()
    assert same_bytes(nothing.transform, np.tile(np.eye(3, 4), (2, 1, 1)))


def test_ragged_batch_equals_the_restatement_and_each_pair_alone(gpu, ragged):
    pairs, float64, exact = ragged
    sizes = [len(r) for r, _ in pairs]
    assert sorted(set(sizes)) == list(sr.SIZES) and len(pairs) == 39 and sizes != sorted(sizes)
    full = [k for k, n in enumerate(sizes) if n >= 3]                           # below 3 positions the rotation is not unique
    for k in full:
        assert float64[k]["edge"] > EDGE and float64[k]["gap"] > GAP, (sizes[k], float64[k]["edge"], float64[k]["gap"])
    assert sum(int(float64[k]["counts"][2]) > 0 for k in full) > 20              # the planted outliers are rejected
    ref, mob, offsets = sr.flatten(pairs)
    got = superpose.superpose_arrays(ref, mob, offsets, device=gpu, transform=True)
    for k, n in enumerate(sizes):
        a, b = int(offsets[k]), int(offsets[k + 1])
        if n >= 3:
            assert same_bytes(got.kept[a:b], float64[k]["kept"]) and same_bytes(got.counts[k], float64[k]["counts"]), (k, n)
        else:
            assert got.counts[k].tolist()[:3] == [n, n, 0] and got.kept[a:b].all() and np.isfinite(got.dist[a:b]).all()
    cat = lambda parts, key, keep: np.concatenate([parts[k][key].ravel() for k in keep])                          # noqa: E731
    mine = np.concatenate([got.dist[offsets[k]:offsets[k + 1]] for k in full])
    check("ragged batch", (mine, got.rmsd[np.array(sizes) > 0]), (cat(float64, "dist", full), cat(float64, "rmsd", [k for k, n in enumerate(sizes) if n])),
          (cat(exact, "dist", full), cat(exact, "rmsd", [k for k, n in enumerate(sizes) if n])))
    again = superpose.superpose_arrays(ref, mob, offsets, device=gpu, transform=True)
    assert same_result(got, again)                                              # a second run: the same bytes
    for k, (r, m) in enumerate(pairs):                                          # a pair alone: the same bytes as in the batch
        a, b = int(offsets[k]), int(offsets[k + 1])
        alone = superpose.superpose_arrays(r, m, [0, len(r)], device=gpu, transform=True)
        assert same_bytes(alone.dist, got.dist[a:b]) and same_bytes(alone.kept, got.kept[a:b]), (k, len(r))
        assert same_bytes(alone.rmsd[0], got.rmsd[k]) and same_bytes(alone.counts[0], got.counts[k]) and same_bytes(alone.transform[0], got.transform[k])
    empty = [k for k, n in enumerate(sizes) if n == 0]
    assert np.isnan(got.rmsd[empty]).all() and not got.counts[empty].any()


def test_degenerate_geometry_gives_the_unique_rmsd_and_finite_outputs(gpu):
    pairs = sr.degenerate_pairs()
    assert [len(r) for r, _ in pairs] == [1, 2, 2, 5, 40]
    float64 = [sr.restate(r, m, cycles=0) for r, m in pairs]
    exact = [sr.restate(r, m, cycles=0, dtype=np.longdouble) for r, m in pairs]
    ref, mob, offsets = sr.flatten(pairs)
    got = superpose.superpose_arrays(ref, mob, offsets, cycles=0, device=gpu, transform=True)
    assert np.isfinite(got.dist).all() and np.isfinite(got.rmsd).all() and np.isfinite(got.transform).all() and got.kept.all()
    assert got.counts[:, 0].tolist() == [1, 2, 2, 5, 40] and got.rmsd[0].tolist() == [0.0, 0.0, 0.0]
    rmsd64, rmsd_exact = np.array([f["rmsd"] for f in float64]), np.array([e["rmsd"] for e in exact])
    own, mine = worst(rmsd64, rmsd_exact), worst(got.rmsd, rmsd_exact)                              # only the RMSDs: the rotation is not unique
    print(f"degenerate RMSD: float64 restatement vs long double {own:.3e} Angstrom, GPU vs long double {mine:.3e}, allowed {MARGIN * own:.3e}")
    assert own > 0 and mine <= MARGIN * own
    for k, (r, m) in enumerate(pairs[1:], 1):
        assert abs(got.rmsd[k, 2] - sr.kabsch_rmsd(r, m)) < 1e-9
    refined = superpose.superpose_arrays(ref, mob, offsets, device=gpu, transform=True)             # with refinement: still finite
    assert np.isfinite(refined.dist).all() and np.isfinite(refined.rmsd).all() and np.isfinite(refined.transform).all()
    assert refined.counts[:3, 2].tolist() == [0, 0, 0] and same_bytes(refined.rmsd[:3], got.rmsd[:3])


def test_cycles_zero_and_the_optional_transform(gpu, cases):
    names = ("noise", "hinge", "mirror")
    ref, mob, offsets = sr.flatten([cases[name] for name in names])
    once = superpose.superpose_arrays(ref, mob, offsets, cycles=0, device=gpu)
    assert same_bytes(once.rmsd[:, 0], once.rmsd[:, 1]) and same_bytes(once.rmsd[:, 0], once.rmsd[:, 2])
    assert once.kept.all() and (once.counts[:, 2] == 0).all() and once.transform is None
    for k, name in enumerate(names):
        assert abs(once.rmsd[k, 2] - sr.kabsch_rmsd(*cases[name])) < 1e-9
    plain = superpose.superpose_arrays(ref, mob, offsets, device=gpu)
    moved = superpose.superpose_arrays(ref, mob, offsets, device=gpu, transform=True)
    assert same_result(plain[:4], moved[:4]) and moved.transform.shape == (3, 3, 4)                 # transform_out = NULL: the same other bytes
    exact = [sr.restate(*cases[name], dtype=np.longdouble) for name in names]
    float64 = [sr.restate(*cases[name]) for name in names]
    applied = []
    for k in range(3):
        R, t = moved.transform[k, :, :3], moved.transform[k, :, 3]
        assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
        lo, hi = offsets[k], offsets[k + 1]
        delta = mob[lo:hi].astype(np.longdouble) @ R.T.astype(np.longdouble) + t.astype(np.longdouble) - ref[lo:hi].astype(np.longdouble)
        applied.append(np.sqrt((delta * delta).sum(axis=1)))
    own = worst(np.concatenate([f["dist"] for f in float64]), np.concatenate([e["dist"] for e in exact]))
    mine = worst(np.concatenate(applied), np.concatenate([e["dist"] for e in exact]))
    print(f"transform applied to mob: float64 restatement d_i vs long double {own:.3e} Angstrom, |R mob + t - ref| vs long double {mine:.3e}, "
          f"allowed {MARGIN * own:.3e}")
    assert own > 0 and mine <= MARGIN * own
    fewer = superpose.superpose_arrays(ref, mob, offsets, cycles=1, device=gpu)
    assert (fewer.counts[:, 2] <= 1).all() and fewer.counts[1, 2] == 1 and fewer.counts[1, 1] > plain.counts[1, 1]
    tight = superpose.superpose_arrays(ref, mob, offsets, cutoff=1.5, device=gpu)
    want = sr.restate(*cases["hinge"], cutoff=1.5)
    assert want["edge"] > EDGE and same_bytes(tight.kept[76:152], want["kept"]) and same_bytes(tight.counts[1], want["counts"])


def test_abi_errors_return_einval_and_leave_the_outputs_untouched(gpu, lib, cases):
    ref, mob, offsets = sr.flatten([cases["noise"], cases["hinge"]])
    total = len(ref)
    decreasing = np.array([0, 80, 79], np.int64)
    short = np.array([0, 76, total - 1], np.int64)
    late = np.array([1, 76, total], np.int64)
    bad_calls = {
        "negative total": dict(total=-1), "negative n_pairs": dict(n_pairs=-1), "total too large": dict(total=1 << 31),
        "n_pairs too large": dict(n_pairs=1 << 31), "ref NULL": dict(ref=None), "mob NULL": dict(mob=None), "offsets NULL": dict(offsets=None),
        "dist NULL": dict(dist=None), "kept NULL": dict(kept=None), "rmsd NULL": dict(rmsd=None), "counts NULL": dict(counts=None),
        "offsets decrease": dict(offsets=decreasing), "offsets end before total": dict(offsets=short), "offsets start late": dict(offsets=late),
        "offsets end past total": dict(total=total - 1), "cycles negative": dict(cycles=-1), "cutoff zero": dict(cutoff=0.0),
        "cutoff negative": dict(cutoff=-2.0), "cutoff NaN": dict(cutoff=float("nan")), "cutoff infinite": dict(cutoff=float("inf")),
    }

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def fresh():
        return dict(dist=np.full(total, 6.5), kept=np.full(total, 9, np.uint8), rmsd=np.full((2, 3), 6.5), counts=np.full((2, 7), 12345, np.int32),
                    moves=np.full((2, 12), 6.5))

    def call(out, ref=ref, mob=mob, total=total, offsets=offsets, n_pairs=2, cycles=5, cutoff=2.0, **replaced):
        o = dict(out, **replaced)
        ms = C.c_double(-1.0)
        rc = lib.th_superpose(gpu, ptr(ref), ptr(mob), total, ptr(offsets), n_pairs, cycles, cutoff, ptr(o["dist"]), ptr(o["kept"]), ptr(o["rmsd"]),
                              ptr(o["counts"]), ptr(o["moves"]), C.byref(ms))
        return rc, ms.value
    for what, change in bad_calls.items():
        out = fresh()
        rc, ms = call(out, **change)
        assert rc == _lib.TH_EINVAL, what
        assert b"th_superpose" in lib.th_last_error(), what
        assert (out["dist"] == 6.5).all() and (out["kept"] == 9).all() and (out["rmsd"] == 6.5).all() and (out["counts"] == 12345).all(), what
        assert (out["moves"] == 6.5).all() and ms == -1.0, what
    out = fresh()
    rc, ms = call(out)
    assert rc == _lib.TH_OK and ms > 0
    want = superpose.superpose_arrays(ref, mob, offsets, device=gpu, transform=True)
    assert same_bytes(out["dist"], want.dist) and same_bytes(out["kept"], want.kept) and same_bytes(out["counts"], want.counts)
    assert same_bytes(out["moves"].reshape(2, 3, 4), want.transform)
    assert lib.th_superpose(gpu, None, None, 0, None, 0, 5, 2.0, None, None, None, None, None, None) == _lib.TH_OK            # n_pairs = 0
    with pytest.raises(_lib.TimedHipError) as err:
        superpose.superpose_arrays(ref, mob, offsets, cycles=-3, device=gpu)
    assert err.value.code == _lib.TH_EINVAL


def test_files_cli_and_the_reference_name_end_to_end(gpu, golden, cases, tmp_path, capsys):
    from design_utils import analyse_utils as au
    import analyse_models
    names = ("rigid", "noise", "hinge", "mirror")
    (tmp_path / "models" / "deep").mkdir(parents=True)
    (tmp_path / "native.pdb").write_text(sr.pdb_text(cases["hinge"][0]))
    for name in names:
        (tmp_path / "models" / "deep" / f"{name}.pdb").write_text(sr.pdb_text(cases[name][1]))
    ok = np.isfinite(cases["invalid"][0]).all(axis=1) & np.isfinite(cases["invalid"][1]).all(axis=1)
    (tmp_path / "native_73.pdb").write_text(sr.pdb_text(cases["invalid"][0][ok]))
    (tmp_path / "models" / "invalid.pdb").write_text(sr.pdb_text(cases["invalid"][1][ok]))
    native = np.round(cases["hinge"][0], 3)
    listed = [(tmp_path / "native.pdb", tmp_path / "models" / "deep" / f"{name}.pdb") for name in names] + [(tmp_path / "native_73.pdb", tmp_path / "models" / "invalid.pdb"),
                                                                                                             (tmp_path / "native.pdb", tmp_path / "models" / "invalid.pdb")]
    stats = {}
    results = superpose.superpose(listed, device=gpu, stats=stats)
    assert stats["submissions"] == 1 and stats["files_parsed"] == 7 and stats["kernel_ms"] > 0
    arrays = [(native, np.round(cases[name][1], 3)) for name in names] + [(np.round(cases["invalid"][0][ok], 3), np.round(cases["invalid"][1][ok], 3))]
    want = superpose.superpose_arrays(*sr.flatten(arrays), device=gpu)
    for k, res in enumerate(results[:5]):
        lo, hi = 76 * k, 76 * k + len(res.dist)
        assert res.error is None and same_bytes(res.dist, want.dist[lo:hi]) and same_bytes(res.kept, want.kept[lo:hi])
        assert [res.rmsd_kept, res.rmsd_all, res.rmsd_fit_all] == want.rmsd[k].tolist()
        assert [res.n_valid, res.n_kept, res.cycles_run] == want.counts[k, :3].tolist() and res.sequence_identity == 1.0
        assert res.gdt == tuple(c / res.n_valid for c in want.counts[k, 3:].tolist())
    assert "length mismatch" in results[5].error
    # three decimals move the hinge case by less than 1e-3 Angstrom; its decisions stay those of the fixture
    hinge = results[2]
    assert same_bytes(hinge.kept, golden["hinge_kept"]) and abs(hinge.rmsd_kept - golden["hinge_rmsd"][0]) < 1e-3
    rmsd, mean_gdt = au.calculate_RMSD_and_gdt(tmp_path / "native.pdb", tmp_path / "models" / "deep" / "hinge.pdb", device=gpu)
    assert (rmsd, mean_gdt) == (hinge.rmsd_kept, hinge.mean_gdt) and mean_gdt == float(np.mean([c / 76 for c in golden["hinge_counts"][3:].tolist()]))
    # both input forms of the command line: one row per pair, one row per position
    out = tmp_path / "out"
    parser = analyse_models.build_parser()
    analyse_models.main(parser.parse_args(["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models", str(tmp_path / "models"),
                                           "--path_to_output", str(out), "--device", str(gpu)]))
    assert "5 pairs (1 with an error), 304 positions, 6 files parsed in 1 GPU submission(s)" in capsys.readouterr().out

    def read(name):
        with open(out / name, newline="") as f:
            return list(csv.reader(f))
    scores, per = read("model_scores.csv"), read("residue_deviation.csv")
    assert scores[0] == analyse_models.SCORE_COLUMNS and [r[0] for r in scores[1:]] == ["deep/hinge.pdb", "deep/mirror.pdb", "deep/noise.pdb", "deep/rigid.pdb", "invalid.pdb"]
    assert per[0] == analyse_models.RESIDUE_COLUMNS and len(per) == 1 + 4 * 76
    row = dict(zip(scores[0], scores[1]))
    assert float(row["rmsd_kept"]) == hinge.rmsd_kept and float(row["mean_gdt"]) == hinge.mean_gdt and int(row["n_kept"]) == hinge.n_kept
    assert [float(r[3]) for r in per[1:77]] == hinge.dist.tolist() and [int(r[4]) for r in per[1:77]] == hinge.kept.tolist()
    assert "length mismatch" in scores[5][-1]
    (tmp_path / "pairs.csv").write_text("native.pdb,models/deep/hinge.pdb,h\nnative_73.pdb,models/invalid.pdb\n")
    analyse_models.main(parser.parse_args(["--pairs", str(tmp_path / "pairs.csv"), "--path_to_output", str(out), "--device", str(gpu), "--pair_by", "number"]))
    scores, per = read("model_scores.csv"), read("residue_deviation.csv")
    assert [r[0] for r in scores[1:]] == ["h", "models/invalid.pdb"] and len(per) == 1 + 76 + 73
    assert scores[1][3:] == [str(v) for v in row.values()][3:]                  # numbered alike: pairing by number gives the same row
    assert float(scores[2][6]) == results[4].rmsd_kept
