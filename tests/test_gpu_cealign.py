"""th_cealign on the GPU against the NumPy restatement (tests/cealign_restatement.py) and the committed fixture: the six cases on the CA
atoms of 1ubq and a helix against a strand, a ragged batch whose two lists have different lengths, a path of 69 fragments, gap_max 0
and 31, another d0 and d1, ABI errors, and cealign() / analyse_models.py --cealign / --pair_by_cealign end to end.

align_out and count_out must be exact.  That is fair only if no decision sits on an edge, so each test first asserts ON THE
RESTATEMENT that every margin it reports — S against d0, c and the step score against d1, the best c against the second best, the
candidate order at rank 20 / 21, the winner's RMSD against the runner-up's — exceeds 1e-9.  The RMSD has a MEASURED tolerance: the
float64 restatement's own worst error against the same rule in np.longdouble is measured on the data of the test, and the GPU is
allowed 64 times that (the margin of tests/test_gpu_superpose.py: a device sqrt or division a few ulp off, a different but
converged Jacobi sweep).  The rigid and the mirror case have scores at rounding level, where ties are
legitimate: they are checked by SELF-CONSISTENCY only.  Each test prints its figures before it asserts; profiles/cealign.txt records
them.
"""
import csv
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cealign_restatement as cr  # noqa: E402
import superpose_restatement as sr  # noqa: E402
from timed_hip import _lib, cealign  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 64
EDGE = 1e-9
LD = np.longdouble


@pytest.fixture(scope="module")
def golden():
    return np.load(cr.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return cr.ubq_cases()


@pytest.fixture(scope="module")
def restated(cases):
    """the float64 restatement of every case and the long double one of the noisy cases: computed once, shared, never changed"""
    return {name: (cr.restate(*cases[name]), cr.restate(*cases[name], dtype=LD) if name in cr.NOISY else None) for name in cr.CASES}


@pytest.fixture(scope="module")
def ragged():
    """the ragged batch, its float64 and long double restatements pair by pair: computed once, shared, never changed"""
    pairs = cr.ragged_batch()
    return pairs, [cr.restate(r, m) for r, m in pairs], [cr.restate(r, m, dtype=LD) for r, m in pairs]


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_result(a, b):
    return all((x is None and y is None) or same_bytes(x, y) for x, y in zip(a, b))


def conditioned(what, float64, exact):
    """The condition on a test's inputs, asserted on the restatement, and the measured tolerance of its data: 64 times the float64
    restatement's worst RMSD error against long double."""
    for f, e in zip(float64, exact):
        assert cr.smallest_margin(f) > EDGE, (what, f["counts"].tolist(), f["margins"])
        assert same_bytes(f["counts"], e["counts"]) and same_bytes(f["align"], e["align"]), (what, f["counts"], e["counts"])
    aligned = [(f, e) for f, e in zip(float64, exact) if f["counts"][3] > 0]
    own = max(abs(float(LD(f["rmsd"]) - e["rmsd"])) for f, e in aligned)
    worst = {name: min(f["margins"][name] for f in float64) for name in cr.MARGINS}
    print(f"{what}: smallest margins " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f"; float64 restatement vs long double: rmsd {own:.3e} "
          f"Angstrom ({len(aligned)} of {len(float64)} pairs aligned)")
    assert own > 0
    return MARGIN * own


def check_against(what, got, float64, exact, tol, ref_offsets):
    worst = 0.0
    for k, (f, e) in enumerate(zip(float64, exact)):
        a, b = int(ref_offsets[k]), int(ref_offsets[k + 1])
        assert same_bytes(got.counts[k], f["counts"]), (what, k, got.counts[k], f["counts"])
        assert same_bytes(got.align[a:b], f["align"]), (what, k)
        if f["counts"][3] == 0:
            assert np.isnan(got.scores[k]).all() and same_bytes(got.transform[k], np.eye(3, 4)), (what, k)
            continue
        assert got.scores[k, 1] == float(f["score"]), (what, k, got.scores[k, 1], float(f["score"]))          # the same sums in the same order
        worst = max(worst, abs(float(LD(got.scores[k, 0]) - e["rmsd"])))
    print(f"{what}: GPU rmsd vs long double {worst:.3e} Angstrom, allowed {tol:.3e}")
    assert worst <= tol, (what, worst, tol)


def self_consistent(what, ref, mob, align, scores, transform, tol):
    """transform_out applied to the aligned model positions in long double reproduces the RMSD; R is a proper rotation"""
    R = transform[:, :3]
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12, what
    applied = float(cr.applied_rmsd(ref, mob, align, transform))
    print(f"{what}: rmsd_out {scores[0]!r}, |R mob + t - ref| over the aligned positions in long double {applied!r} (allowed difference {tol:.3e})")
    assert abs(applied - scores[0]) <= tol, (what, applied, scores[0])


def test_ubq_cases_equal_the_fixture(gpu, golden, cases, restated):
    assert str(golden["sha256"]) == cr.inputs_sha256(cases)
    noisy64, noisy_exact = [restated[n][0] for n in cr.NOISY], [restated[n][1] for n in cr.NOISY]
    tol = conditioned("1ubq noisy cases", noisy64, noisy_exact)
    for name in cr.CASES:
        f = restated[name][0]
        assert same_bytes(f["counts"], golden[f"{name}_counts"]) and same_bytes(f["align"], golden[f"{name}_align"]), name
    ref, ro, mob, mo = cr.flatten([cases[name] for name in cr.CASES])
    timing = {}
    got = cealign.cealign_arrays(ref, ro, mob, mo, device=gpu, transform=True, timing=timing)
    for k, name in enumerate(cr.CASES):
        print(name, "rmsd, score", got.scores[k].tolist(), "counts", got.counts[k].tolist())
    print("kernel ms", timing["kernel_ms"])
    at = [cr.CASES.index(n) for n in cr.NOISY]
    picked = cealign.CeTables(np.concatenate([got.align[ro[k]:ro[k + 1]] for k in at]), got.scores[at], got.counts[at], got.transform[at])
    check_against("1ubq noisy cases", picked, noisy64, noisy_exact, tol, np.concatenate([[0], np.cumsum([76] * 4)]))
    for k, name in enumerate(cr.CASES):
        a = got.align[ro[k]:ro[k + 1]]
        if name in cr.NOISY:
            assert float(golden[f"{name}_rmsd"][1]) == got.scores[k, 1] and abs(float(golden[f"{name}_rmsd"][0]) - got.scores[k, 0]) <= tol, name
            self_consistent(name, *cases[name], a, got.scores[k], got.transform[k], tol)
    # deletion and insertion: the alignment steps over the gap
    gone = got.align[ro[4]:ro[5]]
    assert got.counts[4].tolist()[:2] == [76, 70] and got.counts[4, 4] == 64 and not (gone[30:36] >= 0).any() and got.scores[4, 0] < 0.5
    more = got.align[ro[5]:ro[6]]
    paired = np.nonzero(more >= 0)[0]
    assert got.counts[5].tolist()[:2] == [76, 86] and set((more[paired] - paired).tolist()) == {0, 10} and got.scores[5, 0] < 0.5
    # helix against strand: no start at all, a result and not an error
    assert got.counts[6].tolist() == [40, 40, 0, 0, 0, 0] and np.isnan(got.scores[6]).all() and (got.align[ro[6]:] == -1).all()
    assert same_bytes(got.transform[6], np.eye(3, 4))


def test_rigid_and_mirror_by_self_consistency(gpu, golden, cases):
    """scores at rounding level, where ties are legitimate: nothing here is compared with the restatement's choice among equals"""
    ref, ro, mob, mo = cr.flatten([cases["rigid"], cases["mirror"]])
    got = cealign.cealign_arrays(ref, ro, mob, mo, device=gpu, transform=True)
    print("rigid, mirror: rmsd, score", got.scores.tolist(), "counts", got.counts.tolist())
    for k, name, least in ((0, "rigid", 9), (1, "mirror", 8)):
        a = got.align[ro[k]:ro[k + 1]]
        paired = np.nonzero(a >= 0)[0]
        assert got.counts[k].tolist()[:3] == [76, 76, int(golden[f"{name}_counts"][2])] and got.counts[k, 5] == 20, name
        assert got.counts[k, 3] >= least and got.counts[k, 4] == 8 * got.counts[k, 3] == len(paired) and (a[paired] == paired).all(), name
        self_consistent(name, *cases[name], a, got.scores[k], got.transform[k], 1e-9)
    assert got.counts[0, 3] == 9 and got.scores[0, 0] < 1e-9 and got.scores[1, 0] > 5.0 and got.scores[0, 1] < 1e-9 and got.scores[1, 1] < 1e-9


def test_ragged_batch_equals_the_restatement_and_each_pair_alone(gpu, ragged):
    pairs, float64, exact = ragged
    sizes = [(len(r), len(m)) for r, m in pairs]
    assert sorted({a for a, _ in sizes}) == list(cr.SIZES) == [0, 7, 8, 9, 15, 16, 17, 24, 63, 64, 65, 76, 129] == sorted({b for _, b in sizes})
    assert len(pairs) == 26 and all(a != b for a, b in sizes) and [a for a, _ in sizes] != sorted(a for a, _ in sizes)
    assert sum(1 for r, m in pairs if not (np.isfinite(r).all() and np.isfinite(m).all())) >= 5
    tol = conditioned("ragged batch", float64, exact)
    ref, ro, mob, mo = cr.flatten(pairs)
    got = cealign.cealign_arrays(ref, ro, mob, mo, device=gpu, transform=True)
    check_against("ragged batch", got, float64, exact, tol, ro)
    assert sum(1 for f in float64 if f["counts"][3] >= 2) >= 5 and sum(1 for f in float64 if f["counts"][3] == 0) >= 4
    for k, (r, m) in enumerate(pairs):
        if float64[k]["counts"][3] > 0:
            self_consistent(f"ragged {sizes[k]}", r, m, got.align[ro[k]:ro[k + 1]], got.scores[k], got.transform[k], tol)
    again = cealign.cealign_arrays(ref, ro, mob, mo, device=gpu, transform=True)
    assert same_result(got, again)                                              # a second run: the same bytes
    for k, (r, m) in enumerate(pairs):                                          # a pair alone: the same bytes as in the batch
        alone = cealign.cealign_arrays(r, [0, len(r)], m, [0, len(m)], device=gpu, transform=True)
        assert same_bytes(alone.align, got.align[ro[k]:ro[k + 1]]) and same_bytes(alone.scores[0], got.scores[k]), (k, sizes[k])
        assert same_bytes(alone.counts[0], got.counts[k]) and same_bytes(alone.transform[0], got.transform[k]), (k, sizes[k])


def test_a_path_of_more_than_64_fragments(gpu):
    """560 positions: the winning path has 69 AFPs — the second register of the kernel's path — and 552 position pairs to fit"""
    ref, mob = cr.long_pair()
    kw = dict(d0=cr.LONG_D0, gap_max=cr.LONG_GAP_MAX)
    float64, exact = [cr.restate(ref, mob, **kw)], [cr.restate(ref, mob, dtype=LD, **kw)]
    tol = conditioned("560 positions", float64, exact)
    assert float64[0]["counts"].tolist() == [560, 557, 560, 69, 552, 20] and float64[0]["path"][0] == (8, 5)
    timing = {}
    got = cealign.cealign_arrays(ref, [0, 560], mob, [0, 557], device=gpu, transform=True, timing=timing, **kw)
    print("560 positions: rmsd, score", got.scores[0].tolist(), "counts", got.counts[0].tolist(), "kernel ms", timing["kernel_ms"])
    check_against("560 positions", got, float64, exact, tol, [0, 560])
    self_consistent("560 positions", ref, mob, got.align, got.scores[0], got.transform[0], tol)
    paired = np.nonzero(got.align >= 0)[0]
    assert (got.align[paired] == paired - 3).all() and paired[0] == 8 and paired[-1] == 559


def test_gap_max_and_d0(gpu, cases):
    names = ("deletion", "insertion", "noise")
    ref, ro, mob, mo = cr.flatten([cases[name] for name in names])
    for what, kw in (("gap_max = 0", dict(gap_max=0)), ("gap_max = 31", dict(gap_max=31)), ("d0 = 2.0", dict(d0=2.0)), ("d1 = 3.0", dict(d1=3.0))):
        float64 = [cr.restate(*cases[name], **kw) for name in names]
        exact = [cr.restate(*cases[name], dtype=LD, **kw) for name in names]
        tol = conditioned(what, float64, exact)
        got = cealign.cealign_arrays(ref, ro, mob, mo, device=gpu, transform=True, **kw)
        print(what, "counts", got.counts.tolist(), "rmsd", got.scores[:, 0].tolist())
        check_against(what, got, float64, exact, tol, ro)
    # without gaps no path crosses the deletion: the winner lies on one side of it
    alone = cealign.cealign_arrays(*cases["deletion"][:1], [0, 76], cases["deletion"][1], [0, 70], gap_max=0, device=gpu)
    shifts = set((np.nonzero(alone.align >= 0)[0] - alone.align[alone.align >= 0]).tolist())
    assert len(shifts) == 1 and alone.counts[0, 3] < 8
    fewer = cealign.cealign_arrays(*cases["noise"][:1], [0, 76], cases["noise"][1], [0, 76], d0=2.0, device=gpu)
    assert fewer.counts[0, 2] < 3029


def test_abi_errors_return_einval_and_leave_the_outputs_untouched(gpu, lib, cases):
    ref, ro, mob, mo = cr.flatten([cases["deletion"], cases["insertion"]])
    nr, nm = len(ref), len(mob)
    long_one = np.zeros((2049, 3))
    one = np.array([0, 2049], np.int64)
    bad_calls = {
        "negative ref_total": dict(ref_total=-1), "negative mob_total": dict(mob_total=-1), "negative n_pairs": dict(n_pairs=-1),
        "ref_total too large": dict(ref_total=1 << 31), "n_pairs too large": dict(n_pairs=1 << 31), "ref NULL": dict(ref=None), "mob NULL": dict(mob=None),
        "ref_offsets NULL": dict(ro=None), "mob_offsets NULL": dict(mo=None), "align NULL": dict(align=None), "scores NULL": dict(scores=None),
        "counts NULL": dict(counts=None), "ref_offsets decrease": dict(ro=np.array([0, 80, 79], np.int64)),
        "mob_offsets end before total": dict(mo=np.array([0, 70, nm - 1], np.int64)), "ref_offsets start late": dict(ro=np.array([1, 76, nr], np.int64)),
        "mob_offsets end past total": dict(mob_total=nm - 1), "d0 zero": dict(d0=0.0), "d0 nan": dict(d0=float("nan")), "d1 negative": dict(d1=-1.0),
        "d1 infinite": dict(d1=float("inf")), "gap_max negative": dict(gap_max=-1), "gap_max 32": dict(gap_max=32),
        "2049 reference positions": dict(ref=long_one, ref_total=2049, ro=one, mo=np.array([0, nm], np.int64), n_pairs=1),
        "2049 model positions": dict(mob=long_one, mob_total=2049, mo=one, ro=np.array([0, nr], np.int64), n_pairs=1),
    }

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def fresh():
        return dict(align=np.full(2049, 12345, np.int32), scores=np.full((2, 2), 6.5), counts=np.full((2, 6), 12345, np.int64), moves=np.full((2, 12), 6.5))

    def call(out, ref=ref, ref_total=nr, ro=ro, mob=mob, mob_total=nm, mo=mo, n_pairs=2, d0=3.0, d1=4.0, gap_max=30, **replaced):
        o = dict(out, **replaced)
        ms = C.c_double(-1.0)
        rc = lib.th_cealign(gpu, ptr(ref), ref_total, ptr(ro), ptr(mob), mob_total, ptr(mo), n_pairs, d0, d1, gap_max, ptr(o["align"]), ptr(o["scores"]),
                            ptr(o["counts"]), ptr(o["moves"]), C.byref(ms))
        return rc, ms.value
    for what, change in bad_calls.items():
        out = fresh()
        rc, ms = call(out, **change)
        assert rc == _lib.TH_EINVAL, what
        assert b"th_cealign" in lib.th_last_error(), what
        assert (out["align"] == 12345).all() and (out["scores"] == 6.5).all() and (out["counts"] == 12345).all() and (out["moves"] == 6.5).all(), what
        assert ms == -1.0, what
    out = fresh()
    rc, ms = call(out)
    assert rc == _lib.TH_OK and ms > 0
    want = cealign.cealign_arrays(ref, ro, mob, mo, device=gpu, transform=True)
    assert same_bytes(out["align"][:nr], want.align) and (out["align"][nr:] == 12345).all() and same_bytes(out["scores"], want.scores)
    assert same_bytes(out["counts"], want.counts) and same_bytes(out["moves"].reshape(2, 3, 4), want.transform)
    out = fresh()                                                               # transform_out left out: the same other bytes
    rc, _ = call(out, moves=None)
    assert rc == _lib.TH_OK and same_bytes(out["align"][:nr], want.align) and same_bytes(out["scores"], want.scores) and same_bytes(out["counts"], want.counts)
    assert (out["moves"] == 6.5).all()
    bare = cealign.cealign_arrays(ref, ro, mob, mo, device=gpu)
    assert bare.transform is None and same_bytes(bare.align, want.align) and same_bytes(bare.scores, want.scores)
    assert lib.th_cealign(gpu, None, 0, None, None, 0, None, 0, 3.0, 4.0, 30, None, None, None, None, None) == _lib.TH_OK        # n_pairs = 0
    empty = cealign.cealign_arrays(np.zeros((0, 3)), [0, 0], np.zeros((0, 3)), [0, 0], device=gpu, transform=True)                 # a pair of nothing
    assert empty.counts.tolist() == [[0] * 6] and np.isnan(empty.scores).all() and same_bytes(empty.transform[0], np.eye(3, 4))
    with pytest.raises(_lib.TimedHipError) as err:
        cealign.cealign_arrays(ref, ro, mob, mo, gap_max=32, device=gpu)
    assert err.value.code == _lib.TH_EINVAL and "gap_max" in str(err.value)


def test_files_and_cli_end_to_end(gpu, cases, tmp_path, capsys):
    import analyse_models
    from design_utils import analyse_utils
    from timed_hip import lddt, superpose, tmscore
    native = cases["deletion"][0]
    (tmp_path / "models").mkdir()
    (tmp_path / "native.pdb").write_text(sr.pdb_text(native))
    (tmp_path / "models" / "deletion.pdb").write_text(sr.pdb_text(cases["deletion"][1], first=201))         # renumbered as well
    (tmp_path / "models" / "insertion.pdb").write_text(sr.pdb_text(cases["insertion"][1]))
    listed = [(tmp_path / "native.pdb", tmp_path / "models" / f"{name}.pdb") for name in ("deletion", "insertion")]
    stats = {}
    results = cealign.cealign(listed, device=gpu, transform=True, stats=stats)
    assert stats["submissions"] == 1 and stats["files_parsed"] == 3 and stats["kernel_ms"] > 0
    rounded = [(np.round(native, 3), np.round(cases[name][1], 3)) for name in ("deletion", "insertion")]
    ref, ro, mob, mo = cr.flatten(rounded)
    want = cealign.cealign_arrays(ref, ro, mob, mo, device=gpu, transform=True)
    for k, res in enumerate(results):                                           # files against arrays of the rounded coordinates: the same bytes
        a = want.align[ro[k]:ro[k + 1]]
        assert res.error is None and [res.rmsd, res.path_score] == want.scores[k].tolist() and same_bytes(res.transform, want.transform[k])
        assert [res.n_ref, res.n_model, res.n_starts, res.n_afps, res.n_aligned, res.n_candidates] == want.counts[k].tolist()
        assert res.reference_index.tolist() == np.nonzero(a >= 0)[0].tolist() and res.model_index.tolist() == a[a >= 0].tolist()
    float64 = [cr.restate(r, m) for r, m in rounded]
    tol = conditioned("files", float64, [cr.restate(r, m, dtype=LD) for r, m in rounded])
    assert [r.n_aligned for r in results] == [int(f["counts"][4]) for f in float64] and results[0].n_aligned == 64
    assert abs(analyse_utils.calculate_cealign_RMSD(*listed[0], device=gpu) - results[0].rmsd) == 0.0
    assert abs(results[0].rmsd - float(float64[0]["rmsd"])) <= tol
    # the command line
    parser = analyse_models.build_parser()
    common = ["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models", str(tmp_path / "models"), "--device", str(gpu)]
    plain, out = tmp_path / "plain", tmp_path / "out"
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(plain)]))
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(out), "--cealign"]))
    assert sorted(p.name for p in plain.iterdir()) == ["model_scores.csv", "residue_deviation.csv"]
    assert sorted(p.name for p in out.iterdir()) == ["model_cealign.csv", "model_scores.csv", "residue_cealign.csv", "residue_deviation.csv"]
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (out / name).read_bytes() == (plain / name).read_bytes()

    def read(folder, name):
        with open(folder / name, newline="") as f:
            return list(csv.reader(f))
    rows = read(out, "model_cealign.csv")
    assert rows[0] == analyse_models.CEALIGN_COLUMNS and [r[0] for r in rows[1:]] == ["deletion.pdb", "insertion.pdb"]
    row = dict(zip(rows[0], rows[1]))
    assert float(row["rmsd"]) == results[0].rmsd and float(row["path_score"]) == results[0].path_score and row["error"] == ""
    assert [int(row[k]) for k in ("n_ref", "n_model", "n_starts", "n_afps", "n_aligned")] == [76, 70, results[0].n_starts, 8, 64]
    residues = [r for r in read(out, "residue_cealign.csv")[1:] if r[0] == "deletion.pdb"]
    assert len(residues) == 76 and sum(1 for r in residues if r[5]) == 64
    for r in residues:
        k = int(r[2]) - 1
        assert (int(r[5]) == 201 + (k if k < 30 else k - 6)) if r[5] else r[4:] == ["", "", "", ""]
    spread = float(np.sqrt(np.mean([float(r[7]) ** 2 for r in residues if r[5]])))
    assert abs(spread - results[0].rmsd) < 1e-9
    today = read(plain, "model_scores.csv")
    assert "length mismatch" in today[1][-1] and "length mismatch" in today[2][-1]
    # the alignment as the pairing of every other score: the deletion model, a length mismatch today, gets scores
    ce = tmp_path / "ce"
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(ce), "--pair_by_cealign", "--tmscore", "--lddt"]))
    assert sorted(p.name for p in ce.iterdir()) == ["model_lddt.csv", "model_scores.csv", "model_tmscore.csv", "residue_deviation.csv", "residue_lddt.csv"]
    scores = read(ce, "model_scores.csv")
    first = dict(zip(scores[0], scores[1]))
    assert first["error"] == "" and first["n_valid"] == "64" and (first["unpaired_reference"], first["unpaired_model"]) == ("12", "6")
    assert abs(float(first["rmsd_fit_all"]) - results[0].rmsd) < 1e-9 and float(first["mean_gdt"]) > 0.9
    tm = dict(zip(*read(ce, "model_tmscore.csv")[:2]))
    ld = dict(zip(*read(ce, "model_lddt.csv")[:2]))
    assert tm["error"] == "" and (tm["n_valid"], tm["norm_length"]) == ("64", "76") and 0.7 < float(tm["tm_score"]) <= 64 / 76
    assert ld["error"] == "" and ld["n_valid"] == "64" and float(ld["lddt"]) > 0.9
    prepared = cealign.prepare_aligned(listed, device=gpu)
    (scored,) = tmscore.tmscore(superpose.Prepared(prepared.pairs[:1], 0, "CA"), device=gpu)
    assert scored.tm == float(tm["tm_score"]) and lddt.lddt(prepared, device=gpu)[0].n_valid == 64
    capsys.readouterr()
