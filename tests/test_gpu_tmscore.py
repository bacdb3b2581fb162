"""th_tmscore on the GPU against the NumPy restatement (tests/tmscore_restatement.py) and the committed fixture: the five cases on the
CA atoms of 1ubq, a ragged batch of every size at which the seed schedule or the lane / mask layout changes, a pair of 4096
positions (the upper words of the mask), norm_len and rounds = 0, ABI errors, and tmscore() / analyse_models.py --tmscore end to end.

Integer outputs — n_valid, L, n_seeds, n_fits — must be exact.  That is fair only if no selection sits on an edge, so each test first
asserts ON THE RESTATEMENT that no d_i lies within 1e-9 Angstrom of a cut and that the two largest eigenvalues of Horn's matrix
differ by more than 1e-6 of the largest in every fit of three positions or more.  tm has a MEASURED tolerance: the float64
restatement's own worst error against the same rule in np.longdouble is measured on the data of the test, and the GPU is allowed 64
times that (the margin of tests/test_gpu_superpose.py: a device sqrt or division a few ulp off, the wave's summation order, a
different but converged Jacobi sweep).  dist_out and transform_out are checked by SELF-CONSISTENCY, not against the restatement's
argmax (two seeds may tie to the last bits): transform_out applied to mob in long double reproduces dist_out within 64 times the
float64 restatement's worst d_i error, and dist_out summed again in long double reproduces tm_out within the tolerance of tm.  Each
test prints its figures before it asserts; profiles/tmscore.txt records them.
"""
import csv
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import superpose_restatement as sr  # noqa: E402
import tmscore_restatement as tr  # noqa: E402
from timed_hip import _lib, superpose, tmscore  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 64
EDGE, GAP = 1e-9, 1e-6
LD = np.longdouble


@pytest.fixture(scope="module")
def golden():
    return np.load(tr.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return sr.ubq_cases()


@pytest.fixture(scope="module")
def restated(cases):
    """the float64 and the long double restatement of the five 1ubq cases: computed once, shared, never changed"""
    return {name: (tr.restate(*cases[name]), tr.restate(*cases[name], dtype=LD)) for name in sr.CASES}


@pytest.fixture(scope="module")
def ragged():
    """the ragged batch, its float64 and long double restatements pair by pair: computed once, shared, never changed"""
    pairs = tr.ragged_batch()
    return pairs, [tr.restate(r, m) for r, m in pairs], [tr.restate(r, m, dtype=LD) for r, m in pairs]


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_result(a, b):
    return all((x is None and y is None) or same_bytes(x, y) for x, y in zip(a, b))


def conditioned(what, float64, exact):
    """The condition on a test's inputs, asserted on the restatement, and the two measured tolerances of its data: 64 times the
    float64 restatement's worst error in tm, and in any d_i of the pairs whose winner is the same in both precisions."""
    scored = [(f, e) for f, e in zip(float64, exact) if f["counts"][0] > 0]
    for f, e in scored:
        assert f["edge"] > EDGE and f["gap"] > GAP, (what, f["counts"].tolist(), f["edge"], f["gap"])
        assert same_bytes(f["counts"], e["counts"]), (what, f["counts"], e["counts"])
    own_tm = max(abs(float(LD(f["tm"]) - e["tm"])) for f, e in scored)
    agreed = [(f, e) for f, e in scored if (f["seed"], f["round"]) == (e["seed"], e["round"])]
    own_d = max(float(np.nanmax(np.abs(f["dist"].astype(LD) - e["dist"]))) for f, e in agreed)
    print(f"{what}: nearest edge {min(f['edge'] for f, _ in scored):.3e} Angstrom, smallest eigenvalue gap {min(f['gap'] for f, _ in scored):.3e}; float64 "
          f"restatement vs long double: tm {own_tm:.3e}, d_i {own_d:.3e} Angstrom ({len(agreed)} of {len(scored)} pairs with the same winner)")
    assert own_tm > 0 and own_d > 0 and 2 * len(agreed) > len(scored)
    return MARGIN * own_tm, MARGIN * own_d


def self_consistent(what, got, ref, mob, offsets, tol_tm, tol_d):
    """transform_out applied to mob in long double gives dist_out; dist_out summed in long double gives tm_out; R is a rotation"""
    worst_d = worst_tm = 0.0
    for k in range(len(offsets) - 1):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        R, t = got.transform[k, :, :3], got.transform[k, :, 3]
        assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12, (what, k)
        valid = np.isfinite(ref[lo:hi]).all(axis=1) & np.isfinite(mob[lo:hi]).all(axis=1)
        d = got.dist[lo:hi]
        assert np.array_equal(np.isnan(d), ~valid), (what, k)
        if not valid.any():
            assert np.isnan(got.tm[k, 0]) and same_bytes(got.transform[k], np.eye(3, 4))
            continue
        applied = tr.applied_distances(ref[lo:hi][valid], mob[lo:hi][valid], R, t)
        worst_d = max(worst_d, float(np.abs(applied - d[valid].astype(LD)).max()))
        worst_tm = max(worst_tm, abs(float(tr.score_of_distances(d, int(got.counts[k, 1])) - LD(got.tm[k, 0]))))
    print(f"{what}: |R mob + t - ref| in long double vs dist_out {worst_d:.3e} Angstrom (allowed {tol_d:.3e}); dist_out summed in long double vs tm_out "
          f"{worst_tm:.3e} (allowed {tol_tm:.3e})")
    assert worst_d <= tol_d and worst_tm <= tol_tm, (what, worst_d, worst_tm)


def check_tm(what, got_tm, exact, tol_tm):
    mine = max(abs(float(LD(g) - e["tm"])) for g, e in zip(got_tm, exact) if e["counts"][0] > 0)
    print(f"{what}: GPU tm vs long double {mine:.3e}, allowed {tol_tm:.3e}")
    assert mine <= tol_tm, (what, mine, tol_tm)


def test_ubq_cases_equal_the_fixture(gpu, golden, cases, restated):
    assert str(golden["sha256"]) == sr.inputs_sha256(cases)
    float64, exact = [restated[n][0] for n in sr.CASES], [restated[n][1] for n in sr.CASES]
    tol_tm, tol_d = conditioned("1ubq cases", float64, exact)
    for name, f in zip(sr.CASES, float64):
        assert same_bytes(f["counts"], golden[f"{name}_counts"]) and float(f["tm"]) == float(golden[f"{name}_tm"]), name
    ref, mob, offsets = sr.flatten([cases[name] for name in sr.CASES])
    got = tmscore.tmscore_arrays(ref, mob, offsets, device=gpu, transform=True)
    for k, name in enumerate(sr.CASES):
        print(name, "tm, d0", got.tm[k].tolist(), "counts", got.counts[k].tolist())
        assert same_bytes(got.counts[k], golden[f"{name}_counts"]), name
        assert got.tm[k, 1] == tmscore.d0(76) and abs(got.tm[k, 1] - float(golden[f"{name}_d0"])) < 1e-14
    check_tm("1ubq cases", got.tm[:, 0], exact, tol_tm)
    self_consistent("1ubq cases", got, ref, mob, offsets, tol_tm, tol_d)
    tm = dict(zip(sr.CASES, got.tm[:, 0].tolist()))
    once = superpose.superpose_arrays(*cases["hinge"], [0, 76], cycles=0, device=gpu)
    global_fit = float(tr.score_of_distances(once.dist, 76))
    print("hinge: tm", tm["hinge"], "under the global fit of th_superpose", global_fit)
    assert tm["hinge"] > 0.85 and global_fit < 0.7 and abs(global_fit - float(golden["hinge_tm_global_fit"])) < 1e-12
    assert tm["mirror"] < 0.4 and tm["rigid"] > 1 - 1e-12 and tm["rigid"] <= 1.0
    assert got.counts[4, 0] == 73 and np.isnan(got.dist[4 * 76 + np.array([3, 11, 40])]).all()
    nothing = tmscore.tmscore_arrays(np.full((5, 3), np.nan), np.ones((5, 3)), [0, 5, 5], device=gpu, transform=True)
    assert np.isnan(nothing.tm[:, 0]).all() and nothing.counts.tolist() == [[0, 5, 0, 0], [0, 0, 0, 0]] and np.isnan(nothing.dist).all()
    assert same_bytes(nothing.transform, np.tile(np.eye(3, 4), (2, 1, 1))) and nothing.tm[:, 1].tolist() == [0.5, 0.5]


def test_ragged_batch_equals_the_restatement_and_each_pair_alone(gpu, ragged):
    pairs, float64, exact = ragged
    sizes = [len(r) for r, _ in pairs]
    assert sorted(set(sizes)) == list(tr.SIZES) == [0, 1, 2, 3, 4, 7, 8, 21, 63, 64, 65, 76, 129] and len(pairs) == 39 and sizes != sorted(sizes)
    tol_tm, tol_d = conditioned("ragged batch", float64, exact)
    ref, mob, offsets = sr.flatten(pairs)
    got = tmscore.tmscore_arrays(ref, mob, offsets, device=gpu, transform=True)
    for k, n in enumerate(sizes):
        assert same_bytes(got.counts[k], float64[k]["counts"]), (k, n, got.counts[k], float64[k]["counts"])
        assert got.counts[k, 2] == tr.n_seeds_of(n) and got.tm[k, 1] == tmscore.d0(n)
    check_tm("ragged batch", got.tm[:, 0], exact, tol_tm)
    self_consistent("ragged batch", got, ref, mob, offsets, tol_tm, tol_d)
    again = tmscore.tmscore_arrays(ref, mob, offsets, device=gpu, transform=True)
    assert same_result(got, again)                                              # a second run: the same bytes
    for k, (r, m) in enumerate(pairs):                                          # a pair alone: the same bytes as in the batch
        a, b = int(offsets[k]), int(offsets[k + 1])
        alone = tmscore.tmscore_arrays(r, m, [0, len(r)], device=gpu, transform=True)
        assert same_bytes(alone.dist, got.dist[a:b]) and same_bytes(alone.tm[0], got.tm[k]), (k, len(r))
        assert same_bytes(alone.counts[0], got.counts[k]) and same_bytes(alone.transform[0], got.transform[k]), (k, len(r))
    empty = [k for k, n in enumerate(sizes) if n == 0]
    assert np.isnan(got.tm[empty, 0]).all() and not got.counts[empty].any()
    single = [k for k, n in enumerate(sizes) if n == 1]
    assert got.tm[single, 0].tolist() == [1.0] * 3 and got.counts[single].tolist() == [[1, 1, 1, 1]] * 3


def test_4096_positions_use_every_word_of_the_mask(gpu):
    ref, rigid, hinged = tr.long_chain()
    n = tr.MAX_POSITIONS
    assert len(ref) == n == 4096 == tmscore.MAX_POSITIONS
    two_ref, two_mob = np.concatenate([ref, ref]), np.concatenate([rigid, hinged])
    offsets = np.array([0, n, 2 * n], np.int64)
    timing = {}
    got = tmscore.tmscore_arrays(two_ref, two_mob, offsets, device=gpu, transform=True, timing=timing)
    seeds = sum(n - (n >> k) + 1 for k in range(11))
    print("4096 positions: tm", got.tm[:, 0].tolist(), "counts", got.counts.tolist(), "kernel ms", timing["kernel_ms"])
    assert got.counts[:, :3].tolist() == [[n, n, seeds]] * 2 and seeds == tr.n_seeds_of(n) and (got.counts[:, 3] >= seeds).all()
    assert 1 - 1e-9 < got.tm[0, 0] <= 1.0
    # a lower bound of the maximum: the score, in long double, of the SVD Kabsch fit over the 3096 positions that did not move
    body = n - 1000
    R, t = tr.kabsch_transform(ref[:body], hinged[:body])
    lower = float(tr.score_of_distances(tr.applied_distances(ref, hinged, R, t), n))
    print(f"hinged: tm {got.tm[1, 0]!r}, the fit over the first {body} positions alone scores {lower!r}")
    assert body / n - 1e-9 < lower and lower <= got.tm[1, 0] <= 1.0
    # the tolerances of the self-consistency, measured on this data without the restatement: forming d_i and the sum in float64
    # against long double, under the transforms the GPU returned
    own_d = own_tm = 0.0
    for k, mob in enumerate((rigid, hinged)):
        R, t = got.transform[k, :, :3], got.transform[k, :, 3]
        delta = mob @ R.T + t - ref
        d64 = np.sqrt((delta * delta).sum(axis=1))
        own_d = max(own_d, float(np.abs(d64.astype(LD) - tr.applied_distances(ref, mob, R, t)).max()))
        own_tm = max(own_tm, abs(float(LD(tr.score_of_distances(d64, n, np.float64)) - tr.score_of_distances(d64, n))))
    print(f"4096 positions: float64 against long double under the returned transforms: d_i {own_d:.3e} Angstrom, the sum {own_tm:.3e}")
    assert own_d > 0 and own_tm > 0
    self_consistent("4096 positions", got, two_ref, two_mob, offsets, MARGIN * own_tm, MARGIN * own_d)
    # one position more: the call is refused, and through tmscore() that pair alone carries the error
    longer = np.concatenate([ref, ref[:1] + 1.0])
    with pytest.raises(_lib.TimedHipError) as err:
        tmscore.tmscore_arrays(longer, longer, [0, n + 1], device=gpu)
    assert err.value.code == _lib.TH_EINVAL and "4096" in str(err.value)
    from timed_hip import pdbio
    residues = [pdbio.Residue("A", str(k + 1), "GLY") for k in range(n + 1)]
    lay = lambda xyz: superpose.AtomLayout(np.asarray(xyz, np.float64), residues[:len(xyz)])                      # noqa: E731
    first, middle, last = tmscore.tmscore([(lay(ref), lay(rigid)), (lay(longer), lay(longer)), (lay(ref), lay(hinged))], device=gpu)
    assert "4097" in middle.error and np.isnan(middle.tm) and first.error is None and last.error is None
    assert [first.tm, last.tm] == got.tm[:, 0].tolist() and same_bytes(last.dist, got.dist[n:])


def test_norm_len_and_rounds_zero(gpu, cases, restated):
    names = ("noise", "hinge")
    ref, mob, offsets = sr.flatten([cases[name] for name in names])
    doubled = np.array([152, 152], np.int32)
    float64 = [tr.restate(*cases[name], norm_len=152) for name in names] + [tr.restate(*cases[name], rounds=0) for name in names]
    exact = [tr.restate(*cases[name], norm_len=152, dtype=LD) for name in names] + [tr.restate(*cases[name], rounds=0, dtype=LD) for name in names]
    tol_tm, tol_d = conditioned("norm_len = 152 and rounds = 0", float64, exact)
    got = tmscore.tmscore_arrays(ref, mob, offsets, norm_len=doubled, device=gpu, transform=True)
    plain = tmscore.tmscore_arrays(ref, mob, offsets, device=gpu)
    assert got.tm[:, 1].tolist() == [tmscore.d0(152)] * 2 and tmscore.d0(152) > tmscore.d0(76) == plain.tm[0, 1]
    assert abs(tmscore.d0(152) - (1.24 * 137 ** (1 / 3) - 1.8)) < 1e-14
    for k in range(2):
        assert same_bytes(got.counts[k], float64[k]["counts"]) and got.counts[k, :3].tolist() == [76, 152, 239]
        assert got.tm[k, 0] < plain.tm[k, 0]                                   # twice the length: at most half the sum, at a larger d0
    check_tm("norm_len = 152", got.tm[:, 0], exact[:2], tol_tm)
    self_consistent("norm_len = 152", got, ref, mob, offsets, tol_tm, tol_d)
    once = tmscore.tmscore_arrays(ref, mob, offsets, rounds=0, device=gpu, transform=True)
    for k in range(2):
        assert same_bytes(once.counts[k], float64[2 + k]["counts"]) and once.counts[k, 3] == once.counts[k, 2] == 239
        assert once.tm[k, 0] <= plain.tm[k, 0]
    check_tm("rounds = 0", once.tm[:, 0], exact[2:], tol_tm)                     # the best fit over a seed window
    self_consistent("rounds = 0", once, ref, mob, offsets, tol_tm, tol_d)
    with pytest.raises(_lib.TimedHipError) as err:
        tmscore.tmscore_arrays(ref, mob, offsets, norm_len=[76, 75], device=gpu)
    assert err.value.code == _lib.TH_EINVAL and "norm_len" in str(err.value)


def test_abi_errors_return_einval_and_leave_the_outputs_untouched(gpu, lib, cases):
    ref, mob, offsets = sr.flatten([cases["noise"], cases["hinge"]])
    total = len(ref)
    long_pair = np.zeros((4097, 3))
    bad_calls = {
        "negative total": dict(total=-1), "negative n_pairs": dict(n_pairs=-1), "total too large": dict(total=1 << 31),
        "n_pairs too large": dict(n_pairs=1 << 31), "ref NULL": dict(ref=None), "mob NULL": dict(mob=None), "offsets NULL": dict(offsets=None),
        "tm NULL": dict(tm=None), "counts NULL": dict(counts=None), "offsets decrease": dict(offsets=np.array([0, 80, 79], np.int64)),
        "offsets end before total": dict(offsets=np.array([0, 76, total - 1], np.int64)), "offsets start late": dict(offsets=np.array([1, 76, total], np.int64)),
        "offsets end past total": dict(total=total - 1), "rounds negative": dict(rounds=-1), "norm_len below n": dict(norm=np.array([76, 75], np.int32)),
        "4097 positions": dict(ref=long_pair, mob=long_pair, total=4097, offsets=np.array([0, 4097], np.int64), n_pairs=1),
    }

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def fresh():
        return dict(tm=np.full((2, 2), 6.5), counts=np.full((2, 4), 12345, np.int64), dist=np.full(4097, 6.5), moves=np.full((2, 12), 6.5))

    def call(out, ref=ref, mob=mob, total=total, offsets=offsets, n_pairs=2, norm=None, rounds=20, **replaced):
        o = dict(out, **replaced)
        ms = C.c_double(-1.0)
        rc = lib.th_tmscore(gpu, ptr(ref), ptr(mob), total, ptr(offsets), n_pairs, ptr(norm), rounds, ptr(o["tm"]), ptr(o["counts"]), ptr(o["dist"]),
                            ptr(o["moves"]), C.byref(ms))
        return rc, ms.value
    for what, change in bad_calls.items():
        out = fresh()
        rc, ms = call(out, **change)
        assert rc == _lib.TH_EINVAL, what
        assert b"th_tmscore" in lib.th_last_error(), what
        assert (out["tm"] == 6.5).all() and (out["counts"] == 12345).all() and (out["dist"] == 6.5).all() and (out["moves"] == 6.5).all(), what
        assert ms == -1.0, what
    out = fresh()
    rc, ms = call(out)
    assert rc == _lib.TH_OK and ms > 0
    want = tmscore.tmscore_arrays(ref, mob, offsets, device=gpu, transform=True)
    assert same_bytes(out["tm"], want.tm) and same_bytes(out["counts"], want.counts) and same_bytes(out["dist"][:total], want.dist)
    assert same_bytes(out["moves"].reshape(2, 3, 4), want.transform) and (out["dist"][total:] == 6.5).all()
    for absent in ("dist", "moves"):                                            # an optional output left out: the same other bytes
        out = fresh()
        rc, _ = call(out, **{absent: None})
        assert rc == _lib.TH_OK and same_bytes(out["tm"], want.tm) and same_bytes(out["counts"], want.counts)
        assert same_bytes(out["dist"][:total], want.dist) if absent == "moves" else same_bytes(out["moves"].reshape(2, 3, 4), want.transform)
        assert (out[absent] == 6.5).all()
    bare = tmscore.tmscore_arrays(ref, mob, offsets, device=gpu, dist=False)
    assert bare.dist is None and bare.transform is None and same_bytes(bare.tm, want.tm) and same_bytes(bare.counts, want.counts)
    assert lib.th_tmscore(gpu, None, None, 0, None, 0, None, 20, None, None, None, None, None) == _lib.TH_OK                 # n_pairs = 0
    with pytest.raises(_lib.TimedHipError) as err:
        tmscore.tmscore_arrays(ref, mob, offsets, rounds=-3, device=gpu)
    assert err.value.code == _lib.TH_EINVAL


def test_files_and_cli_end_to_end(gpu, golden, cases, tmp_path, capsys):
    import analyse_models
    names = ("rigid", "noise", "hinge", "mirror")
    (tmp_path / "models" / "deep").mkdir(parents=True)
    (tmp_path / "native.pdb").write_text(sr.pdb_text(cases["hinge"][0]))
    for name in names:
        (tmp_path / "models" / "deep" / f"{name}.pdb").write_text(sr.pdb_text(cases[name][1]))
    ok = np.isfinite(cases["invalid"][0]).all(axis=1) & np.isfinite(cases["invalid"][1]).all(axis=1)
    numbers = np.arange(1, 77)[ok]
    text = sr.pdb_text(cases["invalid"][1][ok]).splitlines()
    (tmp_path / "models" / "invalid.pdb").write_text("\n".join(line[:22] + f"{n:4d}" + line[26:] for line, n in zip(text, numbers)) + "\nEND\n")
    listed = [(tmp_path / "native.pdb", tmp_path / "models" / "deep" / f"{name}.pdb") for name in names] + [(tmp_path / "native.pdb", tmp_path / "models" / "invalid.pdb")]
    stats = {}
    results = tmscore.tmscore(listed, device=gpu, stats=stats)
    assert stats["submissions"] == 1 and stats["files_parsed"] == 6 and stats["kernel_ms"] > 0
    native = np.round(cases["hinge"][0], 3)
    want = tmscore.tmscore_arrays(*sr.flatten([(native, np.round(cases[name][1], 3)) for name in names]), device=gpu)
    for k, res in enumerate(results[:4]):                                       # files against arrays of the rounded coordinates: the same bytes
        assert res.error is None and same_bytes(res.dist, want.dist[76 * k:76 * k + 76]) and [res.tm, res.d0] == want.tm[k].tolist()
        assert [res.n_valid, res.norm_length, res.n_seeds, res.n_fits] == want.counts[k].tolist() and len(res.residues) == 76
    assert "length mismatch" in results[4].error
    # three decimals move the scores by less than 1e-3
    for k, name in enumerate(names):
        assert abs(results[k].tm - float(golden[f"{name}_tm"])) < 1e-3, name
    (numbered,) = tmscore.tmscore([listed[4]], pair_by="number", device=gpu)
    alone = tmscore.tmscore_arrays(native[ok], np.round(cases["invalid"][1][ok], 3), [0, 73], norm_len=[76], device=gpu)
    assert numbered.error is None and (numbered.unpaired_reference, numbered.unpaired_model, numbered.n_valid, numbered.norm_length) == (3, 0, 73, 76)
    assert numbered.tm == alone.tm[0, 0] and same_bytes(numbered.dist, alone.dist) and numbered.n_seeds == 230
    # the command line
    out = tmp_path / "out"
    parser = analyse_models.build_parser()
    common = ["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models", str(tmp_path / "models"), "--device", str(gpu)]
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(out), "--tmscore"]))
    assert "5 pairs (1 with an error), 304 positions, 6 files parsed in 3 GPU submission(s)" in capsys.readouterr().out

    def read(folder, name):
        with open(folder / name, newline="") as f:
            return list(csv.reader(f))
    scores = read(out, "model_tmscore.csv")
    assert scores[0] == analyse_models.TMSCORE_COLUMNS == ["label", "reference", "model", "n_valid", "norm_length", "d0", "tm_score", "tm_global_fit",
                                                           "n_seeds", "n_fits", "error"] and len(scores) == 6
    assert [r[0] for r in scores[1:]] == ["deep/hinge.pdb", "deep/mirror.pdb", "deep/noise.pdb", "deep/rigid.pdb", "invalid.pdb"]
    row = dict(zip(scores[0], scores[1]))
    hinge = results[2]
    assert float(row["tm_score"]) == hinge.tm and float(row["d0"]) == hinge.d0 and row["error"] == ""
    assert [int(row[k]) for k in ("n_valid", "norm_length", "n_seeds", "n_fits")] == [hinge.n_valid, hinge.norm_length, hinge.n_seeds, hinge.n_fits]
    once = superpose.superpose_arrays(native, np.round(cases["hinge"][1], 3), [0, 76], cycles=0, device=gpu)
    assert abs(float(row["tm_global_fit"]) - float(tr.score_of_distances(once.dist, 76))) < 1e-14
    assert float(row["tm_score"]) > 0.85 and float(row["tm_global_fit"]) < 0.7
    for r in scores[1:5]:
        assert float(r[6]) >= float(r[7]) - 1e-12                               # the search starts from the global fit
    assert "length mismatch" in scores[5][-1] and scores[5][6] == scores[5][7] == "nan"
    plain = tmp_path / "plain"
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(plain)]))
    assert sorted(p.name for p in plain.iterdir()) == ["model_scores.csv", "residue_deviation.csv"]
    assert sorted(p.name for p in out.iterdir()) == ["model_scores.csv", "model_tmscore.csv", "residue_deviation.csv"]
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (out / name).read_bytes() == (plain / name).read_bytes()
    by_number = tmp_path / "by_number"
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(by_number), "--tmscore", "--lddt", "--pair_by", "number", "--tm_rounds", "3"]))
    scores = read(by_number, "model_tmscore.csv")
    last = dict(zip(scores[0], scores[5]))
    assert last["error"] == "" and (last["n_valid"], last["norm_length"], last["n_seeds"]) == ("73", "76", "230") and float(last["tm_score"]) <= numbered.tm
    assert sorted(p.name for p in by_number.iterdir()) == ["model_lddt.csv", "model_scores.csv", "model_tmscore.csv", "residue_deviation.csv", "residue_lddt.csv"]
