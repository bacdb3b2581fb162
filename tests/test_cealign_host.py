"""CE alignment without a GPU: the NumPy restatement (tests/cealign_restatement.py) against the committed fixture, against itself in long
double and on cases small enough to check by hand; the Python layer's argument checks, its byte budget and analyse_models.py --cealign
/ --pair_by_cealign with the kernel calls replaced by restatements; the header prototype, the ctypes entry and the build list."""
import csv
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cealign_restatement as cr  # noqa: E402
import superpose_restatement as sr  # noqa: E402
from test_superpose_host import restated_arrays as restated_superpose  # noqa: E402
from timed_hip import _lib, cealign, pdbio, superpose  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHRASE = "PARITY UNPINNED AGAINST PYMOL"


@pytest.fixture(scope="module")
def cases():
    return cr.ubq_cases()


@pytest.fixture(scope="module")
def restated(cases):
    """the float64 restatement of the seven cases: computed once, shared, never changed"""
    return {name: cr.restate(*cases[name]) for name in cr.CASES}


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restated_arrays(ref_xyz, ref_offsets, mob_xyz, mob_offsets, d0=3.0, d1=4.0, gap_max=30, device=0, transform=False, timing=None):
    """cealign.cealign_arrays with the GPU call replaced by the restatement"""
    parts = cr.restate_batch(ref_xyz, ref_offsets, mob_xyz, mob_offsets, d0, d1, gap_max)
    return cealign.CeTables(np.concatenate([p["align"] for p in parts] + [np.zeros(0, np.int32)]),
                            np.array([[p["rmsd"], p["score"]] for p in parts], np.float64).reshape(-1, 2),
                            np.array([p["counts"] for p in parts], np.int64).reshape(-1, 6),
                            np.array([p["transform"] for p in parts], np.float64).reshape(-1, 3, 4) if transform else None)


def test_restatement_reproduces_the_fixture_and_the_figures_of_the_rule(cases, restated):
    assert os.path.getsize(cr.GOLDEN) < 64 * 1024
    golden = np.load(cr.GOLDEN)
    assert str(golden["sha256"]) == cr.inputs_sha256(cases)
    again = cr.golden_arrays(cases)
    assert sorted(golden.files) == sorted(again)
    for key in golden.files:
        assert same_bytes(golden[key], np.asarray(again[key])), key
    text = open(os.path.join(ROOT, "tests", "golden", "make_cealign_golden.py")).read()
    assert "NOT by the kernel" in text and PHRASE in text
    # the four cases of the superposition fixture are its inputs, byte for byte
    base = sr.ubq_cases()
    for name in ("rigid", "noise", "hinge", "mirror"):
        assert all(same_bytes(a, b) for a, b in zip(cases[name], base[name])), name
    want = {"rigid": (9, 3205, None), "noise": (8, 3029, 0.825), "hinge": (8, 3218, 0.479), "mirror": (8, 3205, 9.55), "deletion": (8, None, None),
            "insertion": (9, None, None), "helix_strand": (0, 0, None)}
    for name, (n_afps, n_starts, rmsd) in want.items():
        counts = golden[f"{name}_counts"].tolist()
        assert counts[3] == n_afps and counts[4] == 8 * n_afps and counts[5] == min(20, counts[2]), (name, counts)
        assert n_starts is None or counts[2] == n_starts, (name, counts)
        assert rmsd is None or abs(float(golden[f"{name}_rmsd"][0]) - rmsd) < 5e-3 * rmsd, name
    assert float(golden["rigid_rmsd"][0]) < 1e-12 and np.isnan(golden["helix_strand_rmsd"]).all() and (golden["helix_strand_align"] == -1).all()
    assert golden["deletion_counts"].tolist()[:2] == [76, 70] and golden["insertion_counts"].tolist()[:2] == [76, 86]
    assert float(golden["deletion_rmsd"][0]) < 0.5 and float(golden["insertion_rmsd"][0]) < 0.5
    # the alignment steps over the six missing residues, and over the ten inserted ones
    gone = restated["deletion"]["align"]
    at = np.nonzero(gone >= 0)[0]
    assert set((at - gone[at]).tolist()) == {0, 6} and all(gone[i] == i for i in at if i < 30) and all(gone[i] == i - 6 for i in at if i >= 36)
    assert not ((at >= 30) & (at < 36)).any()
    more = restated["insertion"]["align"]
    at = np.nonzero(more >= 0)[0]
    assert set((more[at] - at).tolist()) == {0, 10} and all(more[i] == i for i in at if i <= 40) and all(more[i] == i + 10 for i in at if i > 40)
    for name in ("rigid", "noise", "hinge", "mirror"):                          # equally long, unmoved in sequence: the diagonal
        a = restated[name]["align"]
        assert (a[a >= 0] == np.nonzero(a >= 0)[0]).all(), name


def test_float64_restatement_against_long_double(cases, restated):
    for name in cr.NOISY:
        a, b = restated[name], cr.restate(*cases[name], dtype=np.longdouble)
        err = abs(float(np.longdouble(a["rmsd"]) - b["rmsd"]))
        print(f"{name}: float64 restatement vs long double, rmsd error {err:.3e}; margins " + ", ".join(f"{k} {v:.3e}" for k, v in a["margins"].items()))
        assert same_bytes(a["counts"], b["counts"]) and same_bytes(a["align"], b["align"]) and a["path"] == b["path"], name
        assert err < 1e-13 and cr.smallest_margin(a) > 1e-6, name                # no decision of these cases sits on an edge
        assert abs(cr.smallest_margin(a) - cr.smallest_margin(b)) < 1e-12
        assert abs(float(cr.applied_rmsd(*cases[name], a["align"], a["transform"]) - np.longdouble(a["rmsd"]))) < 1e-13, name


def fragment(n, seed=3):
    rng = np.random.default_rng(seed)
    steps = rng.normal(size=(n, 3))
    steps *= 3.8 / np.linalg.norm(steps, axis=1, keepdims=True)
    return np.cumsum(steps, axis=0)


def test_tiny_cases_checked_by_hand():
    eight = fragment(8)
    one = cr.restate(eight, eight + 5.0)
    assert one["counts"].tolist() == [8, 8, 1, 1, 8, 1] and one["align"].tolist() == list(range(8)) and one["path"] == [(0, 0)]
    assert float(one["score"]) < 1e-12 and float(one["rmsd"]) < 1e-12               # S(0, 0) of a shifted copy is rounding noise: the path's score
    assert float(cr.restate(eight, eight)["score"]) == 0.0
    seven = cr.restate(eight[:7], eight[:7])
    assert seven["counts"].tolist() == [7, 7, 0, 0, 0, 0] and (seven["align"] == -1).all() and np.isnan(seven["rmsd"]) and np.isnan(seven["score"])
    assert seven["transform"].tolist() == np.eye(3, 4).ravel().tolist()
    assert cr.restate(eight, eight[:7])["counts"].tolist() == [8, 7, 0, 0, 0, 0]
    # 16 residues in two blocks, the model with 3 more between them: two AFPs, the second through candidate g = 6 (b + 8 + 3)
    chain = fragment(19, seed=4)
    ref = np.concatenate([chain[:8], chain[11:]])
    two = cr.restate(ref, chain, keep=1)                                        # the first candidate alone: among exact copies every RMSD is rounding noise
    assert two["counts"].tolist()[:2] == [16, 19] and two["counts"].tolist()[3:] == [2, 16, 1] and two["path"] == [(0, 0), (8, 11)]
    assert two["align"].tolist() == list(range(8)) + list(range(11, 19)) and float(two["rmsd"]) < 1e-12
    assert cr.candidates_of(30)[0][5] == 3 and cr.candidates_of(30)[1][6] == 3 and len(cr.candidates_of(30)[0]) == 61
    assert cr.restate(ref, chain, gap_max=3, keep=1)["path"] == [(0, 0), (8, 11)]          # a gap of 3 is the shortest that reaches it
    # a position that is not finite leaves the compacted list; the outputs speak the caller's indices
    holed = np.insert(eight, 3, [np.nan, 0.0, 0.0], axis=0)
    res = cr.restate(eight, holed)
    assert res["counts"].tolist() == [8, 8, 1, 1, 8, 1] and res["align"].tolist() == [0, 1, 2, 4, 5, 6, 7, 8]
    assert len(cr.S_PAIRS) == 21 and cr.S_PAIRS[:3] == [(0, 2), (0, 3), (0, 4)] and cr.S_PAIRS[-1] == (5, 7)
    assert cr.D_TERMS == [(0, 0), (7, 7), (1, 6), (2, 5), (3, 4), (4, 3), (5, 2), (6, 1)]


def test_python_layer_checks_its_arguments():
    one = np.zeros((1, 3))
    with pytest.raises(ValueError, match="offsets"):
        cealign.cealign_arrays(one, [0, 1], one, [0, 1, 1])
    with pytest.raises(ValueError, match="offsets"):
        cealign.cealign_arrays(one, [], one, [])
    with pytest.raises(ValueError, match="gap_max"):
        cealign.cealign([], gap_max=32)
    with pytest.raises(ValueError, match="d0"):
        cealign.cealign([], d0=0.0)
    with pytest.raises(ValueError, match="d1"):
        cealign.cealign([], d1=float("inf"))
    assert cealign.cealign([]) == [] and (cealign.D0, cealign.D1, cealign.GAP_MAX, cealign.MAX_POSITIONS, cealign.WINDOW, cealign.KEEP) == (3.0, 4.0, 30, 2048, 8, 20)
    assert superpose.PAIR_BY == ("position", "number")


def test_library_exports_th_cealign_and_checks_arguments_without_a_gpu(lib):
    n = 9
    xyz = np.zeros((n, 3))
    offsets = np.array([0, n], np.int64)
    align, scores, counts = np.full(n, 77, np.int32), np.full((1, 2), 6.5), np.full((1, 6), 77, np.int64)
    long_one = np.zeros((2049, 3))

    def call(ref=xyz, ref_total=n, ro=offsets, mob=xyz, mob_total=n, mo=offsets, n_pairs=1, d0=3.0, d1=4.0, gap_max=30, a=align, s=scores, c=counts):
        p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)        # noqa: E731
        return lib.th_cealign(0, p(ref), ref_total, p(ro), p(mob), mob_total, p(mo), n_pairs, d0, d1, gap_max, p(a), p(s), p(c), None, None)
    bad = {"negative ref_total": dict(ref_total=-1), "negative mob_total": dict(mob_total=-1), "negative pairs": dict(n_pairs=-1),
           "too large": dict(ref_total=1 << 31), "ref_offsets NULL": dict(ro=None), "mob_offsets NULL": dict(mo=None), "scores NULL": dict(s=None),
           "counts NULL": dict(c=None), "align NULL": dict(a=None), "ref NULL": dict(ref=None), "mob NULL": dict(mob=None),
           "ref end": dict(ro=np.array([0, n + 1], np.int64)), "mob start": dict(mo=np.array([1, n], np.int64)),
           "mob decrease": dict(mo=np.array([0, n + 1, n], np.int64), ro=np.array([0, 0, n], np.int64), n_pairs=2),
           "d0 zero": dict(d0=0.0), "d0 nan": dict(d0=float("nan")), "d1 negative": dict(d1=-4.0), "d1 infinite": dict(d1=float("inf")),
           "gap_max negative": dict(gap_max=-1), "gap_max 32": dict(gap_max=32),
           "2049 reference positions": dict(ref=long_one, ref_total=2049, ro=np.array([0, 2049], np.int64), a=np.full(2049, 77, np.int32)),
           "2049 model positions": dict(mob=long_one, mob_total=2049, mo=np.array([0, 2049], np.int64))}
    for what, kw in bad.items():
        assert call(**kw) == _lib.TH_EINVAL, what
        assert b"th_cealign" in lib.th_last_error(), what
    assert (align == 77).all() and (scores == 6.5).all() and (counts == 77).all()
    assert lib.th_cealign(0, None, 0, None, None, 0, None, 0, 3.0, 4.0, 30, None, None, None, None, None) == _lib.TH_OK      # no pairs: no launch
    with pytest.raises(_lib.TimedHipError) as err:
        cealign.cealign_arrays(long_one, [0, 2049], xyz, [0, n])
    assert err.value.code == _lib.TH_EINVAL and "2048" in str(err.value)


def layout(xyz, first=1):
    xyz = np.asarray(xyz, np.float64)
    return superpose.AtomLayout(xyz, [pdbio.Residue("A", str(first + k), "GLY") for k in range(len(xyz))])


def test_batches_are_charged_the_similarity_matrix_and_long_structures_carry_an_error(monkeypatch):
    calls = []

    def counted(ref_xyz, ref_offsets, *a, **kw):
        calls.append(len(ref_offsets) - 1)
        return restated_arrays(ref_xyz, ref_offsets, *a, **kw)
    monkeypatch.setattr(cealign, "cealign_arrays", counted)
    chain = fragment(30, seed=7)
    pairs = [(layout(chain[:24]), layout(chain[k:k + 20] + 1.0)) for k in range(5)]
    one = cealign.pair_bytes(24, 20)
    assert one == 17 * 13 * 20 + (17 + 13) * 168 + 44 * 32                       # S and the start records, the window rows, the positions
    assert cealign.pair_bytes(7, 300) == 307 * 32 and cealign.pair_bytes(0, 0) == 0          # no window start: no matrix
    assert cealign.pair_bytes(2048, 2048) > 2041 * 2041 * 20
    stats = {}
    whole = cealign.cealign(pairs, stats=stats)
    assert calls == [5] and stats["submissions"] == 1 and stats["files_parsed"] == 0
    del calls[:]
    split = cealign.cealign(pairs, budget_bytes=2 * one + one // 2)             # two pairs fit, three do not
    assert calls == [2, 2, 1]
    for k, (a, b) in enumerate(zip(whole, split)):
        want = cr.restate(pairs[k][0].xyz, pairs[k][1].xyz)
        assert a.error is None and a.rmsd == b.rmsd == float(want["rmsd"]) and a.path_score == float(want["score"])
        assert [a.n_ref, a.n_model, a.n_starts, a.n_afps, a.n_aligned, a.n_candidates] == want["counts"].tolist()
        assert a.reference_index.tolist() == np.nonzero(want["align"] >= 0)[0].tolist() == b.reference_index.tolist()
        assert a.model_index.tolist() == want["align"][want["align"] >= 0].tolist()
        assert (a.model_index - a.reference_index == -k).all()                    # the model starts k residues into the chain
    # a structure above 2048 positions: its pair's error, and the neighbours are aligned
    giant = (layout(np.zeros((10, 3))), layout(np.zeros((2049, 3))))
    del calls[:]
    first, middle, last = cealign.cealign([pairs[0], giant, pairs[1]])
    assert calls == [2] and "2049" in middle.error and "2048" in middle.error and np.isnan(middle.rmsd) and middle.n_afps == 0
    assert first.rmsd == whole[0].rmsd and last.rmsd == whole[1].rmsd
    # the alignment as a pairing
    prepared = cealign.prepare_aligned([pairs[0], giant, pairs[2]])
    assert isinstance(prepared, superpose.Prepared) and isinstance(prepared.pairs[1], str) and prepared.files == 0
    ref, mod, ours, theirs = prepared.pairs[2]
    assert ref is pairs[2][0] and mod is pairs[2][1] and ours.tolist() == whole[2].reference_index.tolist() and (theirs == ours - 2).all()
    monkeypatch.setattr(superpose, "superpose_arrays", restated_superpose)
    scored = superpose.superpose(prepared)
    assert scored[1].error and scored[2].error is None and scored[2].n_valid == whole[2].n_aligned
    assert scored[2].unpaired_reference == 24 - whole[2].n_aligned and scored[2].unpaired_model == 20 - whole[2].n_aligned
    assert abs(scored[2].rmsd_fit_all - whole[2].rmsd) < 1e-12                   # the same fit over the same positions


def test_analyse_models_writes_the_cealign_tables_and_pairs_by_them(tmp_path, monkeypatch, cases, capsys):
    import analyse_models
    monkeypatch.setattr(superpose, "superpose_arrays", restated_superpose)
    monkeypatch.setattr(cealign, "cealign_arrays", restated_arrays)
    ref, deleted = cases["deletion"]
    (tmp_path / "models").mkdir()
    (tmp_path / "native.pdb").write_text(sr.pdb_text(ref))
    (tmp_path / "models" / "deletion.pdb").write_text(sr.pdb_text(deleted, first=101))
    (tmp_path / "models" / "rigid.pdb").write_text(sr.pdb_text(cases["rigid"][1]))
    parser = analyse_models.build_parser()
    common = ["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models", str(tmp_path / "models")]
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "plain")]))
    capsys.readouterr()
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "out"), "--cealign"]))
    assert "2 pairs (1 with an error), 76 positions, 3 files parsed in 2 GPU submission(s)" in capsys.readouterr().out
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["model_scores.csv", "residue_deviation.csv"]
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["model_cealign.csv", "model_scores.csv", "residue_cealign.csv", "residue_deviation.csv"]
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (tmp_path / "out" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes()

    def read(folder, name):
        with open(tmp_path / folder / name, newline="") as f:
            return list(csv.reader(f))
    rows = read("out", "model_cealign.csv")
    assert rows[0] == analyse_models.CEALIGN_COLUMNS == ["label", "reference", "model", "n_ref", "n_model", "n_starts", "n_afps", "n_aligned", "rmsd",
                                                         "path_score", "error"]
    assert [r[0] for r in rows[1:]] == ["deletion.pdb", "rigid.pdb"]
    got = dict(zip(rows[0], rows[1]))
    want = cr.restate(np.round(ref, 3), np.round(deleted, 3))
    assert [int(got[k]) for k in ("n_ref", "n_model", "n_starts", "n_afps", "n_aligned")] == want["counts"].tolist()[:5] and got["error"] == ""
    assert float(got["rmsd"]) == float(want["rmsd"]) and float(got["path_score"]) == float(want["score"]) and int(got["n_aligned"]) == 64
    residues = read("out", "residue_cealign.csv")
    assert residues[0] == analyse_models.RESIDUE_CEALIGN_COLUMNS and len(residues) == 1 + 2 * 76
    mine = [r for r in residues[1:] if r[0] == "deletion.pdb"]
    paired = [r for r in mine if r[5]]
    assert len(paired) == 64 and all(r[4] == "A" and r[6] == "GLY" for r in paired) and all(r[4:] == ["", "", "", ""] for r in mine if not r[5])
    for r in paired:                                                            # the model is numbered from 101 and lacks residues 31 .. 36
        k = int(r[2]) - 1
        assert int(r[5]) == 101 + int(want["align"][k]) and int(want["align"][k]) == (k if k < 30 else k - 6)
    worst = float(np.sqrt(np.mean([float(r[7]) ** 2 for r in paired])))
    assert abs(worst - float(want["rmsd"])) < 1e-9                              # the distances under the winning fit give its RMSD
    scores = read("out", "model_scores.csv")
    assert "length mismatch" in scores[1][-1]
    # the alignment as the pairing of the other scores
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "ce"), "--pair_by_cealign"]))
    assert sorted(p.name for p in (tmp_path / "ce").iterdir()) == ["model_scores.csv", "residue_deviation.csv"]
    row = dict(zip(*read("ce", "model_scores.csv")[:2]))
    assert row["error"] == "" and row["n_valid"] == "64" and (row["unpaired_reference"], row["unpaired_model"]) == ("12", "6")
    assert abs(float(row["rmsd_fit_all"]) - float(want["rmsd"])) < 1e-9
    rigid = cr.restate(np.round(ref, 3), np.round(cases["rigid"][1], 3))
    assert len(read("ce", "residue_deviation.csv")) == 1 + 64 + int(rigid["counts"][4]) and rigid["counts"][3] >= 8
    for flags in (["--cealign", "--ce_d0", "0"], ["--cealign", "--ce_gap_max", "32"], ["--pair_by_cealign", "--ce_d1", "nan"]):
        with pytest.raises(SystemExit):
            analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "bad")] + flags))
    args = parser.parse_args(["--pairs", "p.csv"])
    assert (args.cealign, args.pair_by_cealign, args.ce_d0, args.ce_d1, args.ce_gap_max, args.pair_by) == (False, False, 3.0, 4.0, 30, "position")


_CTYPES = {"int": "c_int", "int64_t": "c_long", "double": "c_double", "const double*": "c_void_p", "const int64_t*": "c_void_p",
           "int32_t*": "c_void_p", "int64_t*": "c_void_p", "double*": ("c_void_p", "LP_c_double")}


def test_header_ctypes_build_list_and_the_unpinned_parity_phrase():
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    m = re.search(r"^(\w+) th_cealign\(([^;]*)\);", header, re.M)
    assert m
    res, args = _lib.PROTOTYPES["th_cealign"]
    assert res.__name__ == _CTYPES[m.group(1)]
    declared = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(2).split(",")]
    assert len(declared) == len(args) == 16, (declared, args)
    for c_type, ct in zip(declared, args):
        want = _CTYPES[c_type]
        assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (c_type, ct)
    before = header[:m.start()]
    section = before[before.rindex("/* ----"):]
    for phrase in (PHRASE, "MIRROR IMAGES", "no fused multiply-add", "(mA - 7)(mB - 7) * 8 bytes", "of equal costs the smallest g", "NO START",
                   "#define TH_CE_MAX_POSITIONS 2048", "#define TH_CE_WINDOW 8", "#define TH_CE_KEEP 20"):
        assert phrase in section, phrase
    import __graft_entry__
    assert "cealign.hip" in __graft_entry__.HIP_SOURCES
    source = open(os.path.join(ROOT, "timed-design_amd", "csrc", "cealign.hip")).read()
    assert PHRASE in source and '#include "horn_fit.h"' in source and "fp contract(off)" in source and "horn_rotation(C, F)" in source
    shared = open(os.path.join(ROOT, "timed-design_amd", "csrc", "horn_fit.h")).read()
    for only_shared in ("f.cr[x] - ((f.R[3 * x]", "+ f.cr[0]) - ref[0]", "S[x][y] += a[x] * b[y]", "sm[a] += mob[a]"):     # the transform store, the
        assert shared.count(only_shared) == 1, only_shared                                                             # distance, the two sums
    for piece in ("add_position(", "add_covariance(", "distance(fit,", "store(best_fit,"):          # the shared steps, in path order
        assert piece in source, piece
    for copied in ("cr[x] - ((", "[3 * x] *", "+ cr[0]) -", "+ fr[0]) -", "+= u[x] * v[y]", "+= a[x] * b[y]"):
        assert copied not in source, copied
    assert "atomic" not in source.replace("No atomics", "") and "asm" not in source
    for kernel in ("k_ce_windows", "k_ce_similarity", "k_ce_paths", "k_ce_best"):
        assert f"hipLaunchKernelGGL({kernel}" in source, kernel
    import analyse_models
    text = re.sub(r"\s+", " ", analyse_models.build_parser().format_help())
    assert PHRASE in text and "--cealign" in text and "--pair_by_cealign" in text and "2048" in text
    from design_utils import analyse_utils
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert PHRASE in cealign.__doc__ and PHRASE in analyse_utils.calculate_cealign_RMSD.__doc__ and "th_cealign" in readme and "--cealign" in readme
    assert "th_cealign" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_cealign.py")) and os.path.exists(os.path.join(ROOT, "profiles", "cealign.txt"))
