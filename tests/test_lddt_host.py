"""lDDT without a GPU: the NumPy restatement (tests/lddt_restatement.py) against the committed fixture and the figures of the rule's
write-up; the tie case that pins both strict inequalities; the header prototype, the ctypes entry, the build list and the
unpinned-parity phrase; every TH_EINVAL of th_lddt; analyse_models.py --lddt with the kernel call replaced by the restatement."""
import csv
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lddt_restatement as lr  # noqa: E402
import superpose_restatement as sr  # noqa: E402
from timed_hip import _lib, lddt, structure, superpose  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHRASE = "PARITY UNPINNED AGAINST OPENSTRUCTURE"


@pytest.fixture(scope="module")
def cases():
    return sr.ubq_cases()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restated_arrays(ref_xyz, mob_xyz, offsets, radius=15.0, thresholds=lr.THRESHOLDS, device=0, timing=None):
    """lddt.lddt_arrays with the GPU call replaced by the restatement"""
    residue, pair, _ = lr.restate_batch(ref_xyz, mob_xyz, offsets, radius, thresholds)
    return lddt.LddtTables(residue, pair)


def restated_superposition(ref_xyz, mob_xyz, offsets, cycles=5, cutoff=2.0, device=0, transform=False, timing=None):
    """superpose.superpose_arrays with the GPU call replaced by its restatement"""
    dist, kept, rmsd, counts, moves, _, _ = sr.restate_batch(ref_xyz, mob_xyz, np.asarray(offsets), cycles, cutoff)
    return superpose.Superposed(dist, kept, rmsd, counts, moves.reshape(-1, 3, 4) if transform else None)


def test_restatement_equals_the_fixture_and_the_written_figures(cases):
    assert os.path.getsize(lr.GOLDEN) < 64 * 1024
    golden = np.load(lr.GOLDEN)
    assert str(golden["sha256"]) == sr.inputs_sha256(cases) and golden["cases"].tolist() == list(lr.CASES)
    again = lr.golden_arrays(cases)
    assert sorted(golden.files) == sorted(again)
    for key in golden.files:
        assert same_bytes(golden[key], np.asarray(again[key])), key
    text = open(os.path.join(ROOT, "tests", "golden", "make_lddt_golden.py")).read()
    assert "NOT by the kernel" in text and PHRASE in text
    want = {"rigid": [76, 2832, 2832, 2832, 2832, 2832], "mirror": [76, 2832, 2832, 2832, 2832, 2832], "noise": [76, 2832, 1538, 2432, 2822, 2832],
            "hinge": [76, 2832, 2136, 2646, 2720, 2760], "invalid": [73, 2582, 1256, 2082, 2562, 2582]}
    edges = []
    for name in lr.CASES:
        a, b = lr.restate(*cases[name]), lr.restate(*cases[name], dtype=np.longdouble)
        print(name, "n_valid, N, C", a["pair"].tolist(), "lddt", lr.score(a["pair"]), "edge", a["edge"])
        assert a["pair"].tolist() == want[name] and a["pair"].dtype == np.int64 and a["residue"].dtype == np.int32
        assert same_bytes(a["residue"], b["residue"]) and same_bytes(a["pair"], b["pair"])        # float64 and long double agree
        assert a["residue"].astype(np.int64).sum(axis=0).tolist() == want[name][1:]
        edges.append(a["edge"])
    assert 6.4e-5 < min(edges) < 6.6e-5
    assert same_bytes(golden["mirror_residue"], golden["rigid_residue"])                          # lDDT does not see a mirror image
    assert lr.score(golden["rigid_pair"]) == 1.0 and round(lr.score(golden["noise_pair"]), 4) == 0.8496
    assert round(lr.score(golden["hinge_pair"]), 4) == 0.9059
    assert sr.restate(*cases["mirror"])["rmsd"][2] > 10.6                                          # ... where the superposition reports 10.7
    invalid = golden["invalid_residue"]
    assert not invalid[[3, 11, 40]].any() and np.delete(invalid[:, 0], [3, 11, 40]).min() >= 6
    for name in ("rigid", "noise", "hinge", "mirror"):
        n_i = golden[f"{name}_residue"][:, 0]
        assert (n_i.min(), n_i.max()) == (6, 63)
    # pair-weighted, not the mean of the per-position scores
    rows = golden["hinge_residue"].astype(np.float64)
    assert abs(np.mean(rows[:, 1:].sum(axis=1) / (4 * rows[:, 0])) - lr.score(golden["hinge_pair"])) > 1e-3
    # an infinity in one list does not leak through the other list's distance
    ref, mob = cases["noise"][0].copy(), cases["noise"][1].copy()
    mob[7, 0] = np.inf
    leak = lr.restate(ref, mob)
    dropped = lr.restate(np.delete(ref, 7, axis=0), np.delete(mob, 7, axis=0))
    assert not leak["residue"][7].any() and same_bytes(np.delete(leak["residue"], 7, axis=0), dropped["residue"])
    assert leak["pair"].tolist() == dropped["pair"].tolist()
    # two different positions with identical coordinates are a pair like any other
    twin = lr.restate(np.zeros((2, 3)), np.array([[0.0, 0, 0], [0.25, 0, 0]]))
    assert twin["residue"].tolist() == [[1, 1, 1, 1, 1]] * 2 and twin["pair"].tolist() == [2, 2, 2, 2, 2, 2]
    empty = lr.restate(np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty["residue"].shape == (0, 5) and empty["pair"].tolist() == [0] * 6 and np.isnan(lr.score(empty["pair"]))


def test_tie_case_pins_both_strict_inequalities():
    pairs, residue, pair = lr.tie_pairs()
    ref, mob, offsets = sr.flatten(pairs)
    for k, (r, m) in enumerate(pairs):                                         # the ties are exact: integer or half-integer roots
        d_ref, d_mob = lr.distances(r), lr.distances(m)
        assert np.array_equal(d_ref, np.round(d_ref)) and np.array_equal(d_mob[d_ref < 15], (np.round(2 * d_mob) / 2)[d_ref < 15]), k
    assert lr.distances(pairs[0][0])[0, 1] == 15.0
    assert sorted({float(abs(lr.distances(r)[0, 1] - lr.distances(m)[0, 1])) for r, m in pairs[1:9]}) == [0.5, 1.0, 2.0, 4.0]
    for dtype in (np.float64, np.longdouble):
        got_residue, got_pair, edge = lr.restate_batch(ref, mob, offsets, dtype=dtype)
        assert edge == 0.0 and same_bytes(got_residue, residue) and same_bytes(got_pair, pair)
    # the neighbours of the ties fall on the other side
    inside, _, _ = lr.restate_batch(ref, mob, offsets, radius=np.nextafter(15.0, 16.0))
    assert inside[:2].tolist() == [[1, 1, 1, 1, 1]] * 2 and inside[-3:, 0].tolist() == [2, 2, 2]
    wider, _, _ = lr.restate_batch(ref, mob, offsets, thresholds=[np.nextafter(t, 8.0) for t in lr.THRESHOLDS])
    assert wider[2:18].tolist() == [[1] + [1 if t <= u else 0 for u in lr.THRESHOLDS] for t in lr.THRESHOLDS for _ in range(4)]


_CTYPES = {"int": "c_int", "int64_t": "c_long", "double": "c_double", "const double*": "c_void_p", "const int64_t*": "c_void_p",
           "int32_t*": "c_void_p", "int64_t*": "c_void_p", "double*": ("c_void_p", "LP_c_double")}


def test_header_ctypes_build_list_and_the_unpinned_parity_phrase():
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    m = re.search(r"^(\w+) th_lddt\(([^;]*)\);", header, re.M)
    assert m
    res, args = _lib.PROTOTYPES["th_lddt"]
    assert res.__name__ == _CTYPES[m.group(1)]
    declared = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(2).split(",")]
    assert len(declared) == len(args) == 11, (declared, args)
    for c_type, ct in zip(declared, args):
        want = _CTYPES[c_type]
        assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (c_type, ct)
    before = header[:m.start()]
    block = before[before.rindex("/* ----"):]                                    # the text above the prototype
    assert block.startswith("/* ---- ") and PHRASE in block and "*** " + PHRASE + " ***" in block
    flat = re.sub(r"[\s*]+", " ", block)
    for words in ("Mariani et al. 2013", "strict inequalities on both tests", "no stereochemistry checks", "not the mean of lddt_i", "MIRROR IMAGES",
                  "no fused multiply-add", "th_packing_threshold"):
        assert words in flat, words
    import __graft_entry__
    assert "lddt.hip" in __graft_entry__.HIP_SOURCES
    source = open(os.path.join(ROOT, "timed-design_amd", "csrc", "lddt.hip")).read()
    assert PHRASE in source and "th_packing_threshold(radius)" in source and "nextafter" not in source       # called, not copied
    import analyse_models
    text = re.sub(r"\s+", " ", analyse_models.build_parser().format_help())
    assert PHRASE in text and "superposition-free" in text and "--lddt_radius" in text and "PARITY UNPINNED AGAINST PYMOL" in text
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert PHRASE in lddt.__doc__ and PHRASE in readme and "mirror" in lddt.__doc__.lower() and "mirror image" in re.sub(r"\s+", " ", readme)
    assert "lddt" not in structure.__doc__.lower() and "lddt" not in superpose.__doc__.lower()       # the new rule lives in its own module
    assert lddt._load_layouts is superpose._load_layouts and lddt.pair_positions is superpose.pair_positions
    assert lddt._POSITION_BYTES == 48 + 20


def test_library_exports_th_lddt_and_checks_arguments_without_a_gpu(lib):
    two = np.zeros((2, 3))
    offsets = np.array([0, 2], np.int64)
    limits = np.array(lr.THRESHOLDS)
    residue, pair = np.full((2, 5), 77, np.int32), np.full((1, 6), 77, np.int64)
    inf, nan = float("inf"), float("nan")

    def call(ref=two, mob=two, total=2, off=offsets, n_pairs=1, radius=15.0, lim=limits, res=residue, par=pair):
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)        # noqa: E731
        ms = C.c_double(-1.0)
        rc = lib.th_lddt(0, p(ref), p(mob), total, p(off), n_pairs, radius, p(lim), p(res), p(par), C.byref(ms))
        assert rc == _lib.TH_OK or ms.value == -1.0
        return rc
    bad = {"negative total": dict(total=-1), "negative pairs": dict(n_pairs=-1), "total too large": dict(total=1 << 31),
           "pairs too large": dict(n_pairs=1 << 31), "offsets NULL": dict(off=None), "thresholds NULL": dict(lim=None), "pair_out NULL": dict(par=None),
           "ref NULL": dict(ref=None), "mob NULL": dict(mob=None), "residue_out NULL": dict(res=None),
           "offsets end": dict(off=np.array([0, 3], np.int64)), "offsets start": dict(off=np.array([1, 2], np.int64)),
           "offsets decrease": dict(off=np.array([0, 2, 1], np.int64), n_pairs=2), "offsets end before total": dict(off=np.array([0, 1], np.int64)),
           "radius 0": dict(radius=0.0), "radius negative": dict(radius=-15.0), "radius nan": dict(radius=nan), "radius inf": dict(radius=inf)}
    for k in range(4):
        for what, v in (("0", 0.0), ("negative", -1.0), ("nan", nan), ("inf", inf)):
            changed = limits.copy()
            changed[k] = v
            bad[f"threshold {k} {what}"] = dict(lim=changed)
    for what, kw in bad.items():
        assert call(**kw) == _lib.TH_EINVAL, what
        assert b"th_lddt" in lib.th_last_error(), what
    assert (residue == 77).all() and (pair == 77).all()
    assert lib.th_lddt(0, None, None, 0, None, 0, 15.0, limits.ctypes.data_as(C.c_void_p), None, None, None) == _lib.TH_OK      # no pairs: no launch
    assert lib.th_lddt(0, None, None, 1, None, 0, 15.0, limits.ctypes.data_as(C.c_void_p), None, None, None) == _lib.TH_EINVAL
    with pytest.raises(ValueError):
        lddt.lddt_arrays(two, two, offsets, thresholds=(1.0, 2.0, 4.0))
    with pytest.raises(ValueError):
        lddt.lddt_arrays(two, np.zeros((3, 3)), offsets)
    with pytest.raises(_lib.TimedHipError) as err:
        lddt.lddt_arrays(two, two, offsets, radius=-1.0)
    assert err.value.code == _lib.TH_EINVAL


def _ca(serial, res, chain, number, xyz, bfactor=None):
    x, y, z = xyz
    tail = "" if bfactor is None else f"  1.00{bfactor:6.2f}           C"
    return f"ATOM  {serial:5d}  CA  {res:>3s} {chain}{number:4d}    {x:8.3f}{y:8.3f}{z:8.3f}{tail}"


def test_analyse_models_lddt_writes_its_two_files_and_leaves_the_others(tmp_path, monkeypatch, cases, capsys):
    import analyse_models
    monkeypatch.setattr(superpose, "superpose_arrays", restated_superposition)
    monkeypatch.setattr(lddt, "lddt_arrays", restated_arrays)
    ref, hinge = cases["hinge"]
    names = [("GLY", "ALA", "SER", "LEU")[k % 4] for k in range(76)]
    plddt = [round(30.0 + 0.9 * k, 2) for k in range(76)]
    (tmp_path / "models").mkdir()
    (tmp_path / "native.pdb").write_text("\n".join(_ca(k + 1, names[k], "A", k + 1, ref[k]) for k in range(76)) + "\nEND\n")
    (tmp_path / "models" / "hinge.pdb").write_text("\n".join(_ca(k + 1, "GLY", "A", k + 1, hinge[k], plddt[k]) for k in range(76)) + "\nEND\n")
    (tmp_path / "models" / "mirror.pdb").write_text(sr.pdb_text(cases["mirror"][1]))
    (tmp_path / "models" / "short.pdb").write_text(sr.pdb_text(hinge[:70]))
    parser = analyse_models.build_parser()
    common = ["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models", str(tmp_path / "models")]
    plain, out = tmp_path / "plain", tmp_path / "out"
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(plain)]))
    assert sorted(p.name for p in plain.iterdir()) == ["model_scores.csv", "residue_deviation.csv"]          # without the flag: the two old files
    assert "3 pairs (1 with an error), 152 positions, 4 files parsed in 1 GPU submission(s)" in capsys.readouterr().out
    parsed = []
    first_model = structure.first_model
    monkeypatch.setattr(structure, "first_model", lambda path: parsed.append(str(path)) or first_model(path))
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(out), "--lddt"]))
    assert sorted(parsed) == sorted(str(p) for p in [tmp_path / "native.pdb"] + list((tmp_path / "models").iterdir()))   # each file read once
    assert "3 pairs (1 with an error), 152 positions, 4 files parsed in 2 GPU submission(s)" in capsys.readouterr().out
    assert sorted(p.name for p in out.iterdir()) == ["model_lddt.csv", "model_scores.csv", "residue_deviation.csv", "residue_lddt.csv"]
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (out / name).read_bytes() == (plain / name).read_bytes()                               # byte for byte what they were

    def read(name):
        with open(out / name, newline="") as f:
            return list(csv.reader(f))
    scores, per = read("model_lddt.csv"), read("residue_lddt.csv")
    assert scores[0] == analyse_models.LDDT_COLUMNS == ["label", "reference", "model", "n_valid", "n_included", "lddt", "preserved_0.5", "preserved_1",
                                                        "preserved_2", "preserved_4", "mean_model_bfactor", "error"]
    assert per[0] == analyse_models.RESIDUE_LDDT_COLUMNS == ["label", "chain", "number", "residue", "n_included", "lddt", "model_bfactor"]
    assert [r[0] for r in scores[1:]] == ["hinge.pdb", "mirror.pdb", "short.pdb"] and len(per) == 1 + 2 * 76
    want = lr.restate(np.round(ref, 3), np.round(hinge, 3))
    row = dict(zip(scores[0], scores[1]))
    n, c = int(want["pair"][1]), want["pair"][2:].tolist()
    assert [int(row["n_valid"]), int(row["n_included"])] == want["pair"][:2].tolist() and row["error"] == ""
    assert [float(row[f"preserved_{t}"]) for t in ("0.5", "1", "2", "4")] == [v / n for v in c] and float(row["lddt"]) == sum(c) / (4 * n)
    assert float(row["mean_model_bfactor"]) == float(np.mean(plddt))
    mine = [r for r in per[1:] if r[0] == "hinge.pdb"]
    assert [r[1] for r in mine] == ["A"] * 76 and [r[2] for r in mine] == [str(k + 1) for k in range(76)] and [r[3] for r in mine] == names
    assert [int(r[4]) for r in mine] == want["residue"][:, 0].tolist() and [float(r[6]) for r in mine] == plddt
    rows = want["residue"].astype(np.int64)
    assert [float(r[5]) for r in mine] == [int(rows[k, 1:].sum()) / (4 * int(rows[k, 0])) for k in range(76)]
    mirror = dict(zip(scores[0], scores[2]))
    assert float(mirror["lddt"]) > 0.999 and mirror["mean_model_bfactor"] == "0.0"                  # rounded to three decimals, still ~1
    assert "length mismatch" in scores[3][-1] and scores[3][3:5] == ["0", "0"] and scores[3][5] == "nan" and scores[3][10] == "nan"
    args = parser.parse_args(["--pairs", "p.csv"])
    assert args.lddt is False and args.lddt_radius == 15.0
    with pytest.raises(SystemExit):
        analyse_models.main(parser.parse_args(common + ["--path_to_output", str(out), "--lddt", "--lddt_radius", "0"]))


def test_lddt_results_pairing_bfactors_and_the_byte_budget(tmp_path, monkeypatch):
    calls = []

    def counted(ref_xyz, mob_xyz, offsets, *a, **kw):
        calls.append(len(offsets) - 1)
        return restated_arrays(ref_xyz, mob_xyz, offsets, *a, **kw)
    monkeypatch.setattr(lddt, "lddt_arrays", counted)
    rng = np.random.default_rng(3)
    ca = np.round(np.cumsum(rng.normal(0, 2.2, (6, 3)), axis=0), 3)
    moved = np.round(ca @ sr.rotation(rng).T + 4.0, 3)
    (tmp_path / "native.pdb").write_text("\n".join(_ca(k + 1, "ALA", "A", 10 + k, ca[k]) for k in range(6)) + "\nEND\n")
    (tmp_path / "model.pdb").write_text("\n".join(_ca(k + 1, "GLY", "A", 10 + k, moved[k], 90.0 - k) for k in (0, 2, 3, 5)) + "\n"
                                        + _ca(9, "GLY", "B", 1, moved[1]) + "\nEND\n")          # no B-factor column on the last atom
    stats = {}
    first, second, third = lddt.lddt([(tmp_path / "native.pdb", tmp_path / "model.pdb"), (tmp_path / "native.pdb", tmp_path / "absent.pdb"),
                                      (tmp_path / "model.pdb", tmp_path / "model.pdb")], stats=stats)
    assert stats["files_parsed"] == 3 and stats["submissions"] == 1 and calls == [1]
    assert "length mismatch" in first.error and np.isnan(first.lddt) and first.n_included == 0 and len(first.lddt_i) == 0
    assert "absent.pdb" in second.error
    assert third.error is None and third.lddt == 1.0 and third.preserved == (1.0, 1.0, 1.0, 1.0) and third.n_valid == 5
    assert third.model_bfactor[:4].tolist() == [90.0, 88.0, 87.0, 85.0] and np.isnan(third.model_bfactor[4])
    (numbered,) = lddt.lddt([(tmp_path / "native.pdb", tmp_path / "model.pdb")], pair_by="number")
    assert numbered.error is None and [r.number for r in numbered.residues] == ["10", "12", "13", "15"] and [r.name for r in numbered.residues] == ["ALA"] * 4
    assert (numbered.unpaired_reference, numbered.unpaired_model) == (2, 1) and numbered.model_bfactor.tolist() == [90.0, 88.0, 87.0, 85.0]
    want = lr.restate(ca[[0, 2, 3, 5]], moved[[0, 2, 3, 5]])
    assert numbered.n_i.tolist() == want["residue"][:, 0].tolist() and numbered.n_included == want["pair"][1] and numbered.lddt == lr.score(want["pair"])
    with pytest.raises(ValueError):
        lddt.lddt([], pair_by="alignment")
    assert lddt.lddt([]) == []
    assert lddt.fractions([4, 1, 2, 3, 4]) == ((0.25, 0.5, 0.75, 1.0), 0.625) and np.isnan(lddt.fractions([0, 0, 0, 0, 0])[1])
    # batches are cut with the structure budget: 68 bytes per position, nothing per pair of positions
    from timed_hip import pdbio
    layouts = []
    for n in (30, 30, 30, 30, 30):
        ref, mob = sr.synthetic_pair(n, rng)
        residues = [pdbio.Residue("A", str(k + 1), "GLY") for k in range(n)]
        layouts.append((superpose.AtomLayout(ref, residues), superpose.AtomLayout(mob, residues)))
    del calls[:]
    whole = lddt.lddt(layouts)
    split = lddt.lddt(layouts, budget_bytes=2 * 30 * lddt._POSITION_BYTES + 100, stats=stats)       # two pairs of 30 fit, three do not
    assert calls == [5, 2, 2, 1] and stats["submissions"] == 4
    for a, b in zip(whole, split):
        assert same_bytes(a.lddt_i, b.lddt_i) and same_bytes(a.n_i, b.n_i) and a.lddt == b.lddt and np.isnan(a.model_bfactor).all()
