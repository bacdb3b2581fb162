"""Superposition without a GPU: the NumPy restatement (tests/superpose_restatement.py) against an independent SVD Kabsch and the
committed fixture; pairing by position and by number on hand-written PDB text; analyse_models.py with the kernel call replaced by the
restatement; the header prototype, the ctypes entry and the build list."""
import csv
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import superpose_restatement as sr  # noqa: E402
from timed_hip import _lib, pdbio, structure, superpose  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHRASE = "PARITY UNPINNED AGAINST PYMOL"


@pytest.fixture(scope="module")
def cases():
    return sr.ubq_cases()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restated_arrays(ref_xyz, mob_xyz, offsets, cycles=5, cutoff=2.0, device=0, transform=False, timing=None):
    """superpose.superpose_arrays with the GPU call replaced by the restatement"""
    dist, kept, rmsd, counts, moves, _, _ = sr.restate_batch(ref_xyz, mob_xyz, np.asarray(offsets), cycles, cutoff)
    return superpose.Superposed(dist, kept, rmsd, counts, moves.reshape(-1, 3, 4) if transform else None)


def test_fit_over_all_agrees_with_svd_kabsch_on_every_case(cases):
    pairs = list(cases.items()) + [(f"ragged{k}", p) for k, p in enumerate(sr.ragged_batch()) if len(p[0]) >= 3]
    pairs += [(f"degenerate{k}", p) for k, p in enumerate(sr.degenerate_pairs()) if len(p[0]) >= 2]
    worst = 0.0
    for name, (ref, mob) in pairs:
        got = float(sr.restate(ref, mob, cycles=0)["rmsd"][2])
        want = sr.kabsch_rmsd(ref, mob)
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 1e-12 * max(1.0, want), (name, got, want)
    print("restatement rmsd_fit_all vs SVD Kabsch, worst difference over", len(pairs), "pairs:", worst)
    mirror = sr.restate(*cases["mirror"])
    assert 10.6 < mirror["rmsd"][2] < 10.8                                       # a mirror image is not superposable: not 0
    assert sr.restate(*cases["rigid"], cycles=0)["rmsd"][2] < 1e-12
    hinge = sr.restate(*cases["hinge"])
    assert hinge["counts"][2] >= 2 and hinge["counts"][1] < 76 and hinge["rmsd"][0] < 0.6 < 2.0 < hinge["rmsd"][2]
    assert not hinge["kept"][70:].any() and hinge["kept"][:60].sum() >= 57      # the refinement finds the re-oriented tail
    noise = sr.restate(*cases["noise"])
    assert noise["counts"][:3].tolist() == [76, 76, 0] and same_bytes(noise["rmsd"][:1], noise["rmsd"][2:])
    invalid = sr.restate(*cases["invalid"])
    assert invalid["counts"][0] == 73 and np.isnan(invalid["dist"][[3, 11, 40]]).all() and not invalid["kept"][[3, 11, 40]].any()
    empty = sr.restate(np.full((4, 3), np.nan), np.zeros((4, 3)))
    assert np.isnan(empty["rmsd"]).all() and not empty["counts"].any() and np.isnan(empty["dist"]).all()


def test_float64_restatement_against_long_double(cases):
    for name, (ref, mob) in cases.items():
        a = sr.restate(ref, mob, cycles=sr.CASE_CYCLES[name])
        b = sr.restate(ref, mob, cycles=sr.CASE_CYCLES[name], dtype=np.longdouble)
        err = float(np.nanmax(np.abs(a["dist"].astype(np.longdouble) - b["dist"])))
        print(f"{name}: float64 restatement vs long double, worst d_i error {err:.3e} Angstrom; nearest edge {a['edge']:.3e}, eigenvalue gap {a['gap']:.3e}")
        assert same_bytes(a["kept"], b["kept"]) and same_bytes(a["counts"], b["counts"])
        assert err < 1e-12 and a["edge"] > 1e-9 and a["gap"] > 1e-6


def test_fixture_regenerates_to_the_same_bytes(cases):
    assert os.path.getsize(sr.GOLDEN) < 64 * 1024
    golden = np.load(sr.GOLDEN)
    assert str(golden["sha256"]) == sr.inputs_sha256(cases)
    again = sr.golden_arrays(cases)
    assert sorted(golden.files) == sorted(again)
    for key in golden.files:
        assert same_bytes(golden[key], np.asarray(again[key])), key
    assert golden["cases"].tolist() == list(sr.CASES) and len(golden["hinge_dist"]) == 76
    text = open(os.path.join(ROOT, "tests", "golden", "make_superpose_golden.py")).read()
    assert "NOT by the kernel" in text and PHRASE in text


def _atom(serial, name, res, chain, number, xyz, het=False, alt=" "):
    x, y, z = xyz
    return f"{'HETATM' if het else 'ATOM  '}{serial:5d} {name:<4s}{alt}{res:>3s} {chain}{number:>5s}   {x:8.3f}{y:8.3f}{z:8.3f}  1.00  0.00"


def _write(path, lines):
    path.write_text("\n".join(lines) + "\nEND\n")
    return path


def test_pairing_by_position_and_by_number(tmp_path, monkeypatch):
    monkeypatch.setattr(superpose, "superpose_arrays", restated_arrays)
    rng = np.random.default_rng(4)
    ca = np.round(np.cumsum(rng.normal(0, 2.2, (6, 3)), axis=0), 3)
    names = ["MET", "GLN", "ILE", "PHE", "VAL", "LYS"]
    native = [_atom(2 * k + 1, " N", names[k], "A", str(10 + k) + " ", ca[k] + 1.0) for k in range(6)]
    for k in range(6):
        native.insert(2 * k + 1, _atom(2 * k + 2, " CA", names[k], "A", str(10 + k) + " ", ca[k]))
    native.insert(4, _atom(90, " CA", names[1], "A", "11 ", ca[1] + 5.0, alt="B"))       # a second alternate location: ignored
    native.append(_atom(99, " CA", "HOH", "A", "200 ", (0.0, 0.0, 0.0), het=True))       # HETATM: ignored
    ref = _write(tmp_path / "native.pdb", native)
    turned = np.round(ca @ sr.rotation(rng).T + 4.0, 3)
    design = ["MET", "ALA", "ILE", "PHE", "TRP", "LYS"]
    same = _write(tmp_path / "model.pdb", ["MODEL        1"] + [_atom(k + 1, " CA", design[k], "A", str(k + 1) + " ", turned[k]) for k in range(6)]
                  + ["ENDMDL", "MODEL        2"] + [_atom(k + 1, " CA", design[k], "A", str(k + 1) + " ", turned[k] + 9.0 * k) for k in range(6)] + ["ENDMDL"])
    short = _write(tmp_path / "short.pdb", [_atom(k + 1, " CA", design[k], "A", str(10 + k) + " ", turned[k]) for k in (0, 2, 3, 5)]
                   + [_atom(9, " CA", "GLY", "A", "15A", turned[5] + 1.0), _atom(10, " CA", "GLY", "B", "10 ", turned[0]),
                      _atom(11, " CA", "GLY", "B", "11 ", turned[1])])
    stats = {}
    by_position = superpose.superpose([(ref, same), (ref, short), (ref, tmp_path / "absent.pdb")], stats=stats)
    assert stats["files_parsed"] == 4 and stats["submissions"] == 1
    first, second, third = by_position
    assert first.error is None and first.n_valid == 6 and len(first.dist) == 6 and first.rmsd_fit_all < 2e-3      # three decimals
    assert first.sequence_identity == 4 / 6 and [r.number for r in first.residues] == ["10", "11", "12", "13", "14", "15"]
    assert first.gdt == (1.0, 1.0, 1.0, 1.0) and first.mean_gdt == 1.0 and (first.unpaired_reference, first.unpaired_model) == (0, 0)
    assert "length mismatch" in second.error and "6" in second.error and "7" in second.error and np.isnan(second.rmsd_kept) and second.n_valid == 0
    assert "absent.pdb" in third.error
    (numbered,) = superpose.superpose([(ref, short)], pair_by="number")
    assert numbered.error is None and [r.number for r in numbered.residues] == ["10", "12", "13", "15"]
    assert (numbered.unpaired_reference, numbered.unpaired_model) == (2, 3) and numbered.sequence_identity == 1.0
    assert numbered.n_valid == 4 and numbered.rmsd_fit_all < 2e-3
    (renumbered,) = superpose.superpose([(ref, same)], pair_by="number")                 # 1..6 against 10..15: nothing in common
    assert renumbered.error is None and renumbered.n_valid == 0 and np.isnan(renumbered.rmsd_kept) and renumbered.unpaired_model == 6
    with pytest.raises(ValueError):
        superpose.superpose([(ref, same)], pair_by="alignment")
    # models and layouts are taken as they are; a shared native is laid out once
    model = structure.first_model(ref)
    lay = superpose.atom_layout(model)
    assert lay.xyz.shape == (6, 3) and same_bytes(lay.xyz, ca)
    a, b = superpose.superpose([(model, same), (lay, same)], transform=True)
    assert same_bytes(a.dist, first.dist) and same_bytes(b.dist, first.dist) and a.transform.shape == (3, 4)
    assert np.abs(turned @ a.transform[:, :3].T + a.transform[:, 3] - ca).max() < 5e-3
    assert superpose.superpose([]) == []
    assert superpose.gdt_fractions(np.array([4, 4, 0, 1, 2, 3, 4]))[0] == (0.25, 0.5, 0.75, 1.0)


def test_batches_are_cut_with_the_structure_budget(monkeypatch):
    calls = []

    def counted(ref_xyz, mob_xyz, offsets, *a, **kw):
        calls.append(len(offsets) - 1)
        return restated_arrays(ref_xyz, mob_xyz, offsets, *a, **kw)
    monkeypatch.setattr(superpose, "superpose_arrays", counted)
    rng = np.random.default_rng(1)
    layouts = []
    for n in (30, 30, 30, 30, 30):
        ref, mob = sr.synthetic_pair(n, rng)
        residues = [pdbio.Residue("A", str(k + 1), "GLY") for k in range(n)]
        layouts.append((superpose.AtomLayout(ref, residues), superpose.AtomLayout(mob, residues)))
    whole = superpose.superpose(layouts)
    assert calls == [5]
    budget = 2 * 70 * structure._ATOM_BYTES                                      # two pairs of 30 fit, three do not
    assert 2 * structure._ATOM_BYTES >= superpose._POSITION_BYTES
    stats = {}
    split = superpose.superpose(layouts, budget_bytes=budget, stats=stats)
    assert calls == [5, 2, 2, 1] and stats["submissions"] == 3 and stats["files_parsed"] == 0
    for a, b in zip(whole, split):
        assert same_bytes(a.dist, b.dist) and same_bytes(a.kept, b.kept) and a.rmsd_kept == b.rmsd_kept


def test_analyse_models_writes_both_files(tmp_path, monkeypatch, cases, capsys):
    import analyse_models
    monkeypatch.setattr(superpose, "superpose_arrays", restated_arrays)
    ref, hinge = cases["hinge"]
    (tmp_path / "models" / "t1").mkdir(parents=True)
    (tmp_path / "native.pdb").write_text(sr.pdb_text(ref))
    (tmp_path / "models" / "t1" / "hinge.pdb").write_text(sr.pdb_text(hinge))
    (tmp_path / "models" / "noise.ent").write_text(sr.pdb_text(cases["noise"][1]))
    (tmp_path / "models" / "short.pdb").write_text(sr.pdb_text(hinge[:70]))
    (tmp_path / "models" / "notes.txt").write_text("not a structure\n")
    out = tmp_path / "out"
    parser = analyse_models.build_parser()
    analyse_models.main(parser.parse_args(["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models", str(tmp_path / "models"),
                                           "--path_to_output", str(out)]))
    assert "3 pairs (1 with an error), 152 positions, 4 files parsed in 1 GPU submission(s)" in capsys.readouterr().out
    with open(out / "model_scores.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == analyse_models.SCORE_COLUMNS == ["label", "reference", "model", "n_valid", "n_kept", "cycles_run", "rmsd_kept", "rmsd_all",
                                                       "rmsd_fit_all", "gdt_1", "gdt_2", "gdt_4", "gdt_8", "mean_gdt", "sequence_identity",
                                                       "unpaired_reference", "unpaired_model", "error"]
    assert [r[0] for r in rows[1:]] == ["noise.ent", "short.pdb", "t1/hinge.pdb"]
    want = sr.restate(np.round(ref, 3), np.round(hinge, 3))
    got = dict(zip(rows[0], rows[3]))
    assert [int(got[k]) for k in ("n_valid", "n_kept", "cycles_run")] == want["counts"][:3].tolist()
    assert [float(got[k]) for k in ("rmsd_kept", "rmsd_all", "rmsd_fit_all")] == want["rmsd"].tolist()
    fractions = [c / 76 for c in want["counts"][3:].tolist()]
    assert [float(got[f"gdt_{k}"]) for k in (1, 2, 4, 8)] == fractions and float(got["mean_gdt"]) == float(np.mean(fractions))
    assert got["sequence_identity"] == "1.0" and got["error"] == ""
    assert "length mismatch" in rows[2][-1] and rows[2][3:6] == ["0", "0", "0"] and rows[2][6] == "nan"
    with open(out / "residue_deviation.csv", newline="") as f:
        per = list(csv.reader(f))
    assert per[0] == ["label", "chain", "residue_number", "distance", "kept"] and len(per) == 1 + 2 * 76
    mine = [r for r in per[1:] if r[0] == "t1/hinge.pdb"]
    assert [r[2] for r in mine] == [str(k + 1) for k in range(76)] and {r[1] for r in mine} == {"A"}
    assert [float(r[3]) for r in mine] == want["dist"].tolist() and [int(r[4]) for r in mine] == want["kept"].tolist()
    # the --pairs form: relative paths from the CSV's directory, an optional label, comment and empty lines
    (tmp_path / "pairs.csv").write_text("# reference,model,label\nnative.pdb,models/t1/hinge.pdb,first\n\nnative.pdb,models/noise.ent\n")
    analyse_models.main(parser.parse_args(["--pairs", str(tmp_path / "pairs.csv"), "--path_to_output", str(out), "--cycles", "0", "--pair_by", "number"]))
    with open(out / "model_scores.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert [r[0] for r in rows[1:]] == ["first", "models/noise.ent"] and rows[1][5] == "0" and rows[1][6] == rows[1][7] == rows[1][8]
    for bad in (["--pairs", str(tmp_path / "pairs.csv"), "--path_to_reference", "x"], ["--path_to_reference", str(tmp_path / "native.pdb")], []):
        with pytest.raises(SystemExit):
            analyse_models.main(parser.parse_args(bad + ["--path_to_output", str(out)]))
    args = parser.parse_args(["--pairs", "p.csv"])
    assert (args.cycles, args.cutoff, args.pair_by, args.device, args.path_to_output) == (5, 2.0, "position", 0, "model_scores")


def test_calculate_rmsd_and_gdt_under_the_reference_name(tmp_path, monkeypatch, cases):
    from design_utils import analyse_utils as au
    monkeypatch.setattr(superpose, "superpose_arrays", restated_arrays)
    ref, hinge = cases["hinge"]
    (tmp_path / "native.pdb").write_text(sr.pdb_text(ref))
    (tmp_path / "hinge.pdb").write_text(sr.pdb_text(hinge))
    (tmp_path / "short.pdb").write_text(sr.pdb_text(hinge[:9]))
    want = sr.restate(np.round(ref, 3), np.round(hinge, 3))
    rmsd, mean_gdt = au.calculate_RMSD_and_gdt(tmp_path / "native.pdb", tmp_path / "hinge.pdb")
    assert rmsd == float(want["rmsd"][0]) and mean_gdt == float(np.mean([c / 76 for c in want["counts"][3:].tolist()]))
    with pytest.raises(ValueError, match="length mismatch"):
        au.calculate_RMSD_and_gdt(tmp_path / "native.pdb", tmp_path / "short.pdb")


_CTYPES = {"int": "c_int", "int64_t": "c_long", "double": "c_double", "const double*": "c_void_p", "const int64_t*": "c_void_p",
           "uint8_t*": "c_void_p", "int32_t*": "c_void_p", "double*": ("c_void_p", "LP_c_double")}


def test_header_ctypes_build_list_and_the_unpinned_parity_phrase():
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    m = re.search(r"^(\w+) th_superpose\(([^;]*)\);", header, re.M)
    assert m
    res, args = _lib.PROTOTYPES["th_superpose"]
    assert res.__name__ == _CTYPES[m.group(1)]
    declared = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(2).split(",")]
    assert len(declared) == len(args) == 14, (declared, args)
    for c_type, ct in zip(declared, args):
        want = _CTYPES[c_type]
        assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (c_type, ct)
    before = header[:m.start()]
    assert PHRASE in before[before.rindex("/* ----"):]                          # in the text above the prototype
    import __graft_entry__
    assert "superpose.hip" in __graft_entry__.HIP_SOURCES
    import analyse_models
    text = analyse_models.build_parser().format_help()
    assert PHRASE in text and "by position" in re.sub(r"\s+", " ", text) and "NOT by a sequence alignment" in re.sub(r"\s+", " ", text)
    assert PHRASE in superpose.__doc__ and PHRASE in open(os.path.join(ROOT, "README.md")).read()
    assert "superpose" not in structure.__doc__                                 # the new rule lives in its own module


def test_library_exports_th_superpose_and_checks_arguments_without_a_gpu(lib):
    import ctypes as C
    one = np.zeros((1, 3))
    offsets = np.array([0, 1], np.int64)
    dist, kept, rmsd, counts = np.full(1, 6.5), np.full(1, 9, np.uint8), np.full((1, 3), 6.5), np.full((1, 7), 77, np.int32)

    def call(total=1, off=offsets, n_pairs=1, cycles=5, cutoff=2.0, r=rmsd):
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)        # noqa: E731
        return lib.th_superpose(0, p(one), p(one), total, p(off), n_pairs, cycles, cutoff, p(dist), p(kept), p(r), p(counts), None, None)
    for what, kw in {"negative total": dict(total=-1), "negative pairs": dict(n_pairs=-1), "too large": dict(total=1 << 31), "cycles": dict(cycles=-1),
                     "cutoff 0": dict(cutoff=0.0), "cutoff nan": dict(cutoff=float("nan")), "cutoff inf": dict(cutoff=float("inf")),
                     "offsets NULL": dict(off=None), "rmsd NULL": dict(r=None), "end": dict(off=np.array([0, 2], np.int64)),
                     "start": dict(off=np.array([1, 1], np.int64)), "decrease": dict(off=np.array([0, 2, 1], np.int64), n_pairs=2)}.items():
        assert call(**kw) == _lib.TH_EINVAL, what
        assert b"th_superpose" in lib.th_last_error(), what
    assert (dist == 6.5).all() and (kept == 9).all() and (rmsd == 6.5).all() and (counts == 77).all()
    assert lib.th_superpose(0, None, None, 0, None, 0, 5, 2.0, None, None, None, None, None, None) == _lib.TH_OK      # no pairs: no launch
