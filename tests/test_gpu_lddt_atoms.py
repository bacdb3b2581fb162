"""th_lddt_atoms on the GPU against the committed fixture of the NumPy restatement (tests/lddt_atoms_restatement.py): every case as
bytes, alone in spirit and together in one batch with an empty pair among them, in both orders and twice; the CA-only form against
th_lddt; TH_LDDT_NO_SYMMETRY; lddt_atoms() on files under two byte budgets; analyse_models.py --lddt_all_atom and build_sidechains.py
--lddt end to end.

All outputs are integers and must be exact.  That is fair because tests/golden/make_lddt_atoms_golden.py asserted, on the
restatement, that no float decision of a non-tie case lies within 1e-9 Angstrom of its boundary, that no symmetric residue of such a
case has swap_R == keep_R, and that float64 and long double give the same integers; the hand-made tie cases have exact roots, so the
strict inequalities alone decide them.  The largest input is 1ubq's 601 atoms: three tiles of 256 with a partial last one.
"""
import csv
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lddt_atoms_restatement as ar  # noqa: E402
from timed_hip import lddt, lddt_atoms, pdbio  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(ar.GOLDEN)


@pytest.fixture(scope="module")
def batch(golden):
    """every case of the fixture and an empty pair in their midst, flattened: computed once, shared, never changed"""
    cases = ar.golden_cases(golden)
    empty = dict(ref=np.zeros((0, 3)), mob=np.zeros((0, 3)), residue=np.zeros(0, np.int32), partner=np.zeros(0, np.int32))
    names = list(cases)
    names.insert(5, "")
    return names, [cases[name] if name else empty for name in names]


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(got, names, offsets, golden, tag=""):
    for k, name in enumerate(names):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        if not name:
            assert lo == hi and got.pair[k].tolist() == [0] * 8
            continue
        print(name + tag, "n_ref, n_missing, N, C, swapped", got.pair[k].tolist(), "lddt", ar.score(got.pair[k]))
        assert same_bytes(got.atom[lo:hi], golden[f"{name}{tag}_atom"]), name
        assert same_bytes(got.swapped[lo:hi], golden[f"{name}{tag}_swapped"]), name
        assert same_bytes(got.pair[k], golden[f"{name}{tag}_pair"]), name


def test_every_case_in_one_batch_both_orders_and_twice(gpu, golden, batch):
    names, cases = batch
    assert str(golden["sha256"]) == ar.inputs_sha256({name: case for name, case in zip(names, cases) if name})
    flat = ar.flatten(cases)
    got = lddt_atoms.lddt_atoms_arrays(*flat, device=gpu)
    assert got.atom.dtype == np.int32 and got.swapped.dtype == np.uint8 and got.pair.dtype == np.int64 and got.pair.shape == (len(names), 8)
    check(got, names, flat[4], golden)
    again = lddt_atoms.lddt_atoms_arrays(*flat, device=gpu)
    assert same_bytes(again.atom, got.atom) and same_bytes(again.swapped, got.swapped) and same_bytes(again.pair, got.pair)     # two calls: the same bytes
    back = ar.flatten(cases[::-1])
    check(lddt_atoms.lddt_atoms_arrays(*back, device=gpu), names[::-1], back[4], golden)                  # a pair's place does not matter
    # the figures of the write-up
    k, f = names.index("self"), names.index("flipped")
    assert got.pair[k].tolist() == [601, 0, 171464, 171464, 171464, 171464, 171464, 0] and got.pair[f].tolist() == got.pair[k, :7].tolist() + [31]
    assert got.swapped[flat[4][f]:flat[4][f + 1]].sum() == 68 and ar.score(got.pair[f]) == 1.0


def test_no_symmetry_scores_the_model_as_named(gpu, golden, batch):
    names, cases = batch
    flat = ar.flatten(cases)
    got = lddt_atoms.lddt_atoms_arrays(*flat, symmetry=False, device=gpu)
    check(got, names, flat[4], golden, "_named")
    f = names.index("flipped")
    assert got.pair[f, 3] < got.pair[f, 2] and round(ar.score(got.pair[f]), 3) == 0.918 and not got.swapped.any()
    assert got.pair[f].tolist() == [601, 0, 171464, 142358, 150584, 165278, 171418, 0]
    case = cases[f]                                                              # partner is ignored: garbage in it changes nothing
    alone = lddt_atoms.lddt_atoms_arrays(case["ref"], case["mob"], case["residue"], np.full(601, 7, np.int32), [0, 601], symmetry=False, device=gpu)
    assert same_bytes(alone.atom, golden["flipped_named_atom"]) and same_bytes(alone.pair[0], golden["flipped_named_pair"])


def test_ca_atoms_alone_give_the_counts_of_th_lddt(gpu, golden):
    names = ar.ubq()
    ca = np.array([r.atoms["CA"] for r in names.residues if not r.hetero and "CA" in r.atoms])
    rng = np.random.default_rng(5)
    pairs = [(ca, ca + rng.normal(0.0, 0.5, ca.shape)), (ca[:40], ca[:40] + rng.normal(0.0, 1.5, (40, 3))), (ca[:1], ca[:1])]
    ref, mob = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    offsets = np.array([0, 76, 116, 117], np.int64)
    residue = np.concatenate([np.arange(76), np.arange(40), np.arange(1)]).astype(np.int32)
    want = lddt.lddt_arrays(ref, mob, offsets, device=gpu)
    got = lddt_atoms.lddt_atoms_arrays(ref, mob, residue, np.full(117, -1, np.int32), offsets, device=gpu)
    assert same_bytes(got.atom, want.residue) and same_bytes(np.ascontiguousarray(got.pair[:, 2:7]), np.ascontiguousarray(want.pair[:, 1:6]))
    assert got.pair[:, 0].tolist() == [76, 40, 1] and not got.pair[:, [1, 7]].any() and 0 < got.pair[0, 3] < got.pair[0, 2]


def _flipped(model):
    out = pdbio.Model(1, [pdbio.Residue(r.chain, r.number, r.name, dict(r.atoms), dict(r.elements)) for r in model.residues])
    for res in out.residues:
        for a, b in ar.SYMMETRIC.get(res.name, ()):
            res.atoms[a], res.atoms[b] = res.atoms[b], res.atoms[a]
    return out


def test_files_under_two_byte_budgets(gpu, golden, tmp_path):
    native = ar.ubq()
    pdbio.write_pdb(tmp_path / "flipped.pdb", _flipped(native))
    pairs = [(ar.UBQ, ar.UBQ), (ar.UBQ, tmp_path / "flipped.pdb"), (ar.UBQ, tmp_path / "absent.pdb"), (ar.UBQ, ar.UBQ)]
    once, twice = {}, {}
    whole = lddt_atoms.lddt_atoms(pairs, device=gpu, stats=once)
    split = lddt_atoms.lddt_atoms(pairs, device=gpu, budget_bytes=2 * 601 * lddt_atoms._ATOM_BYTES + 100, stats=twice)
    assert once["submissions"] == 1 and twice["submissions"] == 2 and once["files_parsed"] == 3 and once["kernel_ms"] > 0
    for a, b in zip(whole, split):
        assert a.error == b.error and same_bytes(a.n_i, b.n_i) and same_bytes(a.lddt_i, b.lddt_i) and same_bytes(a.swapped, b.swapped)
        assert (a.n_atoms, a.n_missing, a.n_included, a.n_swapped_residues) == (b.n_atoms, b.n_missing, b.n_included, b.n_swapped_residues)
        assert a.preserved == b.preserved or a.error
    assert "absent.pdb" in whole[2].error and whole[0].lddt == 1.0 and whole[1].lddt == 1.0 and whole[1].n_swapped_residues == 31
    assert whole[0].n_atoms == 601 and whole[0].n_included == 171464 and whole[0].lddt_sidechain == 1.0 and whole[1].swapped.sum() == 31
    from design_utils.analyse_utils import calculate_all_atom_lddt
    assert calculate_all_atom_lddt(ar.UBQ, tmp_path / "flipped.pdb", device=gpu) == 1.0
    with pytest.raises(ValueError):
        calculate_all_atom_lddt(ar.UBQ, tmp_path / "absent.pdb", device=gpu)


def test_command_lines_end_to_end(gpu, tmp_path, capsys):
    import analyse_models
    import build_sidechains

    def read(path):
        with open(path, newline="") as f:
            return list(csv.reader(f))
    (tmp_path / "models").mkdir()
    pdbio.write_pdb(tmp_path / "models" / "flipped.pdb", _flipped(ar.ubq()))
    pdbio.write_pdb(tmp_path / "models" / "same.pdb", ar.ubq())
    parser = analyse_models.build_parser()
    common = ["--path_to_reference", ar.UBQ, "--path_to_models", str(tmp_path / "models"), "--device", str(gpu)]
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "out"), "--lddt_all_atom"]))
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["model_lddt_all_atom.csv", "model_scores.csv", "residue_deviation.csv",
                                                                     "residue_lddt_all_atom.csv"]
    rows, per = read(tmp_path / "out" / "model_lddt_all_atom.csv"), read(tmp_path / "out" / "residue_lddt_all_atom.csv")
    assert rows[0] == lddt_atoms.MODEL_COLUMNS and per[0] == lddt_atoms.RESIDUE_COLUMNS and len(per) == 1 + 2 * 76
    flipped, same = dict(zip(rows[0], rows[1])), dict(zip(rows[0], rows[2]))
    assert same["label"] == "same.pdb" and float(same["lddt"]) == 1.0 and same["n_atoms"] == "601" and same["n_swapped_residues"] == "0"
    assert float(flipped["lddt"]) == 1.0 and flipped["n_swapped_residues"] == "31" and flipped["n_included"] == "171464" and flipped["error"] == ""
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "named"), "--lddt_all_atom", "--lddt_no_symmetry"]))
    named = dict(zip(rows[0], read(tmp_path / "named" / "model_lddt_all_atom.csv")[1]))
    assert round(float(named["lddt"]), 3) == 0.918 and named["n_swapped_residues"] == "0" and float(named["lddt_backbone"]) > float(named["lddt_sidechain"])
    # build_sidechains.py --chi native --lddt: the native angles rebuilt on the ideal geometry of the table
    (tmp_path / "pdb").mkdir()
    pdbio.write_pdb(tmp_path / "pdb" / "1ubq.pdb", ar.ubq())
    parser = build_sidechains.build_parser()
    build_sidechains.main(parser.parse_args(["--path_to_pdb", str(tmp_path / "pdb"), "--path_to_output", str(tmp_path / "built"), "--chi", "native",
                                             "--lddt", "--device", str(gpu)]))
    assert sorted(p.name for p in (tmp_path / "built").iterdir()) == ["1ubq_native_chi.pdb", "residue_sidechain_lddt.csv", "residue_sidechains.csv",
                                                                       "structure_sidechain_lddt.csv", "structure_sidechains.csv"]
    rows, per = read(tmp_path / "built" / "structure_sidechain_lddt.csv"), read(tmp_path / "built" / "residue_sidechain_lddt.csv")
    row = dict(zip(rows[0], rows[1]))
    with capsys.disabled():
        print("build_sidechains --chi native --lddt:", row)
    assert rows[0] == lddt_atoms.MODEL_COLUMNS and len(per) == 77 and row["error"] == "" and row["n_atoms"] == "601" and row["n_mismatched_residues"] == "0"
    assert float(row["lddt_backbone"]) > float(row["lddt_sidechain"]) > 0.5 and float(row["lddt"]) < 1.0       # 0.35 Angstrom RMSD: most pairs preserved
