"""Rotamer labels without a GPU: the NumPy restatement (tests/rotamer_restatement.py) against the committed fixture and the figures
the rule gives on 1ubq; th_rotamer_table (host code of csrc/rotamers.hip) against the Python tables; the flat layout; labels in
dataset-map order; the reference's file rule; the command lines, with the GPU call replaced by the restatement."""
import json
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rotamer_restatement as rr  # noqa: E402
from timed_hip import _lib, pdbio, structure  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST_TWENTY = [162, 217, 60, 46, 318, 108, 314, 156, 314, 49, 109, 316, 63, 314, 155, 35, 319, 39, 200, 311]
REDUCTION_GUIDE = [0, 1, 4, 13, 40, 49, 50, 59, 68, 149, 158, 185, 194, 203, 230, 311, 314, 317, 320, 329]


@pytest.fixture(scope="module")
def golden():
    return np.load(rr.GOLDEN)


@pytest.fixture(scope="module")
def ubq():
    return rr.residues_of_model(pdbio.read_pdb(rr.UBQ)[0])


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restated(layouts, device=0, ala_gly_class=True, budget_bytes=None, stats=None):
    """structure.tag_rotamers with the GPU call replaced by the restatement"""
    out = []
    for lay in layouts:
        lay = lay if isinstance(lay, structure.RotamerLayout) else structure.rotamer_layout(structure.first_model(lay))
        cls, chi = rr.restate([(r.name, list(r.atoms.items())) for r in lay.residues], ala_gly_class)
        out.append(structure.StructureRotamers(lay.residues, cls, chi))
    return out


def test_restatement_gives_the_fixture_and_the_figures_of_1ubq(golden, ubq):
    assert os.path.getsize(rr.GOLDEN) < 64 * 1024
    assert rr.coords_sha256(ubq) == str(golden["sha256"])
    cls, chi = rr.restate(ubq)
    assert same_bytes(cls, golden["cls"]) and same_bytes(chi, golden["chi"])
    assert len(cls) == 76 and (cls >= 0).all()
    assert int(np.isfinite(chi).sum()) == 157
    assert len(set(cls.tolist())) == 47
    assert cls[:20].tolist() == FIRST_TWENTY
    assert 0.0719 < rr.edge_distance(chi) < 0.0721               # no float64 implementation can flip a bin on this fixture
    assert rr.N_CLASSES == 338
    # the float64 restatement against long double: the yardstick the GPU's chi angles are measured with
    _, exact = rr.restate(ubq, dtype=np.longdouble)
    worst = float(np.nanmax(np.abs(exact - chi.astype(np.longdouble))))
    print("float64 restatement vs long double on 1ubq, worst chi error in degrees:", worst)
    assert 0.0 < worst < 1e-12                                    # a few dozen ulp of 180 degrees (one ulp: 2.8e-14)
    none, _ = rr.restate(ubq, ala_gly_class=False)
    ala_gly = np.array([res in ("ALA", "GLY") for res, _ in ubq])
    assert (none[ala_gly] == -1).all() and same_bytes(none[~ala_gly], cls[~ala_gly]) and ala_gly.sum() == 8


def test_rotamer_table_matches_the_python_tables(lib):
    from design_utils import utils
    from design_utils.amino_acids import side_chain_dihedrals, standard_amino_acids
    table = structure.rotamer_table()
    assert [row[0] for row in table] == list(standard_amino_acids.values()) == rr.RESIDUES
    assert [row[2] for row in table] == REDUCTION_GUIDE == utils.get_rotamer_codec(return_reduction_guide=True)[2]
    for res, n_chi, base, names in table:
        assert n_chi == len(side_chain_dihedrals.get(res, ())), res
        assert names == rr.path_of(res), res
        assert base == rr.CLASS_BASE[res]
        assert len(names) == (n_chi + 3 if n_chi else 0)
    assert lib.th_rotamer_table(20, None, None, None) == _lib.TH_EINVAL and b"th_rotamer_table" in lib.th_last_error()
    assert lib.th_rotamer_table(-1, None, None, None) == _lib.TH_EINVAL
    assert lib.th_rotamer_table(3, None, None, None) == _lib.TH_OK                 # every output is optional
    # class = base + digits of the bins in base 3, the first angle slowest: the codec's own names
    names = utils.get_rotamer_codec()[1]
    for res, n_chi, base, _ in table:
        for index in range(3 ** n_chi):
            digits = "".join(str(index // 3 ** (n_chi - 1 - k) % 3 + 1) for k in range(n_chi)) or "0"
            assert names[base + index] == f"{res}_{digits}"


def test_layout_of_1ubq_is_the_flat_form_of_its_residues(ubq):
    model = pdbio.read_pdb(rr.UBQ)[0]
    lay = structure.rotamer_layout(model)
    xyz, names, offsets, types = rr.flatten(ubq)
    assert same_bytes(lay.xyz, xyz) and same_bytes(lay.atom_name, names) and same_bytes(lay.res_offsets, offsets) and same_bytes(lay.res_type, types)
    assert len(lay.residues) == 76 and all(not r.hetero for r in lay.residues)
    assert structure.pack_atom_names(["CA", "N", "OD1", "HD11", ""]).tolist() == [0x4143, 0x4E, 0x31444F, 0x31314448, 0]
    assert len(structure.rotamer_layout(pdbio.Model(1, [])).residues) == 0


def test_layout_orders_chains_as_the_file_does_and_keeps_unknown_residues(tmp_path):
    def atom(serial, name, res, chain, number, x, het=False):
        return f"{'HETATM' if het else 'ATOM  '}{serial:5d} {name:<4s} {res:>3s} {chain}{number:>4s}    {x:8.3f}{0.0:8.3f}{0.0:8.3f}  1.00  0.00"
    lines = [atom(1, " N", "SER", "B", "5", 1.0), atom(2, " CA", "SER", "B", "5", 2.0), atom(3, " N", "MSE", "A", "1", 3.0),
             atom(4, " N", "GLY", "B", "6A", 4.0), atom(5, " O", "HOH", "A", "101", 5.0, het=True), atom(6, " N", "ALA", "A", "2", 6.0)]
    path = tmp_path / "two.pdb"
    path.write_text("\n".join(lines) + "\n")
    lay = structure.rotamer_layout(structure.first_model(path))
    assert [(r.chain, r.number, r.name) for r in lay.residues] == [("B", "5", "SER"), ("B", "6A", "GLY"), ("A", "1", "MSE"), ("A", "2", "ALA")]
    assert lay.res_type.tolist() == [15, 5, -1, 0] and lay.res_offsets.tolist() == [0, 2, 3, 4, 5]
    assert lay.xyz[:, 0].tolist() == [1.0, 2.0, 4.0, 3.0, 6.0]
    first = structure.rotamer_layout(structure.first_model(path), all_chains=False)
    assert [r.chain for r in first.residues] == ["B", "B"]
    (tagged,) = restated([lay])
    assert tagged.cls.tolist() == [-1, 49, -1, 0] and tagged.rotamers == [None, "0", None, "0"]       # SER without CB and OG
    labels, unmatched = structure.labels_for_map(tagged, [("two", "A", "2", "ALA"), ("two", "B", "6A", "GLY"), ("two", "B", "6", "GLY"),
                                                          ("two", "A", "1", "MET"), ("two", "B", "5", "SER"), ("two", "C", "5", "SER")])
    assert labels == [0, 49, None, None, None, None] and unmatched == 2


def test_rotamer_strings_of_1ubq(golden):
    (tagged,) = restated([rr.UBQ])
    assert same_bytes(tagged.cls, golden["cls"])
    from design_utils import utils
    names = utils.get_rotamer_codec()[1]
    assert [f"{r.name}_{rot}" for r, rot in zip(tagged.residues, tagged.rotamers)] == [names[c] for c in golden["cls"]]
    assert tagged.rotamers[0] == "122" and tagged.residues[0].name == "MET"


def _tree(tmp_path):
    """ub/1ubq.pdb1.gz, ab/1abc.pdb1 (plain), design_1.pdb — and no file for 2xyz or lost_2"""
    import gzip
    root = tmp_path / "pdb"
    (root / "ub").mkdir(parents=True)
    (root / "ab").mkdir()
    shutil.copy(rr.UBQ, root / "ub" / "1ubq.pdb1.gz")
    with gzip.open(rr.UBQ, "rb") as src:
        text = src.read()
    (root / "ab" / "1abc.pdb1").write_bytes(text)
    (root / "design_1.pdb").write_bytes(text)
    return root


def test_tag_pdb_with_rot_follows_the_reference_file_rule(tmp_path, monkeypatch, capsys, golden):
    from design_utils import analyse_utils as au
    root = _tree(tmp_path)
    before = sorted(str(p) for p in root.rglob("*"))
    assert au.rotamer_structure_path(root, "1ubqA")[0] == root / "ub" / "1ubq.pdb1.gz"
    assert au.rotamer_structure_path(root, "1abc")[0] == root / "ab" / "1abc.pdb1"
    assert au.rotamer_structure_path(root, "design_1")[0] == root / "design_1.pdb"
    assert au.rotamer_structure_path(root, "2xyz") == (None, root / "xy" / "2xyz.pdb1")
    assert au.rotamer_structure_path(root, "lost_2") == (None, root / "lost_2.pdb")
    calls = []

    def tag(layouts, **kw):
        calls.append(len(layouts))
        return restated(layouts, **kw)
    monkeypatch.setattr(structure, "tag_rotamers", tag)
    results, assemblies = au.tag_pdb_with_rot(40, root, np.array(["1ubqA", "2xyz", "1abc", "lost_2", "design_1"]))
    said = capsys.readouterr().out
    assert f"Could not find {root / 'xy' / '2xyz.pdb1'}" in said and f"Could not find {root / 'lost_2.pdb'}" in said
    assert calls == [3]                                           # all structures go to the GPU together
    assert sorted(str(p) for p in root.rglob("*")) == before      # nothing created, nothing fetched
    want = golden["cls"].tolist()
    assert results == {"1ubqA": want, "1abcA": want, "desiA": want}
    assert set(assemblies) == {"1ubq", "1abc", "desi"}
    chain = assemblies["1ubq"]["A"]
    assert chain.sequence.startswith("MQIFVKTLTGK") and len(chain.sequence) == len(chain) == 76 and chain.id == "A"
    assert au.extract_rotamer_encoding("1ubqA", chain) == {"1ubqA": want}
    untagged = au.RotamerChain("B", chain.residues[:2], np.array([-1, 5], np.int16))
    got = au.extract_rotamer_encoding("9xyz_more", untagged)["9xyzB"]
    assert np.isnan(got[0]) and got[1] == 5
    assert au.rotamer_labels_json({"k": [float("nan"), 3.0]}) == {"k": [None, 3]}


def test_tag_rotamers_parser():
    import tag_rotamers
    args = tag_rotamers.build_parser().parse_args(["--path_to_pdb", "a", "b"])
    assert vars(args) == {"path_to_pdb": ["a", "b"], "path_to_output": "rotamers", "device": 0, "workers": 8, "no_ala_gly_class": False}
    args = tag_rotamers.build_parser().parse_args(["--path_to_pdb", "a", "--path_to_output", "o", "--device", "1", "--workers", "2", "--no_ala_gly_class"])
    assert (args.path_to_output, args.device, args.workers, args.no_ala_gly_class) == ("o", 1, 2, True)
    with pytest.raises(SystemExit):
        tag_rotamers.build_parser().parse_args([])
    assert "PARITY UNPINNED AGAINST AMPAL" in tag_rotamers.build_parser().format_help()


def test_tag_rotamers_main_writes_both_files(tmp_path, monkeypatch, golden):
    import csv

    import tag_rotamers
    monkeypatch.setattr(structure, "tag_rotamers", restated)
    out = tmp_path / "out"
    tag_rotamers.main(tag_rotamers.build_parser().parse_args(["--path_to_pdb", rr.UBQ, "--path_to_output", str(out)]))
    assert json.loads((out / "rotamer_labels.json").read_text()) == {"1ubqA": golden["cls"].tolist()}
    with open(out / "chi_angles.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["structure", "chain", "residue", "name", "chi1", "chi2", "chi3", "chi4", "rotamer", "class"] and len(rows) == 77
    assert rows[1][:4] == ["1ubq.pdb1.gz", "A", "1", "MET"] and rows[1][7:] == ["", "122", "162"]
    chi = np.array([[float(x) if x else np.nan for x in r[4:8]] for r in rows[1:]])
    assert same_bytes(chi, golden["chi"])
    tag_rotamers.main(tag_rotamers.build_parser().parse_args(["--path_to_pdb", rr.UBQ, "--path_to_output", str(out), "--no_ala_gly_class"]))
    assert json.loads((out / "rotamer_labels.json").read_text())["1ubqA"].count(None) == 8


def test_analyse_rotamers_decides_between_labels_file_structures_and_neither(tmp_path, monkeypatch, golden):
    import analyse_rotamers
    root = _tree(tmp_path)
    rng = np.random.default_rng(8)
    np.savetxt(tmp_path / "M_rot.csv", rng.dirichlet(np.ones(338), 76).astype(np.float16), delimiter=",")
    (tmp_path / "map.txt").write_text("ignore_uncommon False\ninclude_pdbs\n##########\n1ubqA 76\n")
    seen = []

    def metrics(pdb_to_probability, pdb_to_rotamer, rot_categories, suffix, output_path, device=0):
        seen.append((dict(pdb_to_rotamer), suffix, str(output_path), len(pdb_to_probability["1ubqA"])))
        return {}
    monkeypatch.setattr(analyse_rotamers, "calculate_rotamer_metrics", metrics)
    monkeypatch.setattr(structure, "tag_rotamers", restated)
    common = ["--path_to_pred_matrix", str(tmp_path / "M_rot.csv"), "--path_to_datasetmap", str(tmp_path / "map.txt")]
    # structures, no labels file: tagged here, the labels file is written into the output directory
    analyse_rotamers.main(analyse_rotamers.build_parser().parse_args(common + ["--output_path", str(tmp_path / "a"), "--path_to_pdb", str(root)]))
    written = tmp_path / "a_M_rot" / "rotamer_labels.json"
    want = {"1ubqA": golden["cls"].tolist()}
    assert json.loads(written.read_text()) == want
    assert seen[-1] == (want, "M_rot_vs_original", str(tmp_path / "a_M_rot"), 76)
    # a labels file wins: --path_to_pdb is not read
    analyse_rotamers.main(analyse_rotamers.build_parser().parse_args(
        common + ["--output_path", str(tmp_path / "b"), "--path_to_pdb", str(tmp_path / "nowhere"), "--path_to_rotamer_labels", str(written)]))
    assert seen[-1] == (want, "M_rot_vs_original", str(tmp_path / "b_M_rot"), 76)
    assert not (tmp_path / "b_M_rot" / "rotamer_labels.json").exists()
    # neither: today's message
    with pytest.raises(SystemExit) as stop:
        analyse_rotamers.main(analyse_rotamers.build_parser().parse_args(common + ["--output_path", str(tmp_path / "c")]))
    for word in ("--path_to_rotamer_labels", "tag_pdb_with_rot", "ampal", "SCWRL4", "--path_to_pdb"):
        assert word in str(stop.value), word
    assert not (tmp_path / "c_M_rot").exists() and len(seen) == 2
    with pytest.raises(AssertionError, match="PDB folder"):
        analyse_rotamers.main(analyse_rotamers.build_parser().parse_args(common + ["--output_path", str(tmp_path / "d"), "--path_to_pdb", str(tmp_path / "nowhere")]))
    text = analyse_rotamers.build_parser().format_help()
    for word in ("PARITY", "rotamer_labels.json", "tag_rotamers.py"):
        assert word in text, word


_CTYPES = {"int": "c_int", "int64_t": "c_long", "const double*": "c_void_p", "const uint32_t*": "c_void_p", "const int64_t*": "c_void_p",
           "const int8_t*": "c_void_p", "int16_t*": "c_void_p", "double*": ("c_void_p", "LP_c_double"), "int*": "LP_c_int", "char": "c_void_p"}


def test_header_ctypes_and_build_list_declare_the_new_functions():
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    for name in ("th_tag_rotamers", "th_rotamer_table"):
        m = re.search(r"^(\w+) " + name + r"\(([^;]*)\);", header, re.M)
        assert m, name
        res, args = _lib.PROTOTYPES[name]
        assert res.__name__ == _CTYPES[m.group(1)]
        declared = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(2).split(",")]
        assert len(declared) == len(args), (declared, args)
        for c_type, ct in zip(declared, args):
            want = _CTYPES[c_type]
            assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (name, c_type, ct)
    assert "PARITY UNPINNED AGAINST AMPAL" in header
    assert structure.__doc__.count("PARITY UNPINNED AGAINST AMPAL") == 2
    import __graft_entry__
    assert "rotamers.hip" in __graft_entry__.HIP_SOURCES
