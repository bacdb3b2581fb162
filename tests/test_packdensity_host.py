"""Packing density without a GPU: the NumPy restatement (tests/packdensity_restatement.py) against the reference's own output
(tests/golden/packdensity_golden.npz) byte for byte; th_packing_threshold against np.sqrt over the neighbourhoods of r^2; the
structure rule's layout of 1ubq; B-factor parsing; the atom filters; batching; the command line; header and ctypes prototype."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packdensity_restatement as pr  # noqa: E402
from timed_hip import _lib, pdbio, structure  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
UBQ = os.path.join(G, "1ubq.pdb1.gz")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "packdensity_golden.npz"))


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_fixture_is_small_and_the_structures_rebuild_from_their_seeds(golden):
    assert os.path.getsize(os.path.join(G, "packdensity_golden.npz")) < 256 * 1024
    for name, (_seed, n_heavy, _chains, _planted) in pr.GOLDEN_CASES.items():
        chains = pr.golden_structure(name)
        assert pr.coords_sha256(chains) == str(golden[f"{name}_sha256"]), name
        assert len(pr.flatten(chains, "all")[0]) == n_heavy == len(golden[f"{name}_density_r7.0"])


@pytest.mark.parametrize("name", list(pr.GOLDEN_CASES))
def test_restatement_equals_the_reference_output(golden, name):
    chains = pr.golden_structure(name)
    for radius in pr.RADII:
        xyz, group, selected, n_groups = pr.flatten(chains, "all")
        density = pr.restate_density(xyz, [0, len(xyz)], radius)
        assert same_bytes(density, golden[f"{name}_density_r{radius}"]), (name, radius)
        for atom_filter in pr.FILTERS:
            _, group, selected, n_groups = pr.flatten(chains, atom_filter)
            res = pr.restate_residues(density, group, selected, n_groups)
            assert same_bytes(res, golden[f"{name}_res_{atom_filter}_r{radius}"]), (name, radius, atom_filter)


def test_planted_cases_hold_what_they_claim(golden):
    chains = pr.golden_structure("mix")
    xyz = pr.flatten(chains, "all")[0]
    assert np.isnan(xyz).any(axis=1).sum() == 1 and np.isinf(xyz).any(axis=1).sum() == 1
    bad = ~np.isfinite(xyz).all(axis=1)
    d7 = golden["mix_density_r7.0"]
    assert (d7[bad] == -1).all() and (d7[~bad] >= 0).all()
    finite = xyz[~bad]
    assert len(np.unique(finite, axis=0)) <= len(finite) - 5                # duplicated coordinates
    # pairs at nominal distance exactly r exist for every radius, and float64 puts some on each side of at least one radius
    sides = set()
    for radius in pr.RADII:
        n_ties = 0
        for off in pr.TIE_OFFSETS[radius]:
            want = np.round(finite + np.array(off, dtype=np.float64), 3)
            hit = (want[:, None, :] == finite[None, :, :]).all(axis=2)
            for a, b in zip(*np.nonzero(hit)):
                q = np.square(finite[b] - finite[a])
                sides.add(bool(np.sqrt((q[0] + q[1]) + q[2]) < radius))
                n_ties += 1
        assert n_ties >= len(pr.TIE_OFFSETS[radius]), radius
    assert sides == {True, False}
    # the residue whose leading selected atom has density -1 takes the reference's branch: the next atom replaces it
    _, group, selected, n_groups = pr.flatten(chains, "ca")
    lead = [int(np.flatnonzero((group == g) & (selected == 1))[0]) for g in range(n_groups) if ((group == g) & (selected == 1)).any()]
    assert any(d7[i] == -1 for i in lead)
    # residues without a selected atom exist under every filter
    for atom_filter in pr.FILTERS:
        assert (golden[f"mix_res_{atom_filter}_r7.0"] == -1.0).any(), atom_filter
    assert (golden["mix_res_ca_r7.0"] % 1 != 0).any()                        # halves: the running half-average, not a count


def test_1ubq_layout_follows_the_structure_rule(golden):
    model = pdbio.read_pdb(UBQ)[0]
    lay = structure.layout(model, "all")
    assert same_bytes(lay.xyz, golden["ubq_xyz"]) and len(lay.xyz) == 660
    assert len(lay.residues) == 76 and all(not r.hetero and r.chain == lay.residues[0].chain for r in lay.residues)
    assert (lay.group == -1).sum() == sum(len(r.atoms) for r in model.residues if r.hetero)      # waters are neighbours only
    for radius in pr.RADII:
        density = pr.restate_density(lay.xyz, [0, len(lay.xyz)], radius)
        assert same_bytes(density, golden[f"ubq_density_r{radius}"])
        for atom_filter in pr.FILTERS:
            lay_f = structure.layout(model, atom_filter)
            res = pr.restate_residues(density, lay_f.group, lay_f.selected, len(lay_f.residues))
            assert same_bytes(res, golden[f"ubq_res_{atom_filter}_r{radius}"]), (radius, atom_filter)
    no_het = structure.layout(model, "all", include_hetero=False)
    assert len(no_het.xyz) == 660 - (lay.group == -1).sum() and (no_het.group >= 0).all()


def _radii():
    rng = np.random.default_rng(5)
    grid = [round(0.5 + 0.1 * k, 1) for k in range(115)]
    return grid + list(rng.uniform(0.01, 40.0, 300)) + list(10.0 ** rng.uniform(-170, 170, 100)) + [
        1e-320, 5e-324, 1e-162, 1.5e-154, 1e154, 1.3407807929942596e154, 1e200, 1.7976931348623157e308, 1e9]


def test_threshold_is_exact_for_every_double_near_r_squared(lib):
    differs = 0
    for r in _radii():
        r = np.float64(r)
        t = np.float64(structure.packing_threshold(r))
        with np.errstate(over="ignore", under="ignore"):
            sq = r * r
        probes = set()
        for centre in (t, sq):
            lo = hi = centre
            probes.add(float(centre))
            for _ in range(6):
                lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
                probes.update((float(lo), float(hi)))
        probes.update((0.0, np.inf, float(np.finfo(np.float64).max), 5e-324))
        for s in probes:
            if s < 0:
                continue
            s = np.float64(s)
            assert bool(np.sqrt(s) < r) == bool(s < t), (float(r), float(s), float(t))
        assert not (np.float64(np.nan) < t)
        differs += int(t != sq)
    assert differs > 50                                   # T is not r * r in general
    assert structure.packing_threshold(7.0) == 49.0
    for r in (1.1, 2.2):                                  # sqrt(nextafter(r * r, 0)) rounds back up to r
        assert structure.packing_threshold(r) < r * r


def test_threshold_of_degenerate_radii(lib):
    assert structure.packing_threshold(0.0) == 0.0 and structure.packing_threshold(-0.0) == 0.0
    assert structure.packing_threshold(-3.0) == 0.0 and structure.packing_threshold(-np.inf) == 0.0
    assert structure.packing_threshold(np.inf) == np.inf and np.isnan(structure.packing_threshold(np.nan))


def test_bfactor_parsing(tmp_path):
    atom = "ATOM      1  N   MET A   1      27.340  24.430   2.614  1.00  9.67           N"
    lines = [atom,
             atom[:54].replace("  N   MET", "  CA  MET").replace("    1  ", "    2  "),                     # no occupancy, no B-factor
             (atom[:60] + "  abc ").replace("  N   MET", "  C   MET"),                                     # unparsable
             atom[:66].replace("  N   MET", "  O   MET").replace("  9.67", "-12.50"),                      # ends after the column
             "HETATM    5  O   HOH A 101      1.000   2.000   3.000  1.00 33.10           O",
             "ATOM      6  N   GLY B   2      1.000   2.000   3.000  1.00 50.00           N",
             "ATOM      7  CA  GLY B   2      1.000   2.000   4.000  1.00 60.00           C"]
    path = tmp_path / "b.pdb"
    path.write_text("\n".join(lines) + "\n")
    model = pdbio.read_pdb(path)[0]
    met = model.residues[0]
    assert met.bfactors["N"] == 9.67 and np.isnan(met.bfactors["CA"]) and np.isnan(met.bfactors["C"]) and met.bfactors["O"] == -12.5
    assert list(met.bfactors) == list(met.atoms) == ["N", "CA", "C", "O"]
    assert model.residues[1].hetero and model.residues[1].bfactors == {"O": 33.1}
    assert structure.residue_bfactors(model) == [[9.67], [50.0]]
    from design_utils import analyse_utils as au
    assert au.extract_bfactor_from_ampal(path) == [[9.67], [50.0]]
    assert au.extract_bfactor_from_ampal(model, load_pdb=False) == [[9.67], [50.0]]
    ubq = au.extract_bfactor_from_ampal(UBQ)
    assert len(ubq) == 1 and len(ubq[0]) == 76 and ubq[0][0] == 9.67
    # nothing that existed changes: coordinates, elements and flags of 1ubq as before
    r0 = pdbio.read_pdb(UBQ)[0].residues[0]
    assert (r0.chain, r0.number, r0.name, r0.hetero) == ("A", "1", "MET", False) and r0.elements["CA"] == "C"
    assert r0.atoms["N"].tolist() == [27.34, 24.43, 2.614]


def test_atom_filters_and_the_ca_quirk():
    names = ["N", "CA", "C", "O", "CB", "OXT", "A", ""]
    assert [n for n in names if structure.atom_selected(n, "ca")] == ["CA", "C", "A", ""]
    assert [n for n in names if structure.atom_selected(n, "calpha")] == ["CA"]
    assert [n for n in names if structure.atom_selected(n, "backbone")] == ["N", "CA", "C", "O"]
    assert all(structure.atom_selected(n, "all") for n in names)
    for atom_filter in structure.ATOM_FILTERS:
        assert all(structure.atom_selected(n, atom_filter) == pr.selects(n, atom_filter) for n in names)
    with pytest.raises(ValueError, match="Atom Filter"):
        structure.atom_selected("CA", "sidechain")
    assert structure.is_hydrogen("H", "H") and structure.is_hydrogen("HB2", "h") and structure.is_hydrogen("1HB", "1")
    assert not structure.is_hydrogen("CA", "C") and not structure.is_hydrogen("HG", "HG") and not structure.is_hydrogen("OH", "O")
    model = pdbio.read_pdb(UBQ)[0]
    ca, calpha = structure.layout(model, "ca"), structure.layout(model, "calpha")
    assert ca.selected.sum() == 2 * 76 and calpha.selected.sum() == 76
    everything = structure.layout(model, "all", all_chains=True)
    assert len(everything.residues) == 76                                     # one protein chain


def test_layout_of_synthetic_pdb_files_matches_the_fixture_rule(tmp_path):
    chains = pr.build_structure(17, 900, 3, planted=True, finite_only=True)
    path = tmp_path / "mix.pdb"
    pr.write_pdb(chains, path)
    model = pdbio.read_pdb(path)[0]
    for atom_filter in pr.FILTERS:
        lay = structure.layout(model, atom_filter)
        xyz, group, selected, n_groups = pr.flatten(chains, atom_filter)
        assert same_bytes(lay.xyz, xyz) and same_bytes(lay.selected, selected) and len(lay.residues) == n_groups
        # a reported residue of hydrogens only has no atom in the layout: the group numbering still counts it
        assert same_bytes(lay.group, group)
    every = structure.layout(model, "all", all_chains=True)
    assert len(every.residues) == len(chains[0]) + len(chains[1])              # the third chain is hetero
    assert structure.residue_bfactors(model) == [[pr.bfactor_of(r) for r in chains[0]], [pr.bfactor_of(r) for r in chains[1]]]


def test_batches_are_cut_by_bytes_not_per_structure():
    per = structure._ATOM_BYTES
    assert structure.cut_batches([], 100) == []
    assert structure.cut_batches([10, 10, 10], 1 << 20) == [(0, 3)]
    assert structure.cut_batches([10, 10, 10], 20 * per) == [(0, 2), (2, 3)]
    assert structure.cut_batches([50, 1, 1, 50, 0], 10 * per) == [(0, 1), (1, 3), (3, 4), (4, 5)]      # one above the budget goes alone
    assert structure.cut_batches([0, 0, 0], 1) == [(0, 3)]


def test_analyse_properties_argument_surface(tmp_path):
    import analyse_properties as ap
    args = ap.build_parser().parse_args(["--path_to_pdb", "a", "b"])
    assert vars(args) == {"path_to_pdb": ["a", "b"], "atom_filter_function": "all", "radius": 7.0, "path_to_output": "properties",
                          "workers": 8, "device": 0, "all_chains": False, "batch_mb": 256.0, "path_to_pred_matrix": None,
                          "path_to_datasetmap": None, "rotamer_mode": False, "support_old_datasetmap": False}
    for choice in ("all", "ca", "backbone", "calpha"):
        assert ap.build_parser().parse_args(["--path_to_pdb", "a", "--atom_filter_function", choice]).atom_filter_function == choice
    with pytest.raises(SystemExit):
        ap.build_parser().parse_args(["--path_to_pdb", "a", "--atom_filter_function", "sidechain"])
    with pytest.raises(SystemExit):
        ap.build_parser().parse_args([])
    text = ap.build_parser().format_help()
    for word in ("CE-align", "Out of scope", "structure rule"):
        assert word in text, word
    (tmp_path / "d" / "sub").mkdir(parents=True)
    for name in ("d/x.pdb", "d/sub/y.pdb1.gz", "d/sub/z.ent", "d/notes.txt", "d/w.PDB.GZ", "one.ent.gz"):
        (tmp_path / name).write_text("")
    found = ap.find_structures([tmp_path / "d", tmp_path / "one.ent.gz"])
    assert [label for label, _ in found] == ["sub/y.pdb1.gz", "sub/z.ent", "w.PDB.GZ", "x.pdb", "one.ent.gz"]
    assert [ap.stem_of(label) for label, _ in found] == ["y", "z", "w", "x", "one"]
    with pytest.raises(FileNotFoundError):
        ap.find_structures([tmp_path / "missing"])


_CTYPES = {"int": "c_int", "double": "c_double", "int64_t": "c_long", "const double*": "c_void_p", "const int64_t*": "c_void_p",
           "const int32_t*": "c_void_p", "const uint8_t*": "c_void_p", "int32_t*": "c_void_p", "double*": ("c_void_p", "LP_c_double")}


def test_header_and_ctypes_declare_the_same_prototypes():
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    for name in ("th_packing_density", "th_packing_threshold"):
        m = re.search(r"^(\w+) " + name + r"\(([^;]*)\);", header, re.M)
        assert m, name
        res, args = _lib.PROTOTYPES[name]
        assert res.__name__ == _CTYPES[m.group(1)]
        declared = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(2).split(",")]
        assert len(declared) == len(args), (declared, args)
        for c_type, ct in zip(declared, args):
            want = _CTYPES[c_type]
            assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (name, c_type, ct)
    import __graft_entry__
    assert "packdensity.hip" in __graft_entry__.HIP_SOURCES
