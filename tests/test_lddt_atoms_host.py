"""All-atom lDDT without a GPU: the NumPy restatement (tests/lddt_atoms_restatement.py) against the committed fixture and the figures
of the write-up; ``atom_lists`` against hand-built residues; the header prototype, the ctypes entry, the build list and the
unpinned-parity phrase; every TH_EINVAL of th_lddt_atoms; the three command lines with the kernel calls replaced by restatements."""
import csv
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lddt_atoms_restatement as ar  # noqa: E402
import superpose_restatement as sr  # noqa: E402
from timed_hip import _lib, lddt_atoms, pdbio, sidechains, superpose  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHRASE = ar.PHRASE


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def golden():
    return np.load(ar.GOLDEN)


def restated_arrays(ref_xyz, mob_xyz, residue, partner, offsets, radius=15.0, thresholds=ar.THRESHOLDS, symmetry=True, device=0, timing=None):
    """lddt_atoms.lddt_atoms_arrays with the GPU call replaced by the restatement"""
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0)
    return lddt_atoms.LddtAtomTables(*ar.restate_batch(ref_xyz, mob_xyz, np.asarray(residue), np.asarray(partner), offsets, radius, thresholds, symmetry))


def restated_superposition(ref_xyz, mob_xyz, offsets, cycles=5, cutoff=2.0, device=0, transform=False, timing=None):
    """superpose.superpose_arrays with the GPU call replaced by its restatement"""
    dist, kept, rmsd, counts, moves, _, _ = sr.restate_batch(ref_xyz, mob_xyz, np.asarray(offsets), cycles, cutoff)
    return superpose.Superposed(dist, kept, rmsd, counts, moves.reshape(-1, 3, 4) if transform else None)


def test_restatement_equals_the_fixture_and_the_written_figures(golden):
    assert os.path.getsize(ar.GOLDEN) < 512 * 1024
    cases = ar.build_cases()
    assert str(golden["sha256"]) == ar.inputs_sha256(cases) and golden["cases"].tolist() == list(cases)
    again = ar.golden_arrays(cases)
    assert sorted(golden.files) == sorted(again)
    for key in golden.files:
        assert same_bytes(golden[key], np.asarray(again[key])), key
    text = open(os.path.join(ROOT, "tests", "golden", "make_lddt_atoms_golden.py")).read()
    assert "NOT by the kernel" in text and PHRASE in text
    pair = {name: golden[f"{name}_pair"].tolist() for name in cases}
    named = {name: golden[f"{name}_named_pair"].tolist() for name in cases}
    for name in cases:
        print(name, "n_ref, n_missing, N, C, swapped", pair[name], "lddt", ar.score(golden[f"{name}_pair"]), "as named", ar.score(golden[f"{name}_named_pair"]))
    # case 1: 1ubq against itself: 601 heavy atoms without OXT in 76 residues, 31 symmetric residues, 68 swappable atoms
    partner, residue = golden["self_partner"], golden["self_residue"]
    assert len(partner) == 601 and residue[-1] == 75 and (partner >= 0).sum() == 68 and len(np.unique(residue[partner >= 0])) == 31
    assert pair["self"] == [601, 0, 171464, 171464, 171464, 171464, 171464, 0] and not golden["self_swapped"].any()
    assert same_bytes(golden["self_atom"][:, 1:], np.repeat(golden["self_atom"][:, :1], 4, axis=1))               # every c equals n
    # case 2: every symmetric name pair exchanged: resolved, the bytes of case 1; as named, it is charged
    assert same_bytes(golden["flipped_atom"], golden["self_atom"]) and pair["flipped"] == pair["self"][:7] + [31]
    assert same_bytes(golden["flipped_swapped"], (partner >= 0).astype(np.uint8))
    assert named["flipped"] == [601, 0, 171464, 142358, 150584, 165278, 171418, 0] and named["flipped"][3] < named["flipped"][2]
    assert round(ar.score(golden["flipped_named_pair"]), 3) == 0.918 and ar.score(golden["flipped_pair"]) == 1.0
    assert not golden["flipped_named_swapped"].any()
    # case 3: noise, and the same noise with names exchanged
    assert same_bytes(golden["noise_flipped_atom"], golden["noise_atom"]) and pair["noise"][7] == 0 and pair["noise_flipped"][7] == 31
    assert 0.93 < ar.score(golden["noise_pair"]) < 0.945 and ar.score(golden["noise_flipped_named_pair"]) < ar.score(golden["noise_pair"]) - 0.05
    assert same_bytes(golden["noise_named_atom"], golden["noise_atom"])                                         # nothing to resolve
    # case 4: missing atoms are counted, included and never preserved; an infinity behaves the same way
    for name in ("missing", "missing_symmetric"):
        gone = np.isnan(golden[f"{name}_mob"]).any(axis=1)
        rows = golden[f"{name}_atom"]
        assert pair[name][1] == gone.sum() > 30 and pair[name][0] == 601 and pair[name][2] == 171464
        assert same_bytes(rows[:, 0], golden["self_atom"][:, 0]) and not rows[gone, 1:].any() and rows[gone, 0].min() > 0
        assert pair[name][3] == pair[name][6] < pair[name][2]                                                    # what is there is exact
    assert np.isinf(golden["missing_infinite_mob"]).sum() == 37 and not np.isnan(golden["missing_infinite_mob"]).any()
    for table in ar.TABLES:
        assert same_bytes(golden[f"missing_infinite_{table}"], golden[f"missing_{table}"])
    tied = ar.restate(*(golden[f"missing_symmetric_{key}"] for key in ar.INPUTS))
    assert sorted(r for r in tied["keep"] if tied["keep"][r] == tied["swap"][r]) == [3, 17, 44, 53, 70] and tied["margin"] == 0
    # case 5: a non-finite reference coordinate excludes the atom on both sides
    bad = ~np.isfinite(golden["reference_invalid_ref"]).all(axis=1)
    assert bad.sum() == 6 and pair["reference_invalid"][0] == 595 and not golden["reference_invalid_atom"][bad].any()
    dropped = ar.restate(np.delete(golden["noise_ref"], np.flatnonzero(bad), axis=0), np.delete(golden["noise_mob"], np.flatnonzero(bad), axis=0),
                         np.delete(residue, np.flatnonzero(bad)), np.full(601 - 6, -1), symmetry=False)
    assert same_bytes(np.delete(golden["reference_invalid_named_atom"], np.flatnonzero(bad), axis=0), dropped["atom"])
    # case 6: five residues renamed: only their backbone enters
    assert int(golden["renamed_n_mismatched"]) == 5 and len(golden["renamed_ref"]) == 573 and golden["renamed_residue"][-1] == 75
    counts = np.bincount(golden["renamed_residue"])
    assert (counts[list(ar.FIVE_RESIDUES)] == 4).all() and golden["renamed_backbone"].sum() == 4 * 76
    # case 7: the tables written out by hand
    for name, (case, rows, swapped, totals) in ar.hand_cases().items():
        for tag in ("", "_named"):
            assert golden[f"{name}{tag}_atom"].tolist() == rows and golden[f"{name}{tag}_swapped"].tolist() == swapped, name
            assert golden[f"{name}{tag}_pair"].tolist() == totals, name
    assert np.isnan(ar.score(golden["hand_single_residue_pair"])) and np.isnan(ar.score(golden["chain_1_pair"]))
    inside = ar.restate(*(golden[f"hand_at_the_radius_{key}"] for key in ar.INPUTS), radius=np.nextafter(15.0, 16.0))
    assert inside["pair"].tolist() == [2, 0, 2, 2, 2, 2, 2, 0]                                                  # the next radius includes it
    wider = ar.restate(*(golden[f"hand_at_a_threshold_{key}"] for key in ar.INPUTS), thresholds=[np.nextafter(0.5, 1.0), 1.0, 2.0, 4.0])
    assert wider["pair"].tolist() == [2, 0, 2, 2, 2, 2, 2, 0]
    # case 8: tile edges
    assert golden["chain_257_partner"][255:].tolist() == [256, 255] and golden["chain_257_swapped"][255:].tolist() == [1, 1]
    assert (golden["chain_300_residue"][254:259] == 127).all() and golden["chain_300_residue"][253] == 126 and golden["chain_300_residue"][259] == 128
    assert [len(golden[f"chain_{n}_ref"]) for n in (257, 300, 256, 1)] == [257, 300, 256, 1]
    assert pair["chain_257"][7] == 2 and pair["chain_300"][7] == 3 and pair["chain_256"][7] == 1
    # every non-tie case keeps the margins the maker asks
    for name, case in cases.items():
        if name in ar.TIES:
            continue
        res = ar.restate(*(case[key] for key in ar.INPUTS))
        assert res["edge"] > ar.EDGE and (res["margin"] > 0 or name in ar.MARGIN_TIES), (name, res["edge"], res["margin"])


def _residue(name, atoms, chain="A", number="1", hetero=False, elements=None):
    res = pdbio.Residue(chain, number, name, hetero=hetero)
    for k, atom in enumerate(atoms):
        res.atoms[atom] = np.array([float(k), 0.5 * len(atom), 0.25])
        res.elements[atom] = (elements or {}).get(atom, atom[:1])
    return res


def test_atom_lists_ordering_dropped_atoms_mismatch_and_partners(golden):
    from design_utils.amino_acids import SYMMETRIC_ATOMS
    assert SYMMETRIC_ATOMS == ar.SYMMETRIC
    text = open(os.path.join(ROOT, "timed-design_amd", "design_utils", "amino_acids.py")).read()
    assert "WRITTEN FROM MEMORY, NOT FETCHED" in text[text.index("All-atom lDDT"):text.index("SYMMETRIC_ATOMS = ")]
    phe = ["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ"]
    reference = [_residue("PHE", ["N", "H", "CA", "HA", "C", "O", "OXT"] + phe[4:] + ["1HB", "D1"], number="1", elements={"1HB": "", "D1": "D"}),
                 _residue("ASP", ["N", "CA", "C", "O", "CB", "CG", "OD1"], number="2"),               # OD2 absent: no partner
                 _residue("LEU", ["CD2", "CD1", "CG", "CB", "N", "CA", "C", "O"], number="3"),        # file order is kept
                 _residue("HOH", ["O"], number="4", hetero=True),
                 _residue("VAL", ["N", "CA", "C", "O", "CB", "CG1", "CG2"], number="5"),
                 _residue("GLY", ["H1", "H2"], number="6")]                                           # hydrogens only: no atom, no index
    model = [_residue("PHE", phe[:7] + phe[8:], number="1"),                                          # CD2 missing
             _residue("ASP", ["N", "CA", "C", "O", "CB", "CG", "OD1", "OD2"], number="2"),
             _residue("LEU", ["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2"], number="3"),
             _residue("HOH", ["O"], number="4", hetero=True),
             _residue("ILE", ["N", "CA", "C", "O", "CB", "CG1", "CG2", "CD1"], number="5"),           # renamed: backbone only
             _residue("GLY", ["N", "CA", "C", "O"], number="6")]
    got = lddt_atoms.atom_lists(reference, model)
    assert got.names == phe[:4] + phe[4:] + ["N", "CA", "C", "O", "CB", "CG", "OD1", "CD2", "CD1", "CG", "CB", "N", "CA", "C", "O", "N", "CA", "C", "O"]
    assert got.residue.tolist() == [0] * 11 + [1] * 7 + [2] * 8 + [3] * 4 and got.residue_at.tolist() == [0, 1, 2, 4] and got.n_mismatched_residues == 1
    assert got.partner.tolist() == [-1] * 6 + [7, 6, 9, 8, -1] + [-1] * 7 + [19, 18] + [-1] * 6 + [-1] * 4
    assert got.backbone.tolist() == [True] * 4 + [False] * 7 + [True] * 4 + [False] * 3 + [False] * 4 + [True] * 4 + [True] * 4
    assert np.isnan(got.mob_xyz[7]).all() and np.isfinite(np.delete(got.mob_xyz, 7, axis=0)).all() and np.isfinite(got.ref_xyz).all()
    assert same_bytes(got.ref_xyz[18], reference[2].atoms["CD2"]) and same_bytes(got.mob_xyz[18], model[2].atoms["CD2"])
    assert got.residue.dtype == np.int32 and got.partner.dtype == np.int32
    with pytest.raises(ValueError):
        lddt_atoms.atom_lists(reference, model[:3])
    empty = lddt_atoms.atom_lists([], [])
    assert empty.ref_xyz.shape == (0, 3) and empty.residue.shape == (0,)
    # on 1ubq it gives the arrays of the restatement's own reading of the rules
    native = ar.ubq()
    mine = lddt_atoms.atom_lists([r for r in native.residues if not r.hetero], [r for r in native.residues if not r.hetero])
    assert same_bytes(mine.ref_xyz, golden["self_ref"]) and same_bytes(mine.residue, golden["self_residue"])
    assert same_bytes(mine.partner, golden["self_partner"]) and same_bytes(mine.backbone, golden["self_backbone"]) and "OXT" not in mine.names


_CTYPES = {"int": "c_int", "int64_t": "c_long", "double": "c_double", "unsigned": "c_uint", "const double*": "c_void_p", "const int64_t*": "c_void_p",
           "const int32_t*": "c_void_p", "int32_t*": "c_void_p", "uint8_t*": "c_void_p", "int64_t*": "c_void_p", "double*": ("c_void_p", "LP_c_double")}


def test_header_ctypes_build_list_documents_and_the_unpinned_parity_phrase():
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    m = re.search(r"^(\w+) th_lddt_atoms\(([^;]*)\);", header, re.M)
    assert m
    res, args = _lib.PROTOTYPES["th_lddt_atoms"]
    assert res.__name__ == _CTYPES[m.group(1)]
    declared = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(2).split(",")]
    assert len(declared) == len(args) == 15, (declared, args)
    for c_type, ct in zip(declared, args):
        want = _CTYPES[c_type]
        assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (c_type, ct)
    before = header[:m.start()]
    block = before[before.rindex("/* ----"):]
    assert block.startswith("/* ---- ") and "*** " + PHRASE + " ***" in block and "#define TH_LDDT_NO_SYMMETRY 1u" in block
    flat = re.sub(r"[\s*]+", " ", block)
    for words in ("Mariani et al. 2013", "fp contract(off)", "REFERENCE-VALID", "a missing atom costs score", "residue[i] != residue[j]",
                  "th_packing_threshold", "R is swapped iff swap_R > keep_R; a tie keeps the names", "look only at atoms without a partner",
                  "partner[partner[i]] == i", "unknown flag bits", "No atomics", "stereochemistry checks, sequence-separation filters, ligands"):
        assert words in flat, words
    assert lddt_atoms.TH_LDDT_NO_SYMMETRY == 1 and lddt_atoms._ATOM_BYTES == 77
    import __graft_entry__
    assert "lddt_atoms.hip" in __graft_entry__.HIP_SOURCES
    source = open(os.path.join(ROOT, "timed-design_amd", "csrc", "lddt_atoms.hip")).read()
    assert PHRASE in source and "th_packing_threshold(radius)" in source and "nextafter" not in source and "fp contract(off)" in source
    assert "atomic" not in source.replace("no atomics", "") and all(w in source for w in ("ThLayout", "ThCall", "th_check_offsets", "th_tile_items"))
    for kernel in ("k_lddt_resolve", "k_lddt_decide", "k_lddt_atoms", "k_lddt_atoms_totals"):
        assert re.search(r"__global__ void __launch_bounds__\(kTile\) %s\(" % kernel, source), kernel
    assert PHRASE in lddt_atoms.__doc__ and "WRITTEN FROM MEMORY, NOT FETCHED" in lddt_atoms.__doc__
    import analyse_models
    import build_sidechains
    import pack_sidechains
    text = re.sub(r"\s+", " ", analyse_models.build_parser().format_help())
    assert "--lddt_all_atom" in text and "--lddt_no_symmetry" in text and "model_lddt_all_atom.csv" in text and "residue_lddt_all_atom.csv" in text
    for module in (build_sidechains, pack_sidechains):
        text = re.sub(r"\s+", " ", module.build_parser().format_help())
        assert "--lddt" in text and "structure_sidechain_lddt.csv" in text and PHRASE in text
    readme = re.sub(r"\s+", " ", open(os.path.join(ROOT, "README.md")).read())
    design = re.sub(r"\s+", " ", open(os.path.join(ROOT, "DESIGN.md")).read())
    for document in (readme, design):
        assert "th_lddt_atoms" in document and "profiles/lddt_atoms.txt" in document and PHRASE in document
    assert os.path.exists(os.path.join(ROOT, "profiles", "lddt_atoms.txt")) and os.path.exists(os.path.join(ROOT, "tools", "bench_lddt_atoms.py"))
    from design_utils import analyse_utils
    assert PHRASE in analyse_utils.calculate_all_atom_lddt.__doc__


def test_library_exports_th_lddt_atoms_and_checks_arguments_without_a_gpu(lib):
    ref = np.arange(18, dtype=np.float64).reshape(6, 3)
    residue, partner = np.array([0, 0, 0, 1, 1, 1], np.int32), np.array([1, 0, -1, -1, 5, 4], np.int32)
    offsets, limits = np.array([0, 6], np.int64), np.array(ar.THRESHOLDS)
    atom, swapped, pair = np.full((6, 5), 77, np.int32), np.full(6, 77, np.uint8), np.full((1, 8), 77, np.int64)
    inf, nan = float("inf"), float("nan")

    def call(r=ref, m=ref, res=residue, par=partner, total=6, off=offsets, n_pairs=1, radius=15.0, lim=limits, flags=0, a=atom, s=swapped, p=pair):
        ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731
        ms = (C.c_double * 2)(-1.0, -1.0)
        rc = lib.th_lddt_atoms(0, ptr(r), ptr(m), ptr(res), ptr(par), total, ptr(off), n_pairs, radius, ptr(lim), flags, ptr(a), ptr(s), ptr(p),
                               C.cast(ms, C.POINTER(C.c_double)))
        assert rc == _lib.TH_OK or list(ms) == [-1.0, -1.0]
        return rc

    def changed(array, index, value):
        out = array.copy()
        out[index] = value
        return out
    two = np.array([0, 3, 6], np.int64)
    bad = {"negative total": dict(total=-1), "negative pairs": dict(n_pairs=-1), "total too large": dict(total=1 << 31),
           "pairs too large": dict(n_pairs=1 << 31), "offsets NULL": dict(off=None), "thresholds NULL": dict(lim=None), "pair_out NULL": dict(p=None),
           "ref NULL": dict(r=None), "mob NULL": dict(m=None), "residue NULL": dict(res=None), "partner NULL": dict(par=None),
           "atom_out NULL": dict(a=None), "swapped_out NULL": dict(s=None),
           "offsets end": dict(off=np.array([0, 7], np.int64)), "offsets start": dict(off=np.array([1, 6], np.int64)),
           "offsets decrease": dict(off=np.array([0, 6, 5], np.int64), n_pairs=2), "offsets end before total": dict(off=np.array([0, 5], np.int64)),
           "radius 0": dict(radius=0.0), "radius negative": dict(radius=-15.0), "radius nan": dict(radius=nan), "radius inf": dict(radius=inf),
           "residue starts at 1": dict(res=residue + 1), "residue decreases": dict(res=changed(residue, 5, 0)),
           "residue skips": dict(res=changed(changed(changed(residue, 3, 2), 4, 2), 5, 2)), "residue negative": dict(res=residue - 1),
           "second pair's residue does not start at 0": dict(off=two, n_pairs=2, par=np.full(6, -1, np.int32)),
           "partner out of its pair": dict(par=changed(partner, 2, 6)), "partner below -1": dict(par=changed(partner, 2, -2)),
           "partner in the other pair": dict(off=two, n_pairs=2, res=np.array([0, 0, 0, 0, 0, 0], np.int32), par=np.array([-1, -1, 3, 2, -1, -1], np.int32)),
           "partner is itself": dict(par=changed(partner, 2, 2)), "partner in another residue": dict(par=changed(changed(partner, 2, 3), 3, 2)),
           "partner not mutual": dict(par=changed(partner, 2, 0)), "unknown flag bits": dict(flags=2), "unknown flag bits beside the known": dict(flags=5)}
    for k in range(4):
        for what, v in (("0", 0.0), ("negative", -1.0), ("nan", nan), ("inf", inf)):
            bad[f"threshold {k} {what}"] = dict(lim=changed(limits, k, v))
    for what, kw in bad.items():
        assert call(**kw) == _lib.TH_EINVAL, what
        assert b"th_lddt_atoms:" in lib.th_last_error(), (what, lib.th_last_error())
    assert (atom == 77).all() and (swapped == 77).all() and (pair == 77).all()
    ms = (C.c_double * 2)(-1.0, -1.0)
    none = limits.ctypes.data_as(C.c_void_p)
    assert lib.th_lddt_atoms(0, None, None, None, None, 0, None, 0, 15.0, none, 0, None, None, None, C.cast(ms, C.POINTER(C.c_double))) == _lib.TH_OK
    assert list(ms) == [0.0, 0.0]                                                # no pairs: no launch
    assert lib.th_lddt_atoms(0, None, None, None, None, 1, None, 0, 15.0, none, 0, None, None, None, None) == _lib.TH_EINVAL
    with pytest.raises(ValueError):
        lddt_atoms.lddt_atoms_arrays(ref, ref, residue, partner, offsets, thresholds=(1.0, 2.0, 4.0))
    with pytest.raises(ValueError):
        lddt_atoms.lddt_atoms_arrays(ref, ref[:5], residue, partner, offsets)
    with pytest.raises(_lib.TimedHipError) as err:
        lddt_atoms.lddt_atoms_arrays(ref, ref, residue, partner, offsets, radius=-1.0)
    assert err.value.code == _lib.TH_EINVAL


def _small_pdb(path, n=14):
    native = ar.ubq()
    pdbio.write_pdb(path, pdbio.Model(1, native.residues[:n]))
    return pdbio.read_pdb(path)[0]


def _as_built(layouts):
    """sidechains.build replaced: every side chain 'built' at its native coordinates, CD1 and CD2 (OD1 and OD2, ...) exchanged"""
    out = []
    for layout in layouts:
        residues = layout.residues
        n = len(residues)
        names = [tuple(a for a in r.atoms if a not in sidechains.BACKBONE and a != "OXT")[:10] for r in residues]
        xyz = np.full((n, 10, 3), np.nan)
        for r, res in enumerate(residues):
            flip = {a: b for pair in ar.SYMMETRIC.get(res.name, ()) for a, b in (pair, pair[::-1])}
            for j, name in enumerate(names[r]):
                xyz[r, j] = res.atoms[flip.get(name, name)]
        count = np.array([len(t) for t in names], np.int32)
        out.append(sidechains.BuiltSidechains(residues, [r.name for r in residues], names, xyz, count, count.copy(), np.zeros(n), np.zeros(n, np.int32), 0,
                                              np.full((n, 4), np.nan), None, np.zeros((n, 4, 3))))
    return out


def test_command_lines_keep_their_files_without_the_flags_and_write_two_with_them(tmp_path, monkeypatch, capsys):
    import analyse_models
    import build_sidechains
    import pack_sidechains
    from timed_hip import packer, structure
    monkeypatch.setattr(superpose, "superpose_arrays", restated_superposition)
    monkeypatch.setattr(lddt_atoms, "lddt_atoms_arrays", restated_arrays)
    monkeypatch.setattr(sidechains, "build", lambda structures, **kw: _as_built([structure.rotamer_layout(s) if isinstance(s, pdbio.Model) else s
                                                                               for s in structures]))

    def packed(layouts, **kw):
        built = _as_built(layouts)
        n = len(built[0].residues)
        return [packer.PackedSidechains(np.full(n, -1, np.int16), np.full((n, 4), np.nan), np.full(n, -1, np.int8), np.zeros(n, np.int64),
                                        np.zeros(n, np.int64), 0, 0, 0, 0, True, 0, 0, b) for b in built]
    monkeypatch.setattr(packer, "pack", packed)
    (tmp_path / "pdb").mkdir()
    (tmp_path / "models").mkdir()
    native = _small_pdb(tmp_path / "pdb" / "1ubq.pdb")
    pdbio.write_pdb(tmp_path / "models" / "copy.pdb", native)
    shifted = pdbio.Model(1, [pdbio.Residue(r.chain, r.number, r.name, {a: x + (0.0 if a in sidechains.BACKBONE else 0.4) for a, x in r.atoms.items()},
                                            dict(r.elements)) for r in native.residues])
    pdbio.write_pdb(tmp_path / "models" / "shifted.pdb", shifted)

    def read(path):
        with open(path, newline="") as f:
            return list(csv.reader(f))
    # analyse_models.py
    parser = analyse_models.build_parser()
    common = ["--path_to_reference", str(tmp_path / "pdb" / "1ubq.pdb"), "--path_to_models", str(tmp_path / "models")]
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "plain")]))
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["model_scores.csv", "residue_deviation.csv"]
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "scored"), "--lddt_all_atom"]))
    assert sorted(p.name for p in (tmp_path / "scored").iterdir()) == ["model_lddt_all_atom.csv", "model_scores.csv", "residue_deviation.csv",
                                                                        "residue_lddt_all_atom.csv"]
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (tmp_path / "scored" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes()
    rows, per = read(tmp_path / "scored" / "model_lddt_all_atom.csv"), read(tmp_path / "scored" / "residue_lddt_all_atom.csv")
    assert rows[0] == lddt_atoms.MODEL_COLUMNS == ["label", "reference", "model", "n_atoms", "n_missing", "n_mismatched_residues", "n_included", "lddt",
                                                   "preserved_0.5", "preserved_1", "preserved_2", "preserved_4", "lddt_backbone", "lddt_sidechain",
                                                   "n_swapped_residues", "error"]
    assert per[0] == lddt_atoms.RESIDUE_COLUMNS == ["label", "chain", "number", "residue", "model_residue", "n_atoms", "n_missing", "n_included", "lddt", "swapped"]
    copy, moved = dict(zip(rows[0], rows[1])), dict(zip(rows[0], rows[2]))
    lists = lddt_atoms.atom_lists(native.residues, native.residues)
    assert copy["label"] == "copy.pdb" and float(copy["lddt"]) == 1.0 and int(copy["n_atoms"]) == len(lists.residue) and copy["error"] == ""
    assert float(copy["lddt_backbone"]) == 1.0 and float(copy["lddt_sidechain"]) == 1.0 and copy["n_swapped_residues"] == "0" and copy["n_missing"] == "0"
    assert float(moved["lddt_sidechain"]) < float(moved["lddt"]) < float(moved["lddt_backbone"]) < 1.0 and len(per) == 1 + 2 * 14
    assert [r[3] for r in per[1:15]] == [r.name for r in native.residues] and [int(r[5]) for r in per[1:15]] == np.bincount(lists.residue).tolist()
    args = parser.parse_args(["--pairs", "p.csv"])
    assert not hasattr(args, "lddt_all_atom") and not hasattr(args, "lddt_no_symmetry")
    # build_sidechains.py and pack_sidechains.py: the stand-in builds every side chain at its native place under exchanged names
    for module, flags, old in ((build_sidechains, ["--chi", "native"], ["1ubq_native_chi.pdb", "residue_sidechains.csv", "structure_sidechains.csv"]),
                               (pack_sidechains, [], ["1ubq_packed.pdb", "residue_packing.csv", "rotamer_labels.json", "structure_packing.csv"])):
        parser = module.build_parser()
        name = module.__name__
        module.main(parser.parse_args(["--path_to_pdb", str(tmp_path / "pdb"), "--path_to_output", str(tmp_path / name)] + flags))
        assert sorted(p.name for p in (tmp_path / name).iterdir()) == old, name
        module.main(parser.parse_args(["--path_to_pdb", str(tmp_path / "pdb"), "--path_to_output", str(tmp_path / (name + "_lddt")), "--lddt"] + flags))
        assert sorted(p.name for p in (tmp_path / (name + "_lddt")).iterdir()) == sorted(old + ["residue_sidechain_lddt.csv", "structure_sidechain_lddt.csv"])
        for file in old:
            assert (tmp_path / (name + "_lddt") / file).read_bytes() == (tmp_path / name / file).read_bytes(), (name, file)
        rows, per = read(tmp_path / (name + "_lddt") / "structure_sidechain_lddt.csv"), read(tmp_path / (name + "_lddt") / "residue_sidechain_lddt.csv")
        assert rows[0] == lddt_atoms.MODEL_COLUMNS and per[0] == lddt_atoms.RESIDUE_COLUMNS and len(rows) == 2 and len(per) == 15
        row = dict(zip(rows[0], rows[1]))
        symmetric = sum(1 for r in native.residues if r.name in ar.SYMMETRIC)
        assert float(row["lddt"]) == 1.0 and float(row["lddt_sidechain"]) == 1.0 and int(row["n_swapped_residues"]) == symmetric == 3     # PHE 4, VAL 5, LEU 8: resolved
        assert [int(r[9]) for r in per[1:]] == [1 if r.name in ar.SYMMETRIC else 0 for r in native.residues]
        assert not hasattr(parser.parse_args(["--path_to_pdb", "x"]), "lddt")
    capsys.readouterr()


def test_results_through_the_batch_driver_and_the_byte_budget(monkeypatch, golden):
    calls = []

    def counted(ref_xyz, mob_xyz, residue, partner, offsets, *a, **kw):
        calls.append(len(offsets) - 1)
        return restated_arrays(ref_xyz, mob_xyz, residue, partner, offsets, *a, **kw)
    monkeypatch.setattr(lddt_atoms, "lddt_atoms_arrays", counted)
    native = ar.ubq()
    flipped = pdbio.Model(1, [pdbio.Residue(r.chain, r.number, r.name, dict(r.atoms), dict(r.elements)) for r in native.residues])
    for res in flipped.residues:
        for a, b in ar.SYMMETRIC.get(res.name, ()):
            res.atoms[a], res.atoms[b] = res.atoms[b], res.atoms[a]
    stats = {}
    first, second, third = lddt_atoms.lddt_atoms([(native, native), (native, flipped), (native, "absent.pdb")], stats=stats)
    assert calls == [2] and stats["submissions"] == 1 and "absent.pdb" in third.error and np.isnan(third.lddt) and third.n_atoms == 0
    assert first.error is None and first.lddt == 1.0 and first.n_atoms == 601 and first.n_included == 171464 and first.n_swapped_residues == 0
    assert second.lddt == 1.0 and second.n_swapped_residues == 31 and second.swapped.sum() == 31 and same_bytes(second.n_i, first.n_i)
    assert first.lddt_backbone == 1.0 and first.lddt_sidechain == 1.0 and len(first.lddt_i) == 76 and first.atoms_i.sum() == 601
    assert first.n_i.sum() == 171464 and first.n_i.dtype == np.int64 and first.preserved == (1.0, 1.0, 1.0, 1.0)
    (named,) = lddt_atoms.lddt_atoms([(native, flipped)], symmetry=False)
    want = golden["flipped_named_pair"]
    assert named.n_included == want[2] and named.lddt == ar.score(want) and named.n_swapped_residues == 0 and named.lddt_backbone > named.lddt_sidechain
    rows, backbone = golden["flipped_named_atom"].astype(np.int64), golden["self_backbone"]
    assert named.lddt_backbone == rows[backbone, 1:].sum() / (4 * rows[backbone, 0].sum())
    assert named.lddt_sidechain == rows[~backbone, 1:].sum() / (4 * rows[~backbone, 0].sum())
    starts = np.flatnonzero(np.diff(golden["self_residue"], prepend=-1))
    sums = np.add.reduceat(rows, starts, axis=0)
    assert named.n_i.tolist() == sums[:, 0].tolist() and named.lddt_i.tolist() == (sums[:, 1:].sum(axis=1) / (4.0 * sums[:, 0])).tolist()
    # the byte budget counts bytes per atom: two structures of 601 atoms fit, three do not
    del calls[:]
    stats = {}
    split = lddt_atoms.lddt_atoms([(native, native), (native, flipped), (native, native)], budget_bytes=2 * 601 * lddt_atoms._ATOM_BYTES + 100, stats=stats)
    assert calls == [2, 1] and stats["submissions"] == 2 and split[1].n_swapped_residues == 31 and same_bytes(split[2].lddt_i, first.lddt_i)
    assert lddt_atoms.lddt_atoms([]) == []
    with pytest.raises(ValueError):
        lddt_atoms.lddt_atoms([], pair_by="alignment")
