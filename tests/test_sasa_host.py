"""Solvent-accessible surface area without a GPU: the NumPy restatement (tests/sasa_restatement.py) against the committed fixture and
the analytic cases of the rule's write-up; the header prototypes, the ctypes entries, the build list and the unpinned-parity phrase;
th_sasa_sphere; every refusal of th_sasa; the atom rule of the layout, the radii, the byte budget with the mask counted; areas,
relative accessibility, burial classes and the interface with the kernel call replaced by the restatement; analyse_properties.py and
analyse_models.py --sasa the same way."""
import csv
import ctypes as C
import gzip
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sasa_restatement as sr  # noqa: E402
import superpose_restatement as spr  # noqa: E402
from timed_hip import _lib, pdbio, sasa, structure, superpose  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHRASE = sr.PHRASE


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restated_arrays(xyz, radius, offsets, probe=1.4, points=None, n_points=96, device=0, mask=False, timing=None):
    """sasa.sasa_arrays with the GPU call replaced by the restatement"""
    points = sasa.sphere_points(n_points) if points is None else points
    exposed, words, totals = sr.restate_batch(np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(radius, np.float64), np.asarray(offsets), probe, points)
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0)
    return sasa.SasaTables(exposed, words if mask else None, totals)


def restated_superposition(ref_xyz, mob_xyz, offsets, cycles=5, cutoff=2.0, device=0, transform=False, timing=None):
    dist, kept, rmsd, counts, moves, _, _ = spr.restate_batch(ref_xyz, mob_xyz, np.asarray(offsets), cycles, cutoff)
    return superpose.Superposed(dist, kept, rmsd, counts, moves.reshape(-1, 3, 4) if transform else None)


@pytest.fixture(scope="module")
def golden():
    return np.load(sr.GOLDEN)


def dimer_model():
    """1ubq (chain A) and its moved copy as chain B, as a pdbio.Model: what sasa_restatement.cases()["ubq_dimer"] holds"""
    model = structure.first_model(sr.UBQ)
    polymer = [r for r in model.residues if not r.hetero]
    flat = np.array([pos for r in polymer for pos in r.atoms.values()], dtype=np.float64)
    moved = iter(sr.moved_copy(flat))
    copies = [pdbio.Residue("B", r.number, r.name, {name: next(moved) for name in r.atoms}, dict(r.elements)) for r in polymer]
    return pdbio.Model(1, polymer + copies)


def test_restatement_equals_the_fixture_and_the_written_numbers(lib, golden):
    assert os.path.getsize(sr.GOLDEN) < 256 * 1024
    points_96, points_960 = golden["points_96"], golden["points_960"]
    # the fixture carries the points it was made with: another libm may differ from them in the last place, and nothing hangs on it
    assert np.abs(points_96 - sasa.sphere_points(96)).max() < 1e-15 and np.abs(points_960 - sasa.sphere_points(960)).max() < 1e-15
    again = sr.golden_arrays(points_96, points_960)
    assert golden["cases"].tolist() == list(sr.CASES) and sorted(golden.files) == sorted(again)
    for key in golden.files:
        assert same_bytes(golden[key], np.asarray(again[key])), key
    text = open(os.path.join(ROOT, "tests", "golden", "make_sasa_golden.py")).read()
    assert "NOT by the kernel" in text and PHRASE in text
    for name in sr.CASES:
        assert golden[f"{name}_exposed"].dtype == np.int32 and golden[f"{name}_mask"].dtype == np.uint64 and golden[f"{name}_totals"].dtype == np.int64
        exposed, mask = golden[f"{name}_exposed"], golden[f"{name}_mask"]
        bits = np.array([[bin(int(w)).count("1") for w in row] for row in mask]).reshape(len(exposed), -1).sum(axis=1)
        assert bits.tolist() == np.maximum(exposed, 0).tolist(), name                                           # count = popcount of the mask
    # the analytic cases, spelled out here once more
    assert golden["lone_exposed"].tolist() == [96] and golden["pair_3_exposed"].tolist() == [72, 72] and golden["pair_6_exposed"].tolist() == [96, 96]
    assert golden["inside_exposed"].tolist() == [0, 96] and golden["tie_exposed"].tolist() == [3, 3] and golden["tie_near_exposed"].tolist() == [2, 2]
    assert sr.ANALYTIC == {name: golden[f"{name}_exposed"].tolist() for name in sr.ANALYTIC}
    # the buried cap of pair_3 is z_k > 0.5, k <= 23, on the first atom and its mirror image on the second
    assert int(golden["pair_3_mask"][0, 0]) & 0xFFFFFF == 0 and int(golden["pair_3_mask"][0, 0]) >> 24 == (1 << 40) - 1
    assert (points_96[:24, 2] > 0.5).all() and (points_96[24:, 2] < 0.5).all() and golden["pair_3_mask"][0, 1] == (1 << 32) - 1
    assert golden["tie_near_mask"].tolist() == [[0b110], [0b101]] and golden["tie_mask"].tolist() == [[7], [7]]
    # 1ubq: the numbers of the write-up
    xyz, radius, group, polar, backbone, names = sr.ubq_atoms()
    assert len(xyz) == 602 and len(names) == 76 and group.max() == 75
    ubq = sr.restate(xyz, radius, sr.PROBE, points_96, every_pair=True)
    assert ubq["ties"] == 0 and ubq["n_near"].max() == 59 and round(float(ubq["n_near"].mean()), 1) == 37.0
    assert golden["ubq_totals"].tolist() == [602, 271, int(golden["ubq_exposed"].sum())]
    assert [round(float(v), 1) for v in golden["ubq_area"]] == [4895.6, 2760.2, 2135.4] and round(float(golden["ubq_960_area"][0]), 1) == 4872.5
    rsa = golden["ubq_residue_area"][0] / np.array([sr.MAX_ASA[n] for n in names])
    classes = sr.burial(rsa)
    assert [classes.count(k) for k in (0, 1, 2)] == [24, 35, 17] and 1.35 < rsa[75] < 1.45 and names[75] == "GLY"
    assert golden["ubq_probe0_totals"][1] == 0 and golden["ubq_probe0_area"][0] > 6000.0           # the van der Waals surface: every atom shows
    assert 100.0 < float(golden["ubq_dimer_interface"]) < 1000.0 and (golden["ubq_dimer_area_lost"] >= 0).all()
    assert sr.restate(np.zeros((0, 3)), np.zeros(0), 1.4, points_96)["totals"].tolist() == [0, 0, 0]
    # invalid atoms: -1, mask 0, and they occlude nothing
    one = sr.restate(np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.0, 1e200]]), np.array([1.7, 1.7, -2.0, 1.7]), 1.4, points_96)
    assert one["exposed"].tolist() == [96, -1, -1, 96] and not one["mask"][1:3].any() and one["totals"].tolist() == [2, 0, 192]


_CTYPES = {"int": "c_int", "int32_t": "c_int", "int64_t": "c_long", "double": "c_double", "const double*": "c_void_p", "const int64_t*": "c_void_p",
           "int32_t*": "c_void_p", "int64_t*": "c_void_p", "uint64_t*": "c_void_p", "double*": ("c_void_p", "LP_c_double")}


def test_header_ctypes_build_list_and_the_unpinned_parity_phrase():
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    for name, count in (("th_sasa", 13), ("th_sasa_sphere", 2)):
        m = re.search(r"^(\w+) %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        res, args = _lib.PROTOTYPES[name]
        assert res.__name__ == _CTYPES[m.group(1)]
        declared = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(2).split(",")]
        assert len(declared) == len(args) == count, (declared, args)
        for c_type, ct in zip(declared, args):
            want = _CTYPES[c_type]
            assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (name, c_type, ct)
    before = header[:re.search(r"^int th_sasa\(", header, re.M).start()]
    block = before[before.rindex("/* ----"):]
    assert block.startswith("/* ---- ") and "*** " + PHRASE + " ***" in block
    flat = re.sub(r"[\s*]+", " ", block)
    for words in ("Shrake & Rupley (1973)", "Bio, freesasa and mdtraj", "R_i = radius_i + probe", "R_i > 0", "s < t t, strict", "PART OF THE RULE",
                  "x_i + R_i u_kx", "< R_j R_j, strict", "exactly on a neighbour's sphere is exposed", "no fused multiply-add", "2^31 - 257",
                  "1 <= n_points <= 1024", "32 bytes per atom in, 4 + 8 ceil(n_points / 64) bytes per atom out", "TH_ENOMEM", "No atomics",
                  "4 pi R_i R_i / n_points"):
        assert words in flat, words
    import __graft_entry__
    assert "sasa.hip" in __graft_entry__.HIP_SOURCES
    source = open(os.path.join(ROOT, "timed-design_amd", "csrc", "sasa.hip")).read()
    assert PHRASE in source and "#pragma clang fp contract(off)" in source and "atomic" not in source.replace("No atomics", "")
    assert "ThLayout" in source and "ThCall" in source and "th_check_offsets" in source
    assert PHRASE in sasa.__doc__ and "WRITTEN FROM MEMORY, NOT FETCHED" in sasa.__doc__
    import analyse_models
    import analyse_properties
    for module in (analyse_models, analyse_properties):
        text = re.sub(r"\s+", " ", module.build_parser().format_help())
        assert PHRASE in text and "--sasa" in text and "WRITTEN FROM MEMORY, NOT FETCHED" in text, module.__name__
        for flag in ("--sasa", "--sasa_points", "--sasa_probe", "--rsa_core", "--rsa_surface"):
            assert dict(module.CLI_FLAGS)[flag]["default"] == "==SUPPRESS=="
    assert all(dict(analyse_properties.CLI_FLAGS)[flag]["default"] == "==SUPPRESS==" for flag in ("--sasa_hetero", "--sasa_interface"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert PHRASE in readme and "th_sasa" in readme and "th_sasa" in design and PHRASE in design and "WRITTEN FROM MEMORY, NOT FETCHED" in readme
    from design_utils import amino_acids
    assert amino_acids.vdw_radii == sr.RADII and amino_acids.VDW_RADIUS_OTHER == sr.OTHER_RADIUS and amino_acids.max_asa == sr.MAX_ASA
    assert amino_acids.WATER_NAMES == sr.WATERS
    source = open(os.path.join(ROOT, "timed-design_amd", "design_utils", "amino_acids.py")).read()
    assert "WRITTEN FROM MEMORY, NOT FETCHED" in source and "Tien et al. 2013" in source


def ulps(a, b=1.0):
    return abs(a - b) / np.spacing(b)


def test_th_sasa_sphere(lib):
    for n in (1, 2, 63, 96, 960, 1024):
        p = sasa.sphere_points(n)
        assert p.shape == (n, 3) and p.dtype == np.float64 and np.isfinite(p).all()
        norm = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        assert ulps(norm).max() <= 4, (n, ulps(norm).max())
        assert (np.diff(p[:, 2]) < 0).all() and abs(p[:, 2].sum()) < 1e-12                    # z strictly decreasing, symmetric
        assert np.abs(p - sr.sphere(n)).max() < 1e-12                                           # the formula, within what two libm's may differ
        assert same_bytes(p, sasa.sphere_points(n))
    assert sasa.sphere_points(1).tolist() == [[1.0, 0.0, 0.0]]
    assert sasa.sphere_points(96)[0, 2] == 1.0 - 1.0 / 96.0 and sasa.sphere_points(96)[95, 2] == 1.0 - 191.0 / 96.0
    guard = np.full((2, 3), 77.0)
    for n in (0, -1, 1025, 1 << 20):
        assert lib.th_sasa_sphere(n, guard.ctypes.data_as(C.c_void_p)) == _lib.TH_EINVAL and b"th_sasa_sphere" in lib.th_last_error()
    assert lib.th_sasa_sphere(2, None) == _lib.TH_EINVAL and (guard == 77.0).all()
    with pytest.raises(_lib.TimedHipError):
        sasa.sphere_points(0)


def test_library_exports_th_sasa_and_checks_arguments_without_a_gpu(lib):
    xyz, radius, offsets, points = np.zeros((2, 3)), np.full(2, 1.7), np.array([0, 2], np.int64), sasa.sphere_points(96)
    exposed, mask, totals = np.full(2, 77, np.int32), np.full((2, 2), 77, np.uint64), np.full((1, 3), 77, np.int64)
    bad_points = points.copy()
    bad_points[95, 1] = np.inf
    nan_points = points.copy()
    nan_points[0, 0] = np.nan

    def call(x=xyz, r=radius, total=2, off=offsets, n=1, probe=1.4, pts=points, n_points=96, e=exposed, m=mask, t=totals):
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)        # noqa: E731
        ms = (C.c_double * 2)(-1.0, -1.0)
        rc = lib.th_sasa(0, p(x), p(r), total, p(off), n, probe, p(pts), n_points, p(e), p(m), p(t), C.cast(ms, C.POINTER(C.c_double)))
        assert rc == _lib.TH_OK or list(ms) == [-1.0] * 2
        return rc
    bad = {"negative total": dict(total=-1), "negative structures": dict(n=-1), "total too large": dict(total=(1 << 31) - 256),
           "structures too large": dict(n=1 << 31), "no points": dict(n_points=0), "negative points": dict(n_points=-5),
           "too many points": dict(n_points=1025), "points NULL": dict(pts=None), "an infinite point": dict(pts=bad_points),
           "a NaN point": dict(pts=nan_points), "offsets NULL": dict(off=None), "structure_out NULL": dict(t=None), "xyz NULL": dict(x=None),
           "radius NULL": dict(r=None), "exposed_out NULL": dict(e=None), "offsets end": dict(off=np.array([0, 3], np.int64)),
           "offsets start": dict(off=np.array([1, 2], np.int64)), "offsets decrease": dict(off=np.array([0, 2, 1], np.int64), n=2),
           "offsets end before total": dict(off=np.array([0, 1], np.int64)), "atoms without a structure": dict(n=0)}
    for what, kw in bad.items():
        assert call(**kw) == _lib.TH_EINVAL, what
        assert b"th_sasa" in lib.th_last_error() and b"th_sasa_sphere" not in lib.th_last_error(), what
    assert (exposed == 77).all() and (mask == 77).all() and (totals == 77).all()
    # total = 0: success without a launch (no GPU here), with and without structures
    ms = (C.c_double * 2)(-1.0, -1.0)
    pts = points.ctypes.data_as(C.c_void_p)
    assert lib.th_sasa(0, None, None, 0, None, 0, 1.4, pts, 96, None, None, None, C.cast(ms, C.POINTER(C.c_double))) == _lib.TH_OK
    assert list(ms) == [0.0, 0.0]
    empty = sasa.sasa_arrays(np.zeros((0, 3)), np.zeros(0), [0, 0, 0], mask=True)
    assert empty.exposed.shape == (0,) and empty.mask.shape == (0, 2) and empty.structure.tolist() == [[0, 0, 0]] * 2
    with pytest.raises(ValueError):
        sasa.sasa_arrays(xyz, radius[:1], offsets)
    with pytest.raises(ValueError):
        sasa.sasa_arrays(xyz, radius, [])
    with pytest.raises(_lib.TimedHipError) as err:
        sasa.sasa_arrays(xyz, radius, [0, 3])
    assert err.value.code == _lib.TH_EINVAL


def test_atom_rule_radii_and_the_byte_budget(monkeypatch, golden, tmp_path):
    model = structure.first_model(sr.UBQ)
    lay = sasa.atom_layout(model)
    xyz, radius, group, polar, backbone, names = sr.ubq_atoms()
    assert same_bytes(lay.xyz, xyz) and same_bytes(lay.radius, radius) and same_bytes(lay.group, group) and len(lay.residues) == 76
    assert lay.polar.tolist() == polar.tolist() and lay.backbone.tolist() == backbone.tolist() and [r.name for r in lay.residues] == names
    assert sum(1 for r in model.residues if r.hetero) == 58 and all(sasa.is_water(r) for r in model.residues if r.hetero)
    assert same_bytes(sasa.atom_layout(model, include_hetero=True).xyz, xyz)                    # waters never occlude
    # hydrogens, alternate locations (pdbio keeps the first), waters, hetero atoms, elements and radii
    z = np.zeros(3)
    res = [pdbio.Residue("B", "1", "GLY", {"N": z, "CA": z + 1, "H": z + 2, "1HA": z + 3, "C": z + 4, "O": z + 5},
                         {"N": "N", "CA": "C", "H": "H", "1HA": "", "C": "C", "O": "O"}),
           pdbio.Residue("B", "2", "HOH", {"O": z + 6}, {"O": "O"}, hetero=True),
           pdbio.Residue("A", "1", "MSE", {"SE": z + 7, "CA": z + 8, "SD": z + 9, "P": z + 10, "ZN": z + 11, "X": z + 12},
                         {"SE": "SE", "CA": "", "SD": "s", "P": "P", "ZN": "ZN", "X": "1"}),
           pdbio.Residue("A", "2", "SO4", {"S": z + 13, "O1": z + 14}, {"S": "S", "O1": "O"}, hetero=True),
           pdbio.Residue("A", "3", "DOD", {"O": z + 15}, {"O": "O"}, hetero=True)]
    plain = sasa.atom_layout(pdbio.Model(1, res))
    assert [name for _, name in plain.atoms] == ["N", "CA", "C", "O", "SE", "CA", "SD", "P", "ZN", "X"] and plain.group.tolist() == [0] * 4 + [1] * 6
    assert plain.radius.tolist() == [1.55, 1.70, 1.70, 1.52, 1.90, 1.70, 1.80, 1.80, 1.80, 1.80]
    assert plain.polar.tolist() == [True, False, False, True] + [False] * 6 and plain.backbone.tolist() == [True] * 4 + [False, True] + [False] * 4
    assert [(r.chain, r.number) for r in plain.residues] == [("B", "1"), ("A", "1")]
    het = sasa.atom_layout(pdbio.Model(1, res), include_hetero=True)
    assert [name for _, name in het.atoms][10:] == ["S", "O1"] and het.group.tolist()[10:] == [-1, -1] and len(het.residues) == 2
    assert sasa.atom_layout(pdbio.Model(1, res), radii={"C": 2.0}).radius.tolist() == [1.8, 2.0, 2.0, 1.8, 1.8, 2.0, 1.8, 1.8, 1.8, 1.8]
    assert sasa.element_of("CA", "") == "C" and sasa.element_of("1HB", "") == "H" and sasa.element_of("CA", "Ca") == "CA"
    # both parsers — pdbio above and the restatement's own reader of the fixed columns — give the same atoms, from the gzipped file and
    # from a plain copy with a hydrogen and a second alternate location added, which neither may take
    with gzip.open(sr.UBQ, "rt") as f:
        lines = f.read().splitlines(keepends=True)
    first = next(k for k, line in enumerate(lines) if line[:6] == "ATOM  ")
    extra = [lines[first][:12] + " H1 " + lines[first][16:76] + " H" + lines[first][78:], lines[first][:16] + "B" + lines[first][17:30] + "   9.999" + lines[first][38:]]
    (tmp_path / "plain.pdb").write_text("".join(lines[:first + 1] + extra + lines[first + 1:]))
    again = sasa.atom_layout(structure.first_model(tmp_path / "plain.pdb"))
    assert same_bytes(again.xyz, xyz) and same_bytes(again.radius, radius) and same_bytes(again.group, group)
    assert len(structure.first_model(tmp_path / "plain.pdb").residues[0].atoms) == len(model.residues[0].atoms) + 1          # the hydrogen was read
    # areas and classes
    assert sasa.burial_classes([0.0, 0.19, 0.2, 0.49, 0.5, 1.4, np.nan]).tolist() == [0, 0, 1, 1, 2, 2, -1]
    assert sasa.burial_classes([0.3], core=0.4).tolist() == [0] and sasa.burial_classes([0.3], surface=0.3).tolist() == [2]
    area = sasa.atom_areas(np.array([96, 0, -1, 48]), np.array([1.7, 1.7, 1.7, 1.52]), 1.4, 96)
    R = 1.7 + 1.4
    assert area.tolist() == [96.0 * (4.0 * math.pi * R * R / 96.0), 0.0, 0.0, 48.0 * (4.0 * math.pi * (1.52 + 1.4) * (1.52 + 1.4) / 96.0)]
    assert same_bytes(area, sr.atom_areas(np.array([96, 0, -1, 48]), np.array([1.7, 1.7, 1.7, 1.52]), 1.4, 96))
    # the byte budget: 36 bytes per atom, and 8 per 64 points when the mask is asked for
    assert sasa.atom_bytes(96) == 36 and sasa.atom_bytes(96, True) == 36 + 16 and sasa.atom_bytes(1024, True) == 36 + 128 and sasa.mask_words(65) == 2
    calls = []

    def counted(xyz, radius, offsets, *a, **kw):
        calls.append(len(offsets) - 1)
        return restated_arrays(xyz, radius, offsets, *a, **kw)
    monkeypatch.setattr(sasa, "sasa_arrays", counted)
    layouts = [lay] * 5
    stats = {}
    whole = sasa.sasa_layouts(layouts)
    split = sasa.sasa_layouts(layouts, budget_bytes=2 * 602 * 36 + 10, stats=stats)
    masked = sasa.sasa_layouts(layouts, budget_bytes=2 * 602 * 36 + 10, mask=True)               # the mask counts: one structure per call
    assert calls == [5, 2, 2, 1, 1, 1, 1, 1, 1] and stats["submissions"] == 3
    for a, b, c in zip(whole, split, masked):
        assert same_bytes(a.exposed, golden["ubq_exposed"]) and same_bytes(b.residue_area, golden["ubq_residue_area"][0]) and a.error is None
        assert a.mask is None and same_bytes(c.mask, golden["ubq_mask"]) and a.total_area == b.total_area == float(golden["ubq_area"][0])
    one = whole[0]
    assert same_bytes(one.polar_area, golden["ubq_residue_area"][1]) and same_bytes(one.apolar_area, golden["ubq_residue_area"][2])
    assert same_bytes(one.backbone_area, golden["ubq_residue_area"][3]) and (one.total_polar_area, one.total_apolar_area) == tuple(golden["ubq_area"][1:])
    assert one.counts == (24, 35, 17) and one.n_atoms == 602 and one.n_buried_atoms == 271 and one.burial_letters.count("C") == 24
    assert 1.35 < one.rsa[75] < 1.45 and abs(one.apolar_share - 2135.4 / 4895.6) < 1e-4 and np.isnan(one.interface_area) and one.area_lost is None
    # a file that cannot be read carries its error; a residue outside the table is unknown
    stats = {}
    first, missing, second = sasa.sasa([sr.UBQ, os.path.join(ROOT, "tests", "golden", "absent.pdb"), model], stats=stats)
    assert same_bytes(first.exposed, second.exposed) and "absent.pdb" in missing.error and len(missing.exposed) == 0 and stats["files_parsed"] == 2
    assert sasa.sasa([]) == []
    odd = sasa.sasa([pdbio.Model(1, res)])[0]
    assert np.isnan(odd.rsa[1]) and odd.burial.tolist()[1] == -1 and odd.burial_letters[1] == "?" and odd.rsa[0] == odd.residue_area[0] / 104.0
    # the interface: the dimer's chains alone follow it in the same batch
    del calls[:]
    dimer, single = sasa.sasa([dimer_model(), model], interface=True)
    assert calls == [4]
    assert same_bytes(dimer.exposed, golden["ubq_dimer_exposed"]) and same_bytes(dimer.residue_area, golden["ubq_dimer_residue_area"][0])
    assert same_bytes(dimer.area_lost, golden["ubq_dimer_area_lost"]) and dimer.interface_area == float(golden["ubq_dimer_interface"]) > 0
    assert single.interface_area == 0.0 and not single.area_lost.any() and len(dimer.residues) == 152
    # the pseudo-ligand of the fixture through include_hetero
    waters = [r for r in model.residues if r.hetero][:3]
    ligand = pdbio.Residue("A", "900", "LIG", {name: w.atoms["O"] for name, w in zip(("S", "O1", "O2"), waters)}, {"S": "S", "O1": "O", "O2": "O"}, hetero=True)
    with_ligand = pdbio.Model(1, [r for r in model.residues if not r.hetero] + [ligand])
    got = sasa.sasa([with_ligand], include_hetero=True)[0]
    assert same_bytes(got.exposed, golden["ubq_hetero_exposed"]) and same_bytes(got.residue_area, golden["ubq_hetero_residue_area"][0])
    assert got.total_area == float(golden["ubq_hetero_area"][0]) and same_bytes(sasa.sasa([with_ligand])[0].exposed, golden["ubq_exposed"])
    from design_utils.analyse_utils import extract_sasa_from_ampal
    assert extract_sasa_from_ampal(sr.UBQ) == [golden["ubq_residue_area"][0].tolist()]
    assert [len(c) for c in extract_sasa_from_ampal(dimer_model(), load_pdb=False)] == [76, 76]
    assert sum(1 for line in lines if line[:6] == "HETATM") == 58


def _write_ubq(path):
    """1ubq's ATOM records (no water)"""
    with gzip.open(sr.UBQ, "rt") as f:
        lines = [line for line in f if line[:6] == "ATOM  "]
    path.write_text("".join(lines) + "END\n")


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_analyse_properties_writes_its_two_files_and_leaves_the_others(tmp_path, monkeypatch, capsys, golden):
    import analyse_properties as ap
    monkeypatch.setattr(sasa, "sasa_arrays", restated_arrays)
    monkeypatch.setattr(structure, "contact_numbers", lambda xyz, offsets, radius=7.0, group=None, selected=None, n_groups=0, device=0, atoms=True,
                        timing=None: (np.zeros(len(xyz), np.int32), np.arange(n_groups, dtype=np.float64)))
    (tmp_path / "pdb").mkdir()
    _write_ubq(tmp_path / "pdb" / "ubq.pdb")
    pdbio.write_pdb(tmp_path / "pdb" / "dimer.pdb", dimer_model())
    parser = ap.build_parser()
    common = ["--path_to_pdb", str(tmp_path / "pdb")]
    plain, out = tmp_path / "plain", tmp_path / "out"
    assert not any(k.startswith(("sasa", "rsa")) for k in vars(parser.parse_args(common))) and parser.parse_args(common + ["--sasa"]).sasa is True
    ap.main(parser.parse_args(common + ["--path_to_output", str(plain)]))
    assert sorted(p.name for p in plain.iterdir()) == ["residue_properties.csv", "structure_properties.csv"]
    assert "in 1 GPU submission(s)" in capsys.readouterr().out
    ap.main(parser.parse_args(common + ["--path_to_output", str(out), "--sasa", "--sasa_interface"]))
    assert "in 2 GPU submission(s)" in capsys.readouterr().out
    assert sorted(p.name for p in out.iterdir()) == ["residue_properties.csv", "residue_sasa.csv", "structure_properties.csv", "structure_sasa.csv"]
    for name in ("residue_properties.csv", "structure_properties.csv"):
        assert (out / name).read_bytes() == (plain / name).read_bytes()
    per, whole = _read(out / "residue_sasa.csv"), _read(out / "structure_sasa.csv")
    assert per[0] == ap.SASA_RESIDUE_COLUMNS + ["area_lost_in_complex"] and whole[0] == ap.SASA_COLUMNS + ["interface_area"] and len(per) == 1 + 152 + 76
    assert [r[0] for r in whole[1:]] == ["dimer.pdb", "ubq.pdb"]
    ubq = [r for r in per[1:] if r[0] == "ubq.pdb"]
    assert [r[1:4] for r in ubq[:2]] == [["A", "1", "MET"], ["A", "2", "GLN"]]
    assert [[float(v) for v in r[4:8]] for r in ubq] == golden["ubq_residue_area"].T.tolist()
    assert "".join(r[9] for r in ubq).count("C") == 24 and set(r[10] for r in ubq) == {"0.0"}
    row = dict(zip(whole[0], whole[2]))
    assert [float(row[k]) for k in ("total_area", "polar_area", "apolar_area")] == golden["ubq_area"].tolist()
    assert [int(row[k]) for k in ("atoms", "residues", "n_core", "n_boundary", "n_surface", "buried_atoms")] == [602, 76, 24, 35, 17, 271]
    assert float(row["interface_area"]) == 0.0 and float(dict(zip(whole[0], whole[1]))["interface_area"]) == float(golden["ubq_dimer_interface"])
    assert [float(r[10]) for r in per[1:153]] == golden["ubq_dimer_area_lost"].tolist()
    # other points, probe and thresholds; a prediction entropy per burial class through the pairing of --secondary_structure
    other = tmp_path / "other"
    ap.main(parser.parse_args(["--path_to_pdb", str(tmp_path / "pdb" / "ubq.pdb"), "--path_to_output", str(other), "--sasa", "--sasa_points", "960",
                               "--rsa_core", "0.0", "--rsa_surface", "0.0"]))
    whole = _read(other / "structure_sasa.csv")
    row = dict(zip(whole[0], whole[1]))
    assert float(row["total_area"]) == float(golden["ubq_960_area"][0]) and (row["n_core"], row["n_surface"]) == ("0", "76")
    lay = sasa.atom_layout(structure.first_model(sr.UBQ))
    res = sasa.sasa_layouts([lay])[0]
    value = np.arange(76, dtype=np.float64) / 10.0
    want = [float(value[res.burial == k].mean()) for k in (0, 1, 2)]
    assert ap.class_entropy(ap.paired_entropy("sub/1ubq.pdb1.gz", res.residues, {"1ubq": value}, None), res.burial.tolist(), (0, 1, 2)) == want
    with pytest.raises(SystemExit):
        ap.main(parser.parse_args(common + ["--path_to_output", str(other), "--sasa", "--sasa_points", "2000"]))


def test_analyse_models_writes_its_two_files_and_leaves_the_others(tmp_path, monkeypatch, capsys, golden):
    import analyse_models
    calls = []

    def counted(xyz, radius, offsets, *a, **kw):
        calls.append(len(offsets) - 1)
        return restated_arrays(xyz, radius, offsets, *a, **kw)
    monkeypatch.setattr(superpose, "superpose_arrays", restated_superposition)
    monkeypatch.setattr(sasa, "sasa_arrays", counted)
    (tmp_path / "models").mkdir()
    _write_ubq(tmp_path / "native.pdb")
    _write_ubq(tmp_path / "models" / "same.pdb")
    noisy = pdbio.read_pdb(tmp_path / "native.pdb")[0]
    rng = np.random.default_rng(4)
    for r in noisy.residues:
        for name in r.atoms:
            r.atoms[name] = r.atoms[name] + rng.normal(0.0, 0.6, 3)
    pdbio.write_pdb(tmp_path / "models" / "noisy.pdb", noisy)
    parser = analyse_models.build_parser()
    common = ["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models", str(tmp_path / "models")]
    plain, out = tmp_path / "plain", tmp_path / "out"
    assert "sasa" not in vars(parser.parse_args(common))
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(plain)]))
    assert sorted(p.name for p in plain.iterdir()) == ["model_scores.csv", "residue_deviation.csv"] and calls == []
    capsys.readouterr()
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(out), "--sasa"]))
    assert calls == [3]                                  # the native once and the two models: one batch of three
    assert "3 files parsed in 2 GPU submission(s)" in capsys.readouterr().out
    assert sorted(p.name for p in out.iterdir()) == ["model_sasa.csv", "model_scores.csv", "residue_deviation.csv", "residue_sasa.csv"]
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (out / name).read_bytes() == (plain / name).read_bytes()
    scores, per = _read(out / "model_sasa.csv"), _read(out / "residue_sasa.csv")
    assert scores[0] == analyse_models.SASA_COLUMNS and per[0] == analyse_models.RESIDUE_SASA_COLUMNS
    assert [r[0] for r in scores[1:]] == ["noisy.pdb", "same.pdb"] and len(per) == 1 + 2 * 76
    noise, same = (dict(zip(scores[0], r)) for r in scores[1:])
    assert (same["n_paired"], same["burial_agreement"], same["mean_abs_rsa_difference"], same["error"]) == ("76", "1.0", "0.0", "")
    assert abs(float(same["rsa_correlation"]) - 1.0) < 1e-12
    assert float(same["reference_total_area"]) == float(same["model_total_area"]) == float(golden["ubq_area"][0])
    assert float(same["reference_apolar_area"]) == float(golden["ubq_area"][2])
    native = sasa.sasa_layouts([sasa.atom_layout(structure.first_model(tmp_path / "native.pdb"))])[0]
    model = sasa.sasa_layouts([sasa.atom_layout(structure.first_model(tmp_path / "models" / "noisy.pdb"))])[0]
    agreement = float((native.burial == model.burial).mean())
    assert float(noise["burial_agreement"]) == agreement < 1.0 and float(noise["mean_abs_rsa_difference"]) == float(np.abs(native.rsa - model.rsa).mean()) > 0
    assert abs(float(noise["rsa_correlation"]) - float(np.corrcoef(native.rsa, model.rsa)[0, 1])) < 1e-12 and float(noise["model_total_area"]) == model.total_area
    mine = [r for r in per[1:] if r[0] == "noisy.pdb"]
    assert "".join(r[8] for r in mine) == native.burial_letters and "".join(r[9] for r in mine) == model.burial_letters
    assert [r[1:4] for r in mine[:2]] == [["A", "1", "MET"], ["A", "2", "GLN"]] and [r[10:] for r in mine[:2]] == [["A", "1"], ["A", "2"]]
    assert analyse_models.pearson([1.0], [1.0]) != analyse_models.pearson([1.0], [1.0]) and analyse_models.pearson([1.0, 2.0], [2.0, 4.0]) == 1.0
