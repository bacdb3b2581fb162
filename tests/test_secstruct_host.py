"""Secondary structure without a GPU: the NumPy restatement (tests/secstruct_restatement.py) against the committed fixture and the
strings of the rule's write-up; the header prototype, the ctypes entry, the build list and the unpinned-parity phrase; every refusal of
th_secondary_structure; the layout, three_state and the byte budget; analyse_properties.py and analyse_models.py --secondary_structure
with the kernel call replaced by the restatement; the pairing of entropy rows with residues."""
import csv
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import secstruct_restatement as ss  # noqa: E402
import superpose_restatement as sr  # noqa: E402
from timed_hip import _lib, pdbio, secstruct, structure, superpose  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHRASE = "PARITY UNPINNED AGAINST DSSP"


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restated_arrays(backbone, chain, no_h, offsets, device=0, bits=False, timing=None):
    """secstruct.secondary_structure_arrays with the GPU call replaced by the restatement"""
    cls, residue, totals, words = ss.restate_batch(np.asarray(backbone, np.float64).reshape(-1, 4, 3), np.asarray(chain), np.asarray(no_h), offsets)
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0)
    return secstruct.SecondaryTables(cls, residue, totals, words if bits else None)


def restated_superposition(ref_xyz, mob_xyz, offsets, cycles=5, cutoff=2.0, device=0, transform=False, timing=None):
    dist, kept, rmsd, counts, moves, _, _ = sr.restate_batch(ref_xyz, mob_xyz, np.asarray(offsets), cycles, cutoff)
    return superpose.Superposed(dist, kept, rmsd, counts, moves.reshape(-1, 3, 4) if transform else None)


def test_restatement_equals_the_fixture_and_the_written_strings():
    assert os.path.getsize(ss.GOLDEN) < 64 * 1024
    golden = np.load(ss.GOLDEN)
    inputs = ss.cases()
    again = ss.golden_arrays(inputs)
    assert golden["cases"].tolist() == list(ss.CASES) and sorted(golden.files) == sorted(again)
    for key in golden.files:
        assert same_bytes(golden[key], np.asarray(again[key])), key
    text = open(os.path.join(ROOT, "tests", "golden", "make_secstruct_golden.py")).read()
    assert "NOT by the kernel" in text and PHRASE in text
    for name in ss.CASES:
        got = ss.as_string(golden[f"{name}_cls"])
        print(name, golden[f"{name}_totals"].tolist(), got)
        assert got == ss.STRINGS[name], name
        assert golden[f"{name}_cls"].dtype == np.uint8 and golden[f"{name}_residue"].dtype == np.int32 and golden[f"{name}_bits"].dtype == np.uint64
    # the strings of the write-up, spelled out here once more
    assert ss.STRINGS["ubq"] == "-EEEEEETTS-EEEEE--TTSBHHHHHHHHHHHH---GGGEEEEETTEE--TTSBTGGGT--TT-EEEEEE--S--"
    assert ss.STRINGS["alpha"] == "-HHHHHHHHHHHHHHHHHH-" and ss.STRINGS["three10"] == "-GGGGGGGGGG-" and ss.STRINGS["pi"] == "-IIIIIIIIIIII-"
    assert ss.STRINGS["beta"] == "-" * 12 and ss.STRINGS["two_chains"] == "-HHHHHHHH--HHHHHHHH-" and ss.STRINGS["missing_o"] == "-HHHHH---HHHHHHHHHH-"
    assert "SBHHHHHHH--GGGEEEEE" in ss.STRINGS["ubq_cut"] and len(ss.STRINGS["ubq_cut"]) == 70          # the helix ends at the cut
    ubq = ss.restate(*inputs["ubq"])
    assert ubq["totals"].tolist() == [76, 54, 16, 12, 2, 24, 6, 0, 12, 4] and int(ubq["hb"].sum()) == 54
    # the tables are consistent with the bond matrix they come from
    hb = ubq["hb"]
    assert ubq["residue"][:, 3].tolist() == hb.sum(axis=1).tolist() and ubq["residue"][:, 4].tolist() == hb.sum(axis=0).tolist()
    bits = ubq["bits"].reshape(76, 2)
    assert all(bool((int(bits[a, d // 64]) >> (d % 64)) & 1) == bool(hb[a, d]) for a in range(76) for d in range(76))
    flags = ubq["residue"][:, 2]
    assert (flags & ss.F_VALID).all() and (flags[:75] & ss.F_CONN).all() and not flags[75] & ss.F_CONN
    # bridges are mutual, partners are sorted, and both kinds occur in ubiquitin's mixed sheet
    partners = ubq["residue"][:, :2]
    for i in range(76):
        for j in partners[i]:
            assert j < 0 or i in partners[j].tolist() or ubq["residue"][j, 5] > 2
        assert partners[i, 1] < 0 or partners[i, 0] < partners[i, 1]
    assert (flags & ss.F_PARALLEL).any() and (flags & ss.F_ANTIPARALLEL).any()
    assert ((ubq["cls"] == 2) | (ubq["cls"] == 3)).sum() == (ubq["residue"][:, 5] > 0).sum()
    # proline donates nothing; an empty structure is fine
    assert not ubq["residue"][inputs["ubq"][2].astype(bool), 4].any() and inputs["ubq"][2].sum() == 3
    empty = ss.restate(np.zeros((0, 4, 3)), np.zeros(0, np.int32), np.zeros(0, np.uint8))
    assert empty["totals"].tolist() == [0] * 10 and empty["bits"].shape == (0,)
    # a donor N exactly on an acceptor O: -9900, a bond, nothing non-finite
    two = np.concatenate([inputs["alpha"][0], inputs["alpha"][0]])
    two[20:] += two[5, 3] - two[32, 0]
    two[32, 0] = two[5, 3]
    on = ss.restate(two, np.array([0] * 20 + [1] * 20, np.int32), np.zeros(40, np.uint8))
    assert on["energy"][5, 32] == -9900 and on["hb"][5, 32] and on["energy"].min() == -9900


_CTYPES = {"int": "c_int", "int64_t": "c_long", "const double*": "c_void_p", "const int64_t*": "c_void_p", "const int32_t*": "c_void_p",
           "const uint8_t*": "c_void_p", "uint8_t*": "c_void_p", "int32_t*": "c_void_p", "int64_t*": "c_void_p", "uint64_t*": "c_void_p",
           "double*": ("c_void_p", "LP_c_double")}


def test_header_ctypes_build_list_and_the_unpinned_parity_phrase():
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    m = re.search(r"^(\w+) th_secondary_structure\(([^;]*)\);", header, re.M)
    assert m
    res, args = _lib.PROTOTYPES["th_secondary_structure"]
    assert res.__name__ == _CTYPES[m.group(1)]
    declared = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(2).split(",")]
    assert len(declared) == len(args) == 12, (declared, args)
    for c_type, ct in zip(declared, args):
        want = _CTYPES[c_type]
        assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (c_type, ct)
    before = header[:m.start()]
    block = before[before.rindex("/* ----"):]
    assert block.startswith("/* ---- ") and "*** " + PHRASE + " ***" in block
    flat = re.sub(r"[\s*]+", " ", block)
    for words in ("Kabsch & Sander 1983", "mkdssp", "no \"two best per residue\" cap", "Beta-bulges are NOT bridged over", "H > E > B > G > I > T > S",
                  "0.3420201433256688", "27.888", "no fused multiply-add", "<= 6.25", "< 81.0", "TH_ENOMEM", "row = acceptor"):
        assert words in flat, words
    import __graft_entry__
    assert "secstruct.hip" in __graft_entry__.HIP_SOURCES
    source = open(os.path.join(ROOT, "timed-design_amd", "csrc", "secstruct.hip")).read()
    assert PHRASE in source and "#pragma clang fp contract(off)" in source and "atomic" not in source.replace("No atomics", "")
    assert PHRASE in secstruct.__doc__ and "H > E > B > G > I > T > S" in secstruct.__doc__
    import analyse_models
    import analyse_properties
    for module in (analyse_models, analyse_properties):
        text = re.sub(r"\s+", " ", module.build_parser().format_help())
        assert PHRASE in text and "--secondary_structure" in text, module.__name__
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert PHRASE in readme and "th_secondary_structure" in readme and "th_secondary_structure" in design
    assert secstruct.LETTERS == ss.LETTERS == "-HBEGITS" and secstruct.THREE_STATE == ss.THREE
    assert (secstruct.FLAG_TURN3, secstruct.FLAG_BEND, secstruct.FLAG_PARALLEL, secstruct.FLAG_ANTIPARALLEL, secstruct.FLAG_CONN, secstruct.FLAG_VALID) == (
        ss.F_TURN3, ss.F_BEND, ss.F_PARALLEL, ss.F_ANTIPARALLEL, ss.F_CONN, ss.F_VALID) == (1, 8, 16, 32, 64, 128)


def test_library_exports_th_secondary_structure_and_checks_arguments_without_a_gpu(lib):
    backbone, chain, no_h = np.zeros((2, 4, 3)), np.zeros(2, np.int32), np.zeros(2, np.uint8)
    offsets = np.array([0, 2], np.int64)
    cls, residue, totals, bits = np.full(2, 77, np.uint8), np.full((2, 6), 77, np.int32), np.full((1, 10), 77, np.int64), np.full(2, 77, np.uint64)

    def call(bb=backbone, ch=chain, nh=no_h, total=2, off=offsets, n=1, c=cls, r=residue, t=totals, b=bits):
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)        # noqa: E731
        ms = (C.c_double * 3)(-1.0, -1.0, -1.0)
        rc = lib.th_secondary_structure(0, p(bb), p(ch), p(nh), total, p(off), n, p(c), p(r), p(t), p(b), C.cast(ms, C.POINTER(C.c_double)))
        assert rc == _lib.TH_OK or list(ms) == [-1.0] * 3
        return rc
    bad = {"negative total": dict(total=-1), "negative structures": dict(n=-1), "total too large": dict(total=1 << 31),
           "structures too large": dict(n=1 << 31), "offsets NULL": dict(off=None), "structure_out NULL": dict(t=None),
           "backbone NULL": dict(bb=None), "chain NULL": dict(ch=None), "no_h NULL": dict(nh=None), "class_out NULL": dict(c=None),
           "residue_out NULL": dict(r=None), "offsets end": dict(off=np.array([0, 3], np.int64)), "offsets start": dict(off=np.array([1, 2], np.int64)),
           "offsets decrease": dict(off=np.array([0, 2, 1], np.int64), n=2), "offsets end before total": dict(off=np.array([0, 1], np.int64)),
           "residues without a structure": dict(n=0)}
    for what, kw in bad.items():
        assert call(**kw) == _lib.TH_EINVAL, what
        assert b"th_secondary_structure" in lib.th_last_error(), what
    assert (cls == 77).all() and (residue == 77).all() and (totals == 77).all() and (bits == 77).all()
    ms = (C.c_double * 3)(-1.0, -1.0, -1.0)
    assert lib.th_secondary_structure(0, None, None, None, 0, None, 0, None, None, None, None, C.cast(ms, C.POINTER(C.c_double))) == _lib.TH_OK
    assert list(ms) == [0.0, 0.0, 0.0]                                           # no structures: no launch
    with pytest.raises(ValueError):
        secstruct.secondary_structure_arrays(backbone, chain[:1], no_h, offsets)
    with pytest.raises(ValueError):
        secstruct.secondary_structure_arrays(backbone, chain, no_h, [])
    with pytest.raises(_lib.TimedHipError) as err:
        secstruct.secondary_structure_arrays(backbone, chain, no_h, [0, 3])
    assert err.value.code == _lib.TH_EINVAL


def test_layout_three_state_strings_and_the_byte_budget(monkeypatch):
    model = structure.first_model(ss.UBQ)
    lay = secstruct.backbone_layout(model)
    backbone, chain, no_h = ss.ubq_backbone()
    assert same_bytes(lay.backbone, backbone) and same_bytes(lay.chain, chain) and same_bytes(lay.no_h, no_h) and len(lay.residues) == 76
    assert [r.name for r, p in zip(lay.residues, lay.no_h) if p] == ["PRO"] * 3 and not any(r.hetero for r in lay.residues)
    # chains in order of appearance, a chain that comes back continues its entry, a missing atom is NaN, hetero residues are left out
    res = [pdbio.Residue("B", "1", "GLY", {"N": np.zeros(3), "CA": np.ones(3), "C": np.ones(3), "O": np.ones(3)}),
           pdbio.Residue("A", "1", "PRO", {"N": np.zeros(3), "CA": np.ones(3), "C": np.ones(3)}),
           pdbio.Residue("B", "2", "ALA", {"CA": np.ones(3)}), pdbio.Residue("A", "9", "HOH", {"O": np.ones(3)}, hetero=True)]
    mixed = secstruct.backbone_layout(pdbio.Model(1, res))
    assert [(r.chain, r.number) for r in mixed.residues] == [("B", "1"), ("B", "2"), ("A", "1")] and mixed.chain.tolist() == [0, 0, 1]
    assert mixed.no_h.tolist() == [0, 0, 1] and np.isnan(mixed.backbone[2, 3]).all() and np.isnan(mixed.backbone[1, 0]).all() and np.isfinite(mixed.backbone[0]).all()
    assert [r.chain for r in secstruct.backbone_layout(pdbio.Model(1, res), all_chains=False).residues] == ["B", "B"]
    codes = np.arange(8, dtype=np.uint8)
    assert secstruct.three_state(codes).tolist() == [0, 1, 2, 2, 1, 1, 0, 0] and secstruct.three_state(codes).dtype == np.uint8
    assert secstruct.as_string(codes) == "-HBEGITS" and secstruct.as_string(codes, three=True) == "CHEEHHCC" and secstruct.as_string([]) == ""
    assert secstruct.state_fractions([2, 1, 1, 2, 1, 1, 1, 1]) == (0.3, 0.3, 0.4) and all(np.isnan(f) for f in secstruct.state_fractions([0] * 8))
    # the bitmap is counted in a structure's size: L * ceil(L / 64) words
    assert secstruct.bitmap_words([0, 1, 64, 65, 300, 4096]).tolist() == [0, 1, 64, 130, 1500, 262144]
    assert secstruct.structure_bytes(300) == 300 * secstruct._RESIDUE_BYTES + 1500 * 8 and secstruct._RESIDUE_BYTES == 126
    calls = []

    def counted(backbone, chain, no_h, offsets, *a, **kw):
        calls.append(len(offsets) - 1)
        return restated_arrays(backbone, chain, no_h, offsets, *a, **kw)
    monkeypatch.setattr(secstruct, "secondary_structure_arrays", counted)
    layouts = [secstruct.BackboneLayout(*ss.cases()["alpha"], [pdbio.Residue("A", str(k), "ALA") for k in range(20)])] * 5
    stats = {}
    whole = secstruct.secondary_structure_layouts(layouts)
    split = secstruct.secondary_structure_layouts(layouts, budget_bytes=2 * secstruct.structure_bytes(20) + 10, stats=stats)
    assert calls == [5, 2, 2, 1] and stats["submissions"] == 3
    for a, b in zip(whole, split):
        assert a.string == b.string == ss.STRINGS["alpha"] and a.n_hbonds == 16 and a.counts.tolist() == [2, 18, 0, 0, 0, 0, 0, 0] and a.error is None
    stats = {}
    one, missing, two = secstruct.secondary_structure([ss.UBQ, os.path.join(ROOT, "tests", "golden", "absent.pdb"), model], stats=stats)
    assert one.string == two.string == ss.UBQ_STRING and "absent.pdb" in missing.error and len(missing.cls) == 0 and stats["files_parsed"] == 2
    assert one.fractions == (18 / 76, 26 / 76, 32 / 76) and secstruct.secondary_structure([]) == []


def _write_ubq(path, numbers=None, drop=()):
    """1ubq's ATOM records (no water), optionally without some residue numbers"""
    import gzip
    with gzip.open(ss.UBQ, "rt") as f:
        lines = [line for line in f if line[:6] == "ATOM  " and int(line[22:26]) not in drop]
    path.write_text("".join(lines) + "END\n")


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_analyse_properties_writes_its_two_files_and_leaves_the_others(tmp_path, monkeypatch, capsys):
    import analyse_properties as ap
    monkeypatch.setattr(secstruct, "secondary_structure_arrays", restated_arrays)
    monkeypatch.setattr(structure, "contact_numbers", lambda xyz, offsets, radius=7.0, group=None, selected=None, n_groups=0, device=0, atoms=True,
                        timing=None: (np.zeros(len(xyz), np.int32), np.arange(n_groups, dtype=np.float64)))
    (tmp_path / "pdb").mkdir()
    _write_ubq(tmp_path / "pdb" / "ubq.pdb")
    _write_ubq(tmp_path / "pdb" / "cut.pdb", drop=range(31, 37))
    parser = ap.build_parser()
    common = ["--path_to_pdb", str(tmp_path / "pdb")]
    plain, out = tmp_path / "plain", tmp_path / "out"
    assert "secondary_structure" not in vars(parser.parse_args(common)) and parser.parse_args(common + ["--secondary_structure"]).secondary_structure is True
    ap.main(parser.parse_args(common + ["--path_to_output", str(plain)]))
    assert sorted(p.name for p in plain.iterdir()) == ["residue_properties.csv", "structure_properties.csv"]
    assert "in 1 GPU submission(s)" in capsys.readouterr().out
    ap.main(parser.parse_args(common + ["--path_to_output", str(out), "--secondary_structure"]))
    assert "in 2 GPU submission(s)" in capsys.readouterr().out
    assert sorted(p.name for p in out.iterdir()) == ["residue_properties.csv", "residue_secondary_structure.csv", "structure_properties.csv",
                                                    "structure_secondary_structure.csv"]
    for name in ("residue_properties.csv", "structure_properties.csv"):
        assert (out / name).read_bytes() == (plain / name).read_bytes()
    per, whole = _read(out / "residue_secondary_structure.csv"), _read(out / "structure_secondary_structure.csv")
    assert per[0] == ap.SECSTRUCT_RESIDUE_COLUMNS and whole[0] == ap.SECSTRUCT_COLUMNS and len(per) == 1 + 70 + 76
    assert [r[0] for r in whole[1:]] == ["cut.pdb", "ubq.pdb"]
    ubq = [r for r in per[1:] if r[0] == "ubq.pdb"]
    want = ss.restate(*ss.ubq_backbone())
    assert "".join(r[4] for r in ubq) == ss.UBQ_STRING and "".join(r[5] for r in ubq) == "".join(ss.THREE[c] for c in want["cls"])
    assert "".join(r[4] for r in per[1:71]) == ss.STRINGS["ubq_cut"]
    assert [r[1:4] for r in ubq[:2]] == [["A", "1", "MET"], ["A", "2", "GLN"]]
    assert [[r[6], r[7]] for r in ubq] == [[f"A:{j + 1}" if j >= 0 else "" for j in row] for row in want["residue"][:, :2].tolist()]
    assert [[int(r[8]), int(r[9])] for r in ubq] == want["residue"][:, 3:5].tolist()
    row = dict(zip(whole[0], whole[2]))
    assert [int(row[k]) for k in whole[0][1:11]] == [76, 54, 16, 12, 2, 24, 6, 0, 12, 4]
    assert [float(row[k]) for k in whole[0][11:]] == [18 / 76, 26 / 76, 32 / 76]
    assert int(whole[1][1]) == 70 and int(whole[1][2]) == int(np.load(ss.GOLDEN)["ubq_cut_totals"][1])


def test_entropy_rows_pair_with_residues_by_chain_and_number():
    import analyse_properties as ap
    lay = secstruct.backbone_layout(structure.first_model(ss.UBQ))
    want = ss.restate(lay.backbone, lay.chain, lay.no_h)
    rows = want["residue"]
    res = secstruct.StructureSecondary(None, want["cls"], rows[:, :2], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5], 76, 54, want["totals"][2:], lay.residues)
    states = secstruct.three_state(want["cls"])
    value = np.arange(76, dtype=np.float64) / 10.0
    means = [float(value[states == s].mean()) for s in (1, 2, 0)]
    # a two-column map: by position, and only when the counts agree
    assert ap.state_entropy("sub/1ubq.pdb1.gz", res, {"1ubq": value}, None) == means
    assert all(np.isnan(v) for v in ap.state_entropy("1ubq.pdb", res, {"1ubq": value[:75]}, None))
    assert all(np.isnan(v) for v in ap.state_entropy("other.pdb", res, {"1ubq": value}, None))
    # an old map: by chain and number, in any order, rows of residues the file lacks and of other files ignored
    order = np.random.default_rng(1).permutation(76)
    mine = [["1ubq", "A", str(k + 1), "ALA"] for k in order] + [["1ubq", "A", "999", "ALA"]]
    maps = {"1ubqA": mine, "2xyzA": [["2xyz", "A", "1", "GLY"]], "1ubqB": [["1ubq", "B", "1", "GLY"]]}
    entropy = {"1ubqA": np.concatenate([value[order], [100.0]]), "2xyzA": np.array([50.0]), "1ubqB": np.array([70.0])}
    assert ap.state_entropy("1ubq.pdb", res, entropy, maps) == means and ap.state_entropy("1ubqA.pdb", res, entropy, maps) == means
    helix_only = {"1ubqA": [["1ubq", "A", str(k + 1), "ALA"] for k in range(22, 34)]}
    got = ap.state_entropy("1ubq.pdb", res, {"1ubqA": value[22:34]}, helix_only)
    assert got[0] == float(value[22:34].mean()) and np.isnan(got[1]) and np.isnan(got[2])         # NaN where a state has no row


def test_analyse_models_writes_its_two_files_and_leaves_the_others(tmp_path, monkeypatch, capsys):
    import analyse_models
    calls = []

    def counted(backbone, chain, no_h, offsets, *a, **kw):
        calls.append(len(offsets) - 1)
        return restated_arrays(backbone, chain, no_h, offsets, *a, **kw)
    monkeypatch.setattr(superpose, "superpose_arrays", restated_superposition)
    monkeypatch.setattr(secstruct, "secondary_structure_arrays", counted)
    (tmp_path / "models").mkdir()
    _write_ubq(tmp_path / "native.pdb")
    _write_ubq(tmp_path / "models" / "same.pdb")
    _write_ubq(tmp_path / "models" / "cut.pdb", drop=range(31, 37))
    noisy = pdbio.read_pdb(tmp_path / "native.pdb")[0]
    rng = np.random.default_rng(4)
    for r in noisy.residues:
        for name in r.atoms:
            r.atoms[name] = r.atoms[name] + rng.normal(0.0, 0.6, 3)
    pdbio.write_pdb(tmp_path / "models" / "noisy.pdb", noisy)
    parser = analyse_models.build_parser()
    common = ["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models", str(tmp_path / "models")]
    plain, out, numbered = tmp_path / "plain", tmp_path / "out", tmp_path / "numbered"
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(plain)]))
    assert sorted(p.name for p in plain.iterdir()) == ["model_scores.csv", "residue_deviation.csv"] and calls == []
    capsys.readouterr()
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(out), "--secondary_structure"]))
    assert calls == [3]                                  # the native once, the two models that pair with it: one batch of three
    assert "4 files parsed in 2 GPU submission(s)" in capsys.readouterr().out
    assert sorted(p.name for p in out.iterdir()) == ["model_scores.csv", "model_secstruct.csv", "residue_deviation.csv", "residue_secstruct.csv"]
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (out / name).read_bytes() == (plain / name).read_bytes()
    scores, per = _read(out / "model_secstruct.csv"), _read(out / "residue_secstruct.csv")
    assert scores[0] == analyse_models.SECSTRUCT_COLUMNS and per[0] == analyse_models.RESIDUE_SECSTRUCT_COLUMNS
    assert [r[0] for r in scores[1:]] == ["cut.pdb", "noisy.pdb", "same.pdb"] and len(per) == 1 + 2 * 76
    cut, noise, same = (dict(zip(scores[0], r)) for r in scores[1:])
    assert "length mismatch" in cut["error"] and cut["n_paired"] == "0" and cut["q8"] == "nan"
    assert (same["n_paired"], same["q8"], same["q3"], same["error"]) == ("76", "1.0", "1.0", "") and same["reference_n_hbonds"] == same["model_n_hbonds"] == "54"
    assert [float(same[k]) for k in scores[0][6:10]] == [18 / 76, 26 / 76] * 2
    native = ss.restate(*ss.ubq_backbone())
    lay = secstruct.backbone_layout(structure.first_model(tmp_path / "models" / "noisy.pdb"))
    model = ss.restate(lay.backbone, lay.chain, lay.no_h)
    q8 = float((native["cls"] == model["cls"]).mean())
    q3 = float((secstruct.three_state(native["cls"]) == secstruct.three_state(model["cls"])).mean())
    assert float(noise["q8"]) == q8 and float(noise["q3"]) == q3 and q8 < q3 < 1.0 and int(noise["model_n_hbonds"]) == model["totals"][1] != 54
    mine = [r for r in per[1:] if r[0] == "noisy.pdb"]
    assert "".join(r[4] for r in mine) == ss.UBQ_STRING and "".join(r[5] for r in mine) == ss.as_string(model["cls"])
    assert [r[1:4] for r in mine[:2]] == [["A", "1", "MET"], ["A", "2", "GLN"]] and [r[8:] for r in mine[:2]] == [["A", "1"], ["A", "2"]]
    # --pair_by number: only the pairing indices change; the cut model pairs 70 residues and keeps its own assignment
    del calls[:]
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(numbered), "--secondary_structure", "--pair_by", "number"]))
    scores, per = _read(numbered / "model_secstruct.csv"), _read(numbered / "residue_secstruct.csv")
    cut = dict(zip(scores[0], scores[1]))
    keep = np.r_[0:30, 36:76]
    cut_cls = np.load(ss.GOLDEN)["ubq_cut_cls"]
    assert calls == [4] and cut["error"] == "" and cut["n_paired"] == "70" and float(cut["q8"]) == float((native["cls"][keep] == cut_cls).mean())
    mine = [r for r in per[1:] if r[0] == "cut.pdb"]
    assert [r[2] for r in mine] == [str(k + 1) for k in keep] == [r[9] for r in mine] and "".join(r[5] for r in mine) == ss.STRINGS["ubq_cut"]
    assert parser.parse_args(["--pairs", "p.csv"]).secondary_structure is False
