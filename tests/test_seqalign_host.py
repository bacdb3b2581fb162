"""Sequence alignment without a GPU: the restatement (tests/seqalign_restatement.py) against the committed fixture, against the figures
the rule was first run at, its two fills against one another and on cases small enough to check by hand; the ABI's argument checks, which
all happen before any device call; the header prototype, the ctypes entry and the build list; the Python layer's name -> code mapping,
byte budget and argument checks; analyse_models.py --seqalign / --pair_by_seqalign with the kernel calls replaced by restatements."""
import csv
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqalign_restatement as ar  # noqa: E402
from test_superpose_host import restated_arrays as restated_superpose  # noqa: E402
from timed_hip import _lib, analysis, pdbio, seqalign, seqset, superpose  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return ar.cases()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_restatement_reproduces_the_fixture_and_the_figures_of_the_rule(cases):
    assert os.path.getsize(ar.GOLDEN) < 128 * 1024
    golden = np.load(ar.GOLDEN)
    plain, rows = ar.golden_arrays(ar.restate_plain), ar.golden_arrays(ar.restate)
    assert sorted(golden.files) == sorted(plain) == sorted(rows)
    for key in golden.files:
        assert same_bytes(golden[key], np.asarray(plain[key])), key
        assert same_bytes(golden[key], np.asarray(rows[key])), key            # the row-at-a-time fill is the same rule
    text = open(os.path.join(ROOT, "tests", "golden", "make_seqalign_golden.py")).read()
    assert "NOT by the kernel" in text and ar.PHRASE in text
    assert same_bytes(ar.default_matrix(), seqalign.default_matrix()) and ar.default_matrix()[0, 0] == 8 and ar.default_matrix()[20, 3] == -2
    # the figures the rule was first run at: scores with free and with charged ends, and how many of the 76 residues are aligned
    for name, (free, charged, aligned) in ar.TABLE.items():
        a, b = golden[f"{name}_blosum_free_counts"].tolist(), golden[f"{name}_blosum_global_counts"].tolist()
        assert (a[2], b[2], a[3], b[3]) == (free, charged, aligned, aligned), (name, a, b)
        assert a[3] == a[4] == a[5]                                               # every aligned pair is an identity
    # ... and the alignments themselves
    assert golden["self_blosum_free_align"].tolist() == list(range(76))
    assert golden["deletion_blosum_free_align"].tolist() == list(range(22)) + [-1] * 6 + list(range(22, 70))
    assert golden["deletion_blosum_free_counts"].tolist()[6:] == [1, 6]
    assert golden["insertion_blosum_global_align"].tolist() == list(range(33)) + list(range(43, 86))
    assert golden["insertion_blosum_free_counts"].tolist()[6:] == [1, 10]
    assert golden["tag_blosum_free_align"].tolist() == list(range(10, 86)) == golden["tag_blosum_global_align"].tolist()
    assert golden["fragment_blosum_free_align"].tolist() == [-1] * 20 + list(range(40)) + [-1] * 16
    assert golden["tag_blosum_global_counts"].tolist()[6:] == [0, 0]              # an end run is charged but is no inner gap
    # a run before the first aligned pair is on the path with free ends too: 30 identities less the five W
    a, b = cases["overhangs"]
    got = ar.restate_plain(a, b)
    assert got["stop"] == (10, 0) and got["align"].tolist() == [-1] * 10 + list(range(5, 35)) and got["counts"].tolist()[6:] == [0, 0]
    assert got["counts"][2] == sum(int(ar.default_matrix()[c, c]) for c in a[10:]) - 24
    # ties: only the order of the rule decides
    assert golden["poly_a_blosum_free_align"].tolist() == [4, 5, 6, 7, 8] and golden["poly_a_swapped_blosum_free_align"].tolist() == [-1] * 4 + [0, 1, 2, 3, 4]
    assert golden["poly_a_blosum_global_align"].tolist() == [4, 5, 6, 7, 8] and golden["poly_a_blosum_global_counts"][2] == 5 * 8 - 23
    # the edges
    assert golden["empty_both_blosum_global_counts"].tolist() == [0] * 8 and golden["empty_reference_blosum_free_counts"].tolist() == [0, 7, 0, 0, 0, 0, 0, 0]
    assert golden["empty_reference_blosum_global_counts"].tolist() == [0, 7, -26, 0, 0, 0, 0, 0]
    assert golden["empty_model_identity_global_counts"].tolist() == [7, 0, -9, 0, 0, 0, 0, 0] and (golden["empty_model_identity_global_align"] == -1).all()
    assert golden["one_one_same_blosum_free_counts"].tolist() == [1, 1, 22, 1, 1, 1, 0, 0]
    assert golden["one_one_other_blosum_free_counts"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]          # W against P is -8: nothing aligned is better
    assert golden["one_one_other_blosum_global_counts"].tolist() == [1, 1, -8, 1, 0, 0, 0, 0]
    assert golden["all_unknown_blosum_global_counts"].tolist()[2:6] == [9 * -2 - 23, 9, 9, 0]       # code 20 equals code 20, and scores -2
    # the table really is an input
    assert not same_bytes(golden["mutated_50_blosum_free_align"], golden["mutated_50_identity_free_align"])
    assert golden["self_identity_global_counts"].tolist()[2] == 76


def test_tiny_cases_checked_by_hand():
    S = ar.identity_matrix()
    a, b = ar.encode("ACDE"), ar.encode("ACE")
    H, E, F, origin, e_ext, f_ext = ar.tables_plain(a.tolist(), b.tolist(), S.tolist(), 3, 1, 0)
    assert H[0] == [0, -3, -4, -5] and [row[0] for row in H] == [0, -3, -4, -5, -6] and E[0][2] == -4 and F[2][0] == -4 and E[2][0] == ar.NEG
    assert H[1][1] == 1 and H[2][2] == 2 and H[3][2] == -1 and F[3][2] == -1 and origin[3][2] == 1 and H[4][3] == 0
    got = ar.restate_plain(a, b, S, 3, 1, 0)
    assert got["align"].tolist() == [0, 1, -1, 2] and got["counts"].tolist() == [4, 3, 0, 3, 3, 3, 1, 1]
    # free ends: E at the end costs nothing, so ACDE against AC stops in the last column
    free = ar.restate_plain(a, ar.encode("AC"), S, 3, 1, 1)
    assert free["end"] == (2, 2) and free["align"].tolist() == [0, 1, -1, -1] and free["counts"][2] == 2
    # a gap of two in the model and one of three in the reference: two runs, five residues; extended bits carry the trace through them
    a, b = ar.encode("AAAACCGGGG"), ar.encode("AAAAWWWGGGG")
    got = ar.restate_plain(a, b, S, 1, 0, 0)                                    # two runs cost 2, two mismatches and a run would cost 3
    assert got["align"].tolist() == [0, 1, 2, 3, -1, -1, 7, 8, 9, 10] and got["counts"].tolist() == [10, 11, 6, 8, 8, 8, 2, 5]
    assert ar.cost(0, 20, 1) == 0 and ar.cost(1, 20, 1) == 20 and ar.cost(6, 20, 1) == 25


def fresh():
    return dict(align=np.full(4097, 12345, np.int32), counts=np.full((2, 8), 12345, np.int64))


def abi_call(lib, device, out, good, **kw):
    def p(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    ref, ro, mob, mo, matrix = good
    args = dict(ref=ref, ref_total=len(ref), ro=ro, mob=mob, mob_total=len(mob), mo=mo, n_pairs=len(ro) - 1, matrix=matrix, gap_open=20, gap_extend=1,
                free_ends=1, align=out["align"], counts=out["counts"])
    args.update(kw)
    ms = (C.c_double * 2)(-1.0, -1.0)
    rc = lib.th_seqalign(device, p(args["ref"]), args["ref_total"], p(args["ro"]), p(args["mob"]), args["mob_total"], p(args["mo"]), args["n_pairs"],
                         p(args["matrix"]), args["gap_open"], args["gap_extend"], args["free_ends"], p(args["align"]), p(args["counts"]),
                         C.cast(ms, C.POINTER(C.c_double)))
    return rc, list(ms)


def bad_calls(ref, ro, mob, mo, matrix):
    """every refusal of the ABI, as replaced arguments of a good two-pair call"""
    nr, nm = len(ref), len(mob)
    long_one, one = np.zeros(4097, np.uint8), np.array([0, 4097], np.int64)
    too_high, too_low, bad_ref, bad_mob = matrix.copy(), matrix.copy(), ref.copy(), mob.copy()
    too_high[3, 4], too_low[20, 20], bad_ref[5], bad_mob[-1] = 128, -128, 21, 255
    return {
        "negative ref_total": dict(ref_total=-1), "negative mob_total": dict(mob_total=-1), "negative n_pairs": dict(n_pairs=-1),
        "ref_total too large": dict(ref_total=1 << 31), "n_pairs too large": dict(n_pairs=1 << 31), "ref NULL": dict(ref=None), "mob NULL": dict(mob=None),
        "ref_offsets NULL": dict(ro=None), "mob_offsets NULL": dict(mo=None), "matrix NULL": dict(matrix=None), "align NULL": dict(align=None),
        "counts NULL": dict(counts=None), "ref_offsets decrease": dict(ro=np.array([0, nr, nr - 1], np.int64), ref_total=nr - 1),
        "mob_offsets end before total": dict(mo=np.array([0, 3, nm - 1], np.int64)), "ref_offsets start late": dict(ro=np.array([1, 3, nr], np.int64)),
        "mob_offsets end past total": dict(mob_total=nm - 1), "no pairs but residues": dict(n_pairs=0),
        "gap_open below gap_extend": dict(gap_open=1, gap_extend=2), "gap_extend negative": dict(gap_extend=-1), "gap_open 32768": dict(gap_open=32768),
        "free_ends 2": dict(free_ends=2), "table entry 128": dict(matrix=too_high), "table entry -128": dict(matrix=too_low),
        "reference code 21": dict(ref=bad_ref), "model code 255": dict(mob=bad_mob),
        "4097 reference residues": dict(ref=long_one, ref_total=4097, ro=one, mo=np.array([0, nm], np.int64), n_pairs=1),
        "4097 model residues": dict(mob=long_one, mob_total=4097, mo=one, ro=np.array([0, nr], np.int64), n_pairs=1),
    }


def test_library_exports_th_seqalign_and_checks_arguments_without_a_gpu(lib, cases):
    ref, ro, mob, mo = ar.flatten([cases["deletion"], cases["one_many"]])
    matrix = ar.default_matrix()
    for what, change in bad_calls(ref, ro, mob, mo, matrix).items():
        out = fresh()
        rc, ms = abi_call(lib, 0, out, (ref, ro, mob, mo, matrix), **change)
        assert rc == _lib.TH_EINVAL, what
        assert b"th_seqalign" in lib.th_last_error(), what
        assert (out["align"] == 12345).all() and (out["counts"] == 12345).all() and ms == [-1.0, -1.0], what
    assert lib.th_seqalign(0, None, 0, None, None, 0, None, 0, None, 20, 1, 1, None, None, None) == _lib.TH_OK         # no pairs: no launch
    with pytest.raises(_lib.TimedHipError) as err:
        seqalign.seqalign_arrays(np.zeros(4097, np.uint8), [0, 4097], ref, [0, len(ref)])
    assert err.value.code == _lib.TH_EINVAL and "4096" in str(err.value)
    with pytest.raises(_lib.TimedHipError) as err:
        seqalign.seqalign_arrays(ref, ro, mob, mo, gap_open=0, gap_extend=1)
    assert err.value.code == _lib.TH_EINVAL and "gap_open" in str(err.value)


_CTYPES = {"int": "c_int", "int64_t": "c_long", "const uint8_t*": "c_void_p", "const int64_t*": "c_void_p", "const int32_t*": "c_void_p",
           "int32_t*": "c_void_p", "int64_t*": "c_void_p", "double*": ("c_void_p", "LP_c_double")}


def test_header_ctypes_build_list_and_the_unpinned_parity_phrase():
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    m = re.search(r"^(\w+) th_seqalign\(([^;]*)\);", header, re.M)
    assert m
    res, args = _lib.PROTOTYPES["th_seqalign"]
    assert res.__name__ == _CTYPES[m.group(1)]
    declared = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(2).split(",")]
    assert len(declared) == len(args) == 15, (declared, args)
    for c_type, ct in zip(declared, args):
        want = _CTYPES[c_type]
        assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (c_type, ct)
    before = header[:m.start()]
    section = before[before.rindex("/* ----"):]
    for phrase in (ar.PHRASE, "only if strictly greater", "#define TH_SEQALIGN_MAX_LENGTH 4096", "(n, j) for j = m - 1 .. 0", "before any device call",
                   "minus infinity\" = -2^30", "gap_open + (k - 1) gap_extend"):
        assert phrase in section, phrase
    import __graft_entry__
    assert "seqalign.hip" in __graft_entry__.HIP_SOURCES
    source = open(os.path.join(ROOT, "timed-design_amd", "csrc", "seqalign.hip")).read()
    assert ar.PHRASE in source and '#include "oneshot.h"' in source and "th_check_offsets(" in source
    code = "\n".join(line.split("//")[0] for line in source.splitlines())
    assert "atomic" not in code and "float" not in code and "double" not in code.replace("double* kernel_ms", "")
    for kernel in ("k_seqalign_fill", "k_seqalign_trace"):
        assert f"hipLaunchKernelGGL({kernel}" in source, kernel
    assert code.index("call.open(") > max(code.rindex("TH_FAIL("), code.rindex("th_check_offsets("))        # every check precedes the device
    import analyse_models
    text = re.sub(r"\s+", " ", analyse_models.build_parser().format_help())
    assert ar.PHRASE in text and "--seqalign" in text and "--pair_by_seqalign" in text and "--sa_global" in text and "4096" in text
    from design_utils import analyse_utils
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert ar.PHRASE in seqalign.__doc__ and ar.PHRASE in analyse_utils.align_sequences.__doc__ and "th_seqalign" in readme and "--pair_by_seqalign" in readme
    assert "th_seqalign" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_seqalign.py")) and os.path.exists(os.path.join(ROOT, "profiles", "seqalign.txt"))


def test_names_letters_costs_and_the_byte_budget():
    names = ["ALA", "CYS", "TYR", "MSE", "HOH", " gly", "UNK", ""]
    assert seqalign.codes_of_names(names).tolist() == [0, 1, 19, 20, 20, 5, 20, 20] and seqalign.codes_of_names([]).dtype == np.uint8
    assert seqalign.codes_of_string("ACDEFGHIKLMNPQRSTVWYXB-a").tolist() == list(range(20)) + [20, 20, 20, 0]
    assert same_bytes(seqalign.codes_of_string("MQIFVK"), seqset.encode(["MQIFVK"])[0]) and seqalign.UNKNOWN == 20
    table = seqalign.default_matrix()
    assert table.dtype == np.int32 and table.shape == (21, 21) and (table[:20, :20] == 2 * analysis.BLOSUM62).all()
    assert (table[20] == -2).all() and (table[:, 20] == -2).all() and (seqalign.GAP_OPEN, seqalign.GAP_EXTEND, seqalign.MAX_LENGTH) == (20, 1, 4096)
    # the trace bits: a dword per step and strip of 8 columns; 64 strips to a panel
    assert seqalign.trace_bytes(76, 76) == 4 * (76 + 9) * 10 and seqalign.trace_bytes(0, 9) == seqalign.trace_bytes(9, 0) == 0
    assert seqalign.trace_bytes(5, 512) == 4 * (5 + 63) * 64 and seqalign.trace_bytes(5, 513) == 4 * ((5 + 63) * 64 + 5)
    assert seqalign.trace_bytes(4096, 4096) == 4 * 8 * 4159 * 64
    assert seqalign.pair_bytes(76, 70) == seqalign.trace_bytes(76, 70) + 17 * 76 + 5 * 70 + 120 and seqalign.pair_bytes(0, 0) == 120
    for bad in (dict(gap_open=0.5), dict(gap_extend=-1), dict(gap_open=1, gap_extend=2), dict(gap_open=32768)):
        with pytest.raises(ValueError, match="gap_open"):
            seqalign.align_strings([], **bad)
        with pytest.raises(ValueError, match="gap_open"):
            seqalign.align([], **bad)
    with pytest.raises(ValueError, match="offsets"):
        seqalign.seqalign_arrays(np.zeros(1, np.uint8), [0, 1], np.zeros(1, np.uint8), [0, 1, 1])
    with pytest.raises(ValueError, match="matrix"):
        seqalign.seqalign_arrays(np.zeros(1, np.uint8), [0, 1], np.zeros(1, np.uint8), [0, 1], matrix=np.zeros((20, 20), np.int32))
    assert seqalign.align([]) == [] and seqalign.align_strings([]) == []


def layout(letters, first=1, chain="A"):
    from design_utils.amino_acids import standard_amino_acids
    return superpose.AtomLayout(np.arange(3.0 * len(letters)).reshape(-1, 3),
                                [pdbio.Residue(chain, str(first + k), standard_amino_acids.get(c, "UNK")) for k, c in enumerate(letters)])


def test_batches_long_structures_strings_and_prepare_aligned(monkeypatch):
    calls = []

    def counted(ref_codes, ref_offsets, *a, **kw):
        calls.append(len(ref_offsets) - 1)
        return ar.restated_arrays(ref_codes, ref_offsets, *a, **kw)
    monkeypatch.setattr(seqalign, "seqalign_arrays", counted)
    ubq = ar.ubq_sequence()
    pairs = [(layout(ubq[:40]), layout(ubq[k:k + 30], first=501)) for k in range(5)]
    one = seqalign.pair_bytes(40, 30)
    stats = {}
    whole = seqalign.align(pairs, stats=stats)
    assert calls == [5] and stats["submissions"] == 1 and stats["files_parsed"] == 0
    del calls[:]
    split = seqalign.align(pairs, budget_bytes=2 * one + one // 2)                # two pairs fit, three do not
    assert calls == [2, 2, 1]
    for k, (a, b) in enumerate(zip(whole, split)):
        want = ar.restate(ar.encode(ubq[:40]), ar.encode(ubq[k:k + 30]))
        assert a.error is None and [a.n_ref, a.n_model, a.score, a.n_aligned, a.n_identical, a.n_positive, a.n_gaps, a.n_gap_residues] == want["counts"].tolist()
        assert a.reference_index.tolist() == list(range(k, k + 30)) == b.reference_index.tolist() and a.model_index.tolist() == list(range(30))
        assert a.identity == 1.0 and a.coverage_ref == 30 / 40 and a.coverage_model == 1.0 and a.positives == 1.0
    # a structure above 4096 positions: its pair's error, and the neighbours are aligned
    giant = (layout("A" * 10), layout("G" * 4097))
    del calls[:]
    first, middle, last = seqalign.align([pairs[0], giant, pairs[1]])
    assert calls == [2] and "4097" in middle.error and "4096" in middle.error and middle.n_aligned == 0 and np.isnan(middle.identity)
    assert first.score == whole[0].score and last.score == whole[1].score
    # plain strings, an unknown letter among them
    del calls[:]
    (res, long_one) = seqalign.align_strings([("MQIFVKTLTGK", "QIFXKTL"), ("A" * 4097, "A")])
    assert calls == [1] and res.reference_index.tolist() == [1, 2, 3, 4, 5, 6, 7] and res.model_index.tolist() == list(range(7)) and "4097" in long_one.error
    assert (res.n_identical, res.n_positive, res.n_aligned) == (6, 6, 7)
    assert seqalign.gapped("MQIFVKTLTGK", "QIFXKTL", res) == ("MQIFVKTLTGK", "-QIFXKTL---")
    (gap,) = seqalign.align_strings([("AAAAWWWGGGG", "AAAACCGGGG")], matrix=ar.identity_matrix(), gap_open=1, gap_extend=0, free_ends=False)
    assert seqalign.gapped("AAAAWWWGGGG", "AAAACCGGGG", gap) in (("AAAAWWW--GGGG", "AAAA---CCGGGG"), ("AAAA--WWWGGGG", "AAAACC---GGGG")) and gap.n_gaps == 2
    from design_utils import analyse_utils
    assert analyse_utils.align_sequences("MQIFVKTLTGK", "QIFXKTL") == ("MQIFVKTLTGK", "-QIFXKTL---", res.score)
    # the alignment as a pairing, by hand-made results
    made = [seqalign.SeqalignResult(None, 40, 30, 1, 3, 3, 3, 0, 0, np.array([2, 3, 4]), np.array([0, 1, 2]), pairs[2][0], pairs[2][1]),
            seqalign._failed("no such file")]
    prepared = seqalign.prepare_aligned([pairs[2], giant], results=made)
    assert isinstance(prepared, superpose.Prepared) and prepared.pairs[1] == "no such file" and prepared.files == 0 and prepared.atom == "CA"
    ref, mod, ours, theirs = prepared.pairs[0]
    assert ref is pairs[2][0] and mod is pairs[2][1] and ours.tolist() == [2, 3, 4] and theirs.tolist() == [0, 1, 2]
    del calls[:]
    prepared = seqalign.prepare_aligned([pairs[2], giant])
    assert calls == [1] and isinstance(prepared.pairs[1], str) and (prepared.pairs[0][3] == prepared.pairs[0][2] - 2).all()
    monkeypatch.setattr(superpose, "superpose_arrays", restated_superpose)
    scored = superpose.superpose(prepared)
    assert scored[1].error and scored[0].error is None and scored[0].n_valid == 30 and (scored[0].unpaired_reference, scored[0].unpaired_model) == (10, 0)
    assert scored[0].sequence_identity == 1.0


def test_analyse_models_writes_the_seqalign_tables_and_pairs_by_them(tmp_path, monkeypatch, capsys):
    import analyse_models
    monkeypatch.setattr(superpose, "superpose_arrays", restated_superpose)
    monkeypatch.setattr(seqalign, "seqalign_arrays", ar.restated_arrays)
    protein = ar.write_ubq_files(tmp_path)
    parser = analyse_models.build_parser()
    native = ["--path_to_reference", str(tmp_path / "native.pdb")]
    common = native + ["--path_to_models", str(tmp_path / "models")]

    def read(folder, name):
        with open(tmp_path / folder / name, newline="") as f:
            return list(csv.reader(f))
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "plain")]))
    capsys.readouterr()
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "out"), "--seqalign"]))
    assert "3 pairs (1 with an error), 152 positions, 4 files parsed in 2 GPU submission(s)" in capsys.readouterr().out
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["model_scores.csv", "residue_deviation.csv"]
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["model_scores.csv", "model_seqalign.csv", "residue_deviation.csv", "residue_seqalign.csv"]
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (tmp_path / "out" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes()
    rows = read("out", "model_seqalign.csv")
    assert rows[0] == analyse_models.SEQALIGN_COLUMNS == ["label", "reference", "model", "n_ref", "n_model", "score", "n_aligned", "identity", "positives",
                                                          "n_gaps", "n_gap_residues", "coverage_ref", "coverage_model", "error"]
    assert [r[0] for r in rows[1:]] == ["copy.pdb", "deleted.pdb", "moved.pdb"]
    assert rows[1][3:] == ["76", "76", "762", "76", "1.0", "1.0", "0", "0", "1.0", "1.0", ""]
    assert rows[2][3:] == ["76", "70", "681", "70", "1.0", "1.0", "1", "6", repr(70 / 76), "1.0", ""]
    residues = read("out", "residue_seqalign.csv")
    assert residues[0] == analyse_models.RESIDUE_SEQALIGN_COLUMNS and len(residues) == 1 + 3 * 76
    mine = [r for r in residues[1:] if r[0] == "deleted.pdb"]
    assert [r[2] for r in mine if not r[5]] == [protein[k].number for k in range(22, 28)] and all(r[4:] == ["", "", ""] for r in mine if not r[5])
    assert all(r[3] == r[6] and r[2] == r[5] and r[4] == "A" for r in mine if r[5])               # the model kept the native's numbers
    copied = [r for r in residues[1:] if r[0] == "copy.pdb"]
    assert [r[5] for r in copied] == [str(101 + k) for k in range(76)]
    assert "length mismatch" in read("out", "model_scores.csv")[2][-1]
    # the alignment as the pairing: the deleted-loop model is scored over its 70 aligned residues
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "sa"), "--pair_by_seqalign"]))
    assert sorted(p.name for p in (tmp_path / "sa").iterdir()) == ["model_scores.csv", "residue_deviation.csv"]
    scores = read("sa", "model_scores.csv")
    row = dict(zip(scores[0], scores[2]))
    assert row["error"] == "" and row["n_valid"] == "70" and (row["unpaired_reference"], row["unpaired_model"]) == ("6", "0") and row["sequence_identity"] == "1.0"
    assert float(row["rmsd_fit_all"]) < 1e-9 and len(read("sa", "residue_deviation.csv")) == 1 + 76 + 70 + 76
    # on pairs of one sequence the self alignment is the identity: the same bytes as pairing by position
    same = native + ["--path_to_models", str(tmp_path / "same")]
    analyse_models.main(parser.parse_args(same + ["--path_to_output", str(tmp_path / "by_position"), "--pair_by", "position"]))
    analyse_models.main(parser.parse_args(same + ["--path_to_output", str(tmp_path / "by_sequence"), "--pair_by_seqalign"]))
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (tmp_path / "by_sequence" / name).read_bytes() == (tmp_path / "by_position" / name).read_bytes()
    # charged ends and other costs reach the call
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "global"), "--seqalign", "--sa_global", "--sa_gap_open", "5",
                                                    "--sa_gap_extend", "1.5"]))
    assert read("global", "model_seqalign.csv")[2][5] == str(762 - 56 - (10 + 5 * 3))
    for flags in (["--pair_by_seqalign", "--pair_by_cealign"], ["--seqalign", "--sa_gap_open", "10.25"], ["--seqalign", "--sa_gap_extend", "-0.5"],
                  ["--pair_by_seqalign", "--sa_gap_open", "1", "--sa_gap_extend", "2"], ["--seqalign", "--sa_gap_open", "20000"]):
        with pytest.raises(SystemExit):
            analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "bad")] + flags))
    assert not (tmp_path / "bad").exists()
    args = parser.parse_args(["--pairs", "p.csv"])
    assert not any(hasattr(args, flag) for flag in ("seqalign", "pair_by_seqalign", "sa_gap_open", "sa_gap_extend", "sa_global"))
    capsys.readouterr()
