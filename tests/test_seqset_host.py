"""Diversity and native recovery of sampled sequences without a GPU: the NumPy restatement (tests/seqset_restatement.py) against the
committed fixture and against the reference's two formulas restated literally; the header prototype, the ctypes entry, the build list
and the own-rule phrase; every refusal of th_seqset; encode, both readers of sample.py's files, the per-mille threshold, the byte
budget with the matrix counted and the parser's defaults; analyse() and analyse_samples.py with the kernel call replaced by the
restatement."""
import csv
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqset_restatement as qr  # noqa: E402
from timed_hip import _lib, analysis, batching, seqset  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHRASE = qr.PHRASE


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restated_arrays(codes, seq_offsets, lengths, native=None, min_matches=None, substitution=None, matrix=False, device=0, timing=None):
    """seqset.seqset_arrays with the GPU call replaced by the restatement"""
    seq, profile, sets, squares = [], [], [], []
    at_code = at_pos = 0
    for k, length in enumerate(np.asarray(lengths).tolist()):
        n = int(seq_offsets[k + 1] - seq_offsets[k])
        got = qr.restate(np.asarray(codes[at_code:at_code + n * length]).reshape(n, length), None if native is None else native[at_pos:at_pos + length],
                         None if min_matches is None else int(min_matches[k]))
        seq.append(got["seq"])
        profile.append(got["profile"])
        sets.append(got["set"])
        squares.append(got["matrix"].reshape(-1))
        at_code += n * length
        at_pos += length
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0)
    return seqset.SeqsetTables(np.concatenate(seq), np.concatenate(profile), np.array(sets, np.int64).reshape(-1, 4), np.concatenate(squares) if matrix else None)


@pytest.fixture(scope="module")
def golden():
    return np.load(qr.GOLDEN)


def test_restatement_equals_the_fixture_and_the_written_numbers(golden):
    assert os.path.getsize(qr.GOLDEN) < 256 * 1024
    again = qr.golden_arrays()
    assert golden["cases"].tolist() == list(qr.CASES) and sorted(golden.files) == sorted(again)
    for key in golden.files:
        assert same_bytes(golden[key], np.asarray(again[key])), key
    text = open(os.path.join(ROOT, "tests", "golden", "make_seqset_golden.py")).read()
    assert "NOT by the kernel" in text and PHRASE in text
    shapes = {name: golden[f"{name}_codes"].shape for name in qr.CASES}
    assert shapes == dict(ubq_drift=(70, 76), ubq_drift_07=(70, 76), two_tiles=(130, 9), long=(3, 1030), single=(1, 5), empty=(0, 4), all_same=(66, 4))
    assert seqset.decode(golden["ubq_drift_native"]).startswith("MQIFVKTLTGK") and golden["two_tiles_native"].size == 0
    for name in qr.CASES:
        seq, profile, totals, square = (golden[f"{name}_{table}"] for table in qr.TABLES)
        n, length = shapes[name]
        assert seq.dtype == np.int32 and profile.dtype == np.int32 and totals.dtype == np.int64 and square.dtype == np.int32
        assert seq.shape == (n, 8) and profile.shape == (length, 21) and square.shape == (n, n)
        assert (profile.sum(axis=1) == n).all() and np.array_equal(square, square.T) and (np.diag(square) == length).all()
        assert (seq[:, 6] <= np.arange(n)).all() and totals[1] == (seq[:, 6] == np.arange(n)).sum() and totals[0] * 2 == seq[:, 3].sum()
        assert (seq[:, 7] <= np.arange(n)).all() and totals[2] == (seq[:, 7] == np.arange(n)).sum()
    # the written numbers
    drift, drift_07 = golden["ubq_drift_seq"], golden["ubq_drift_07_seq"]
    assert golden["ubq_drift_min_matches"] == 61 and golden["ubq_drift_07_min_matches"] == 54 and golden["two_tiles_min_matches"] == 9
    assert golden["ubq_drift_set"][1] == 68 and 1 < golden["ubq_drift_07_set"][2] < golden["ubq_drift_set"][2] < 70
    assert same_bytes(drift[:, :7], drift_07[:, :7]) and drift[[2, 5, 69], 6].tolist() == [2, 2, 2] and drift[[5, 69], 7].tolist() == [2, 2]
    assert drift[2, 4:6].tolist() == [76, 5] and drift[5, 4:6].tolist() == [76, 2] and drift[69, 4:6].tolist() == [76, 2]
    two = golden["two_tiles_seq"]
    assert not two[:, :3].any() and two[[0, 3, 127], 6].tolist() == [0, 0, 0] and two[0, 4:6].tolist() == [9, 3] and two[127, 5] == 0
    ties = sum(1 for i in range(130) if (np.delete(golden["two_tiles_matrix"][i], i) == two[i, 4]).sum() > 1)
    assert ties > 65                                                                        # ties for the lowest index abound
    assert golden["single_seq"].tolist() == [[3, 2, 5 + 0 + 7, 0, -1, -1, 0, 0]] and golden["single_set"].tolist() == [0, 1, 1, 3]
    assert golden["empty_set"].tolist() == [0, 0, 0, 0] and not golden["empty_profile"].any()
    same = golden["all_same_seq"]
    assert (same[:, 6] == 0).all() and (same[:, 7] == 0).all() and same[0, 4:6].tolist() == [4, 1] and same[1, 4:6].tolist() == [4, 0]
    assert golden["all_same_set"].tolist() == [66 * 65 // 2 * 4, 1, 1, 66 * 3] and (golden["long_codes"] == 20).sum() > 50 and (golden["long_native"] == 20).sum() > 20
    # no clustering: -1 everywhere
    bare = qr.restate(golden["single_codes"])
    assert bare["seq"][0, 7] == -1 and bare["set"][2] == -1 and not bare["seq"][:, :3].any()


def test_restatement_equals_the_two_formulas_of_the_reference(golden):
    """ui.py: accuracy_score(list(seq), list(native)) = mean(a == b); _calculate_sequence_similarity_wrapper = mean(1 if
    lookup_blosum62(a, b) > 0 else 0), here over the positions where the lookup is defined: both letters known"""
    from design_utils.utils import lookup_blosum62
    for name in ("ubq_drift", "long"):
        codes, native, seq = golden[f"{name}_codes"], golden[f"{name}_native"], golden[f"{name}_seq"]
        real = seqset.decode(native)
        for i, row in enumerate(codes):
            predicted = seqset.decode(row)
            identity = float(np.mean([a == b for a, b in zip(real, predicted)]))
            known = [(a, b) for a, b in zip(real, predicted) if a != "X" and b != "X"]
            similarity = float(np.mean([1 if lookup_blosum62(a, b) > 0 else 0 for a, b in known]))
            assert seq[i, 0] / codes.shape[1] == identity and seq[i, 1] / len(known) == similarity, (name, i)
            assert seq[i, 2] == sum(lookup_blosum62(a, b) for a, b in known)
    assert (golden["long_codes"] == 20).any() and lookup_blosum62("W", "W") == 11 and lookup_blosum62("A", "S") == lookup_blosum62("S", "A") == 1
    with pytest.raises(KeyError):
        lookup_blosum62("A", "X")


_CTYPES = {"int": "c_int", "int64_t": "c_long", "const uint8_t*": "c_void_p", "const int8_t*": "c_void_p", "const int64_t*": "c_void_p",
           "const int32_t*": "c_void_p", "int32_t*": "c_void_p", "int64_t*": "c_void_p", "double*": ("c_void_p", "LP_c_double")}


def test_header_ctypes_build_list_and_the_own_rule_phrase():
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    for name, count in (("th_seqset", 14), ("th_seqset_tiles", 1)):
        m = re.search(r"^(\w+) %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        res, args = _lib.PROTOTYPES[name]
        assert res.__name__ == _CTYPES[m.group(1)]
        declared = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(2).split(",")]
        assert len(declared) == len(args) == count, (declared, args)
        for c_type, ct in zip(declared, args):
            want = _CTYPES[c_type]
            assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (name, c_type, ct)
    before = header[:re.search(r"^int th_seqset\(", header, re.M).start()]
    block = before[before.rindex("/* ----"):]
    flat = re.sub(r"[\s*]+", " ", block)
    assert block.startswith("/* ---- ") and PHRASE in flat
    for words in ("ACDEFGHIKLMNPQRSTVWY", "code 20 equals code 20", "lowest j != i attaining it", "first_equal <= i", "greedy, in input order",
                  "lowest-indexed representative r < n", "CD-HIT-like tools", "no word filter, no length sorting and no alignment", "ceil(p L / 1000)",
                  "no atomics", "2^31 - 1", "set s at offset sum_{t<s} N_t^2", "native without substitution", "n_sets = 0 with nothing else is TH_OK",
                  "wherever it sits in a batch and whether or not the matrix is asked for"):
        assert words in flat, words
    import __graft_entry__
    assert "seqset.hip" in __graft_entry__.HIP_SOURCES
    source = open(os.path.join(ROOT, "timed-design_amd", "csrc", "seqset.hip")).read()
    assert PHRASE in source and "atomic" not in source.replace("no atomics", "") and "TH_SEQSET_PACKED" in source and "0x7f7f7f7f" in source
    assert "ThLayout" in source and "ThCall" in source and "th_check_offsets" in source and "th_tile_items" in source
    for kernel in ("k_seqset_pairs", "k_seqset_columns", "k_seqset_native", "k_seqset_cluster", "k_seqset_totals"):
        assert re.search(r"__global__ void __launch_bounds__\(k\w*Threads\) " + kernel, source), kernel
    assert PHRASE in re.sub(r"\s+", " ", seqset.__doc__)
    import analyse_samples
    assert PHRASE in re.sub(r"\s+", " ", analyse_samples.build_parser().format_help())
    readme = re.sub(r"\s+", " ", open(os.path.join(ROOT, "README.md")).read())
    design = re.sub(r"\s+", " ", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert PHRASE in readme and "th_seqset" in readme and "analyse_samples.py" in readme and "profiles/seqset.txt" in readme
    assert PHRASE in design and "th_seqset" in design
    from design_utils import utils
    assert "BLOSUM lookup" not in utils.__doc__ and "lookup_blosum62" in utils.__doc__


def test_library_exports_th_seqset_and_checks_arguments_without_a_gpu(lib):
    assert seqset.tiles() == (64, 64, 256)
    assert lib.th_seqset_tiles(None) == _lib.TH_EINVAL and b"th_seqset_tiles" in lib.th_last_error()
    codes, offsets, lengths = np.array([0, 1, 2, 20, 19, 5], np.uint8), np.array([0, 2], np.int64), np.array([3], np.int32)
    native, table, thresholds = np.array([0, 20, 2], np.uint8), np.ascontiguousarray(analysis.BLOSUM62).reshape(-1), np.array([3], np.int32)
    seq, profile, square, sets = np.full((2, 8), 77, np.int32), np.full((3, 21), 77, np.int32), np.full(4, 77, np.int32), np.full((1, 4), 77, np.int64)
    many = np.zeros(50000, np.uint8)

    def call(c=codes, total=6, off=offsets, l=lengths, n=1, nat=native, sub=table, thr=thresholds, s=seq, p=profile, m=square, t=sets):
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
        ms = (C.c_double * 3)(-1.0, -1.0, -1.0)
        rc = lib.th_seqset(0, ptr(c), total, ptr(off), ptr(l), n, ptr(nat), ptr(sub), ptr(thr), ptr(s), ptr(p), ptr(m), ptr(t), C.cast(ms, C.POINTER(C.c_double)))
        assert rc == _lib.TH_OK or list(ms) == [-1.0] * 3
        return rc
    bad_code, bad_native = codes.copy(), native.copy()
    bad_code[4], bad_native[2] = 21, 255
    bad = {"negative total": dict(total=-1), "negative sets": dict(n=-1), "too many sets": dict(n=1 << 31), "total too small": dict(total=5),
           "total too large": dict(total=7), "length 0": dict(l=np.array([0], np.int32)), "negative length": dict(l=np.array([-3], np.int32)),
           "N L above 2^31 - 1": dict(off=np.array([0, 1 << 20], np.int64), l=np.array([1 << 12], np.int32), total=1 << 32),
           "sequences above 2^31 - 1": dict(off=np.array([0, 1 << 31], np.int64)), "negative sequences": dict(off=np.array([0, -2], np.int64)),
           "matrix above 2^31 - 1": dict(c=many, total=50000, off=np.array([0, 50000], np.int64), l=np.array([1], np.int32), thr=np.array([1], np.int32)),
           "a code above 20": dict(c=bad_code), "a native code above 20": dict(nat=bad_native), "min_matches negative": dict(thr=np.array([-1], np.int32)),
           "min_matches above L": dict(thr=np.array([4], np.int32)), "codes NULL": dict(c=None), "seq_offsets NULL": dict(off=None),
           "lengths NULL": dict(l=None), "seq_out NULL": dict(s=None), "profile_out NULL": dict(p=None), "set_out NULL": dict(t=None),
           "native without substitution": dict(sub=None), "offsets start": dict(off=np.array([1, 2], np.int64)),
           "offsets decrease": dict(off=np.array([0, 3, 2], np.int64), l=np.array([3, 3], np.int32), n=2), "residues without a set": dict(n=0)}
    for what, kw in bad.items():
        assert call(**kw) == _lib.TH_EINVAL, what
        assert b"th_seqset:" in lib.th_last_error(), (what, lib.th_last_error())
    assert call(c=bad_code) == _lib.TH_EINVAL and b"codes[4]" in lib.th_last_error()
    assert call(nat=bad_native) == _lib.TH_EINVAL and b"native[2]" in lib.th_last_error()
    assert call(thr=np.array([4], np.int32)) == _lib.TH_EINVAL and b"min_matches[0]" in lib.th_last_error()
    assert (seq == 77).all() and (profile == 77).all() and (square == 77).all() and (sets == 77).all()
    ms = (C.c_double * 3)(-1.0, -1.0, -1.0)
    assert lib.th_seqset(0, None, 0, None, None, 0, None, None, None, None, None, None, None, C.cast(ms, C.POINTER(C.c_double))) == _lib.TH_OK
    assert list(ms) == [0.0, 0.0, 0.0]
    for bad_arguments in (dict(seq_offsets=[0, 2, 3]), dict(native=native[:2]), dict(min_matches=[1, 2])):
        with pytest.raises(ValueError):
            seqset.seqset_arrays(**{**dict(codes=codes, seq_offsets=offsets, lengths=lengths), **bad_arguments})
    with pytest.raises(_lib.TimedHipError) as err:
        seqset.seqset_arrays(bad_code, offsets, lengths)
    assert err.value.code == _lib.TH_EINVAL


def test_encode_readers_threshold_budget_and_parser(tmp_path):
    assert seqset.encode(["acdEFGHIKLMNPQRSTVWY", "XBZ-*acdefghiklmnpqr"]).tolist() == [list(range(20)), [20] * 5 + list(range(15))]
    assert seqset.encode([]).shape == (0, 0) and seqset.encode(["AC"]).dtype == np.uint8 and seqset.decode([0, 20, 19]) == "AXY"
    assert seqset.LETTERS[:20] == analysis.RESIDUES and len(seqset.LETTERS) == 21
    with pytest.raises(ValueError):
        seqset.encode(["AC", "ACD"])
    # the per-mille threshold, in integers
    assert seqset.min_matches_of(0.8, 76) == 61 and seqset.min_matches_of(0.9, 9) == 9 and seqset.min_matches_of(0.7, 76) == 54
    assert seqset.min_matches_of(0.9, 300) == 270 and seqset.min_matches_of(0.0, 5) == 0 and seqset.min_matches_of(1.0, 1030) == 1030
    assert seqset.min_matches_of(0.29999999, 10) == 3 and seqset.min_matches_of(0.3004, 10) == 3 and seqset.min_matches_of(0.3006, 10) == 4
    assert all(seqset.min_matches_of(p / 1000.0, length) == qr.min_matches(p, length) for p in range(0, 1001, 7) for length in (1, 9, 76, 1030))
    with pytest.raises(ValueError):
        seqset.min_matches_of(1.2, 10)
    # the byte budget: N L + 32 N + 88 L, and 4 N^2 with the matrix
    assert seqset.set_bytes(70, 76) == 70 * 76 + 32 * 70 + 88 * 76 and seqset.set_bytes(70, 76, True) == seqset.set_bytes(70, 76) + 4 * 70 * 70
    sizes = [seqset.set_bytes(10, 5), seqset.set_bytes(10, 5), seqset.set_bytes(10, 5)]
    assert batching.cut_batches(sizes, 2 * sizes[0], 1) == [(0, 2), (2, 3)]
    assert batching.cut_batches([seqset.set_bytes(10, 5, True)] * 3, 2 * sizes[0], 1) == [(0, 1), (1, 2), (2, 3)]          # the matrix counts
    # what sample.py writes
    from design_utils import sampling_utils as su
    sampled = {"1abcA": [("ACD", 0.1, 5.0, 300.0, 0.0), ("ACE", 0.2, 5.1, 310.0, 0.0)], "2xyz_B": [("WWYYV", 0.0, 6.0, 700.0, 11000.0)]}
    written = su.save_as(sampled, str(tmp_path / "draws"), "all")
    want = {"1abcA": ["ACD", "ACE"], "2xyz_B": ["WWYYV"]}
    assert seqset.read_sample_json(written[0]) == want and seqset.read_sample_fasta(written[1]) == want            # the key: before the LAST underscore
    assert seqset.read_samples(written[0]) == want and seqset.read_samples(written[1]) == want
    (tmp_path / "native.fasta").write_text(">1abcA some text\nAC\nD\n\n>2xyz_B\nWWYYA\n")
    assert seqset.read_native_fasta(tmp_path / "native.fasta") == {"1abcA": "ACD", "2xyz_B": "WWYYA"}
    (tmp_path / "wrapped.fasta").write_text(">k_0\nAC\nDE\n>k_1\nACDF\n")
    assert seqset.read_sample_fasta(tmp_path / "wrapped.fasta") == {"k": ["ACDE", "ACDF"]}
    # the parser
    import analyse_samples
    flags = dict(analyse_samples.CLI_FLAGS)
    assert list(flags) == ["--path_to_samples", "--path_to_output", "--path_to_datasetmap", "--support_old_datasetmap", "--path_to_native_fasta",
                           "--cluster_identity", "--matrix", "--device"]
    args = analyse_samples.build_parser().parse_args(["--path_to_samples", "a.json", "b.fasta", "--path_to_output", "out"])
    assert args.path_to_samples == ["a.json", "b.fasta"] and args.cluster_identity == 0.9 and args.matrix is False and args.device == 0
    assert args.path_to_datasetmap is None and args.support_old_datasetmap is False and args.path_to_native_fasta is None
    with pytest.raises(SystemExit):
        analyse_samples.build_parser().parse_args(["--path_to_output", "out"])


def test_analyse_and_the_command_line_on_the_restatement(monkeypatch, tmp_path, golden, capsys):
    calls = []

    def counted(codes, seq_offsets, lengths, *a, **kw):
        calls.append(len(lengths))
        return restated_arrays(codes, seq_offsets, lengths, *a, **kw)
    monkeypatch.setattr(seqset, "seqset_arrays", counted)
    drift, native = golden["ubq_drift_codes"], golden["ubq_drift_native"]
    two = golden["two_tiles_codes"]
    sets = [drift, [seqset.decode(r) for r in two], ["ACD", "AC"], golden["single_codes"], golden["empty_codes"], drift]
    natives = [native, None, None, seqset.decode(golden["single_native"]), golden["empty_native"], "ACD"]
    stats = {}
    res = seqset.analyse(sets, natives, cluster_identity=0.8, matrix=True, stats=stats)
    assert calls == [4] and stats["submissions"] == 1
    ubq, toy, ragged, single, empty, wrong = res
    assert "unequal lengths" in ragged.error and "the native has 3 residues, the sequences 76" in wrong.error and ragged.n == 0 and len(ragged.seq) == 0
    assert ubq.error is None and same_bytes(ubq.seq, golden["ubq_drift_seq"]) and same_bytes(ubq.profile, golden["ubq_drift_profile"])
    assert same_bytes(ubq.totals, golden["ubq_drift_set"]) and same_bytes(ubq.matrix, golden["ubq_drift_matrix"]) and ubq.min_matches == 61
    assert ubq.identity_to_native.tolist() == (ubq.seq[:, 0] / 76.0).tolist() and ubq.similarity_to_native.tolist() == (ubq.seq[:, 1] / 76.0).tolist()
    assert ubq.mean_identity_to_others.tolist() == (ubq.seq[:, 3] / (69.0 * 76.0)).tolist() and ubq.nearest_identity[2] == 1.0
    assert ubq.mean_pairwise_identity == float(ubq.totals[0]) / (2415 * 76) and ubq.mean_identity_to_native == float(ubq.totals[3]) / (70 * 76)
    assert ubq.representatives.tolist() == np.flatnonzero(ubq.seq[:, 7] == np.arange(70)).tolist() and len(ubq.representatives) == ubq.n_clusters
    assert ubq.n_distinct == 68 and ubq.native_recovery.tolist() == (ubq.profile[np.arange(76), native] / 70.0).tolist()
    assert 0.75 < ubq.native_recovery.mean() < 0.95 and (seqset.decode(ubq.consensus) == seqset.decode(native))
    assert same_bytes(toy.seq[:, :7], golden["two_tiles_seq"][:, :7]) and np.isnan(toy.identity_to_native).all() and np.isnan(toy.native_recovery).all()
    assert np.isnan(toy.mean_identity_to_native) and toy.min_matches == 8 and not toy.native_count.any()
    # consensus: the lowest code on ties; entropy in bits from the counts
    tie = seqset.analyse([["AC", "CC", "CA", "AA"]], cluster_identity=None)[0]
    assert tie.consensus.tolist() == [0, 0] and tie.position_entropy.tolist() == [1.0, 1.0] and tie.n_clusters == -1 and len(tie.representatives) == 0
    flat = seqset.analyse([["AC", "AD", "AE", "AF"]])[0]
    assert flat.position_entropy.tolist() == [0.0, 2.0] and seqset.decode(flat.consensus) == "AC"
    assert same_bytes(single.seq, golden["single_seq"]) and np.isnan(single.nearest_identity).all() and np.isnan(single.mean_pairwise_identity)
    assert single.similarity_to_native.tolist() == [2.0 / 3.0] and single.identity_to_native.tolist() == [3.0 / 5.0]
    assert empty.n == 0 and empty.error is None and np.isnan(empty.position_entropy).all() and np.isnan(empty.mean_identity_to_native)
    # the budget cuts the calls
    del calls[:]
    stats = {}
    split = seqset.analyse([drift, two, drift], [native, None, native], cluster_identity=0.8, budget_bytes=seqset.set_bytes(70, 76) + 10, stats=stats)
    assert calls == [1, 1, 1] and stats["submissions"] == 3 and same_bytes(split[2].seq, golden["ubq_drift_seq"]) and same_bytes(split[1].seq[:, :7], golden["two_tiles_seq"][:, :7])
    from design_utils.analyse_utils import calculate_sequence_identity, calculate_sequence_similarity
    assert calculate_sequence_identity("ACDX", "ACEX") == 0.75 and calculate_sequence_similarity("ACDX", "ACEX") == 1.0       # D/E score 2; X is skipped
    with pytest.raises(ValueError):
        calculate_sequence_identity("ACD", "AC")
    # the command line: a JSON and a FASTA of sample.py, natives from an old 4-column map and from a FASTA
    import analyse_samples
    from design_utils.amino_acids import standard_amino_acids
    json.dump({"1ubqA": [[seqset.decode(r), 0.0, 0.0, 0.0, 0.0] for r in drift[:40]]}, open(tmp_path / "one.json", "w"))
    with open(tmp_path / "two.fasta", "w") as f:
        f.writelines(f">1ubqA_{n}\n{seqset.decode(r)}\n" for n, r in enumerate(drift[40:]))
        f.writelines(f">toy_{n}\n{seqset.decode(r)}\n" for n, r in enumerate(two))
        f.write(">ragged_0\nACD\n>ragged_1\nAC\n")
    with open(tmp_path / "map.txt", "w") as f:
        f.writelines(f"1ubq,A,{k + 1},{standard_amino_acids[seqset.decode([c])]}\n" for k, c in enumerate(native))
    common = ["--path_to_samples", str(tmp_path / "one.json"), str(tmp_path / "two.fasta"), "--cluster_identity", "0.8"]
    parser = analyse_samples.build_parser()
    paths = analyse_samples.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "a"), "--path_to_datasetmap", str(tmp_path / "map.txt"),
                                                             "--support_old_datasetmap", "--matrix"]))
    assert "3 keys (1 with an error), 200 sequences in 1 GPU submission(s)" in capsys.readouterr().out
    assert [os.path.basename(p) for p in paths] == ["sample_scores.csv", "set_scores.csv", "position_profile.csv", "representatives.fasta",
                                                    "1ubqA_identity.csv", "toy_identity.csv"]
    (tmp_path / "native.fasta").write_text(f">1ubqA\n{seqset.decode(native)}\n")
    again = analyse_samples.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "b"), "--path_to_native_fasta", str(tmp_path / "native.fasta")]))
    assert len(again) == 4 and all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(paths, again))
    with open(paths[1], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == analyse_samples.SET_COLUMNS and [r[0] for r in rows[1:]] == ["1ubqA", "toy", "ragged"]
    assert rows[1][1:3] == ["70", "76"] and rows[1][5:9] == ["68", str(int(golden["ubq_drift_set"][2])), "61", ""] and "unequal lengths" in rows[3][8]
    assert float(rows[1][3]) == ubq.mean_identity_to_native and float(rows[1][4]) == ubq.mean_pairwise_identity and rows[2][3] == ""
    with open(paths[0], newline="") as f:
        draws = list(csv.reader(f))
    assert draws[0] == analyse_samples.SAMPLE_COLUMNS and len(draws) == 201 and [float(r[3]) for r in draws[1:71]] == ubq.identity_to_native.tolist()
    assert [int(r[11]) for r in draws[1:71]] == ubq.cluster.tolist() and draws[71][3:6] == ["", "", ""] and draws[70][2] == "1ubqA_69"
    with open(paths[2], newline="") as f:
        profile = list(csv.reader(f))
    assert profile[0] == analyse_samples.PROFILE_COLUMNS and len(profile) == 1 + 76 + 9 and profile[1][:4] == ["1ubqA", "0", "M", "M"]
    assert [float(r[4]) for r in profile[1:77]] == ubq.position_entropy.tolist() and [int(r[5]) for r in profile[1:77]] == ubq.native_count.tolist()
    assert [[int(v) for v in r[6:]] for r in profile[77:]] == golden["two_tiles_profile"].tolist() and profile[77][2] == "" and profile[77][5] == ""
    fasta = open(paths[3]).read().splitlines()
    assert fasta[:2] == [">1ubqA_0", seqset.decode(drift[0])] and len(fasta) == 2 * (ubq.n_clusters + toy.n_clusters)
    assert np.array_equal(np.loadtxt(paths[4], delimiter=",", dtype=np.int32), golden["ubq_drift_matrix"])
