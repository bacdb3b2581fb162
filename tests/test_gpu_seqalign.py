"""th_seqalign on the GPU against the restatement (tests/seqalign_restatement.py) and the committed fixture.  Everything is an integer:
align_out and count_out are EXACT everywhere, no tolerance exists.  The lengths sit around every boundary of k_seqalign_fill — a strip
of 8 columns, the 64 rows a wavefront fetches at a time, a panel of 512 columns (511, 512, 513; two and three panels), n >> m and
m >> n — one pair of 700 x 900 crosses a panel with a long trace, and a ragged batch of 40 pairs with empty ones among them is
submitted in two orders and split into two calls: a pair's bytes do not depend on its place.  Then the ABI errors on the device build,
and align() / analyse_models.py --seqalign / --pair_by_seqalign end to end on files written by pdbio.write_pdb.
"""
import csv
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqalign_restatement as ar  # noqa: E402
from test_seqalign_host import abi_call, bad_calls, fresh  # noqa: E402
from timed_hip import _lib, seqalign  # noqa: E402

pytestmark = pytest.mark.gpu

STRIP, ROWS, PANEL = 8, 64, 512


@pytest.fixture(scope="module")
def golden():
    return np.load(ar.GOLDEN)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def related(n, m, rng, letters=20):
    """two sequences of n and m residues with a common ancestor: copies of one random sequence with substitutions, and a stretch cut
    out of the longer one's middle, so that the best path has real gaps; ``letters`` small makes equal scores frequent"""
    base = rng.integers(0, letters, max(n, m) + 40).astype(np.uint8)

    def copy(length):
        start = int(rng.integers(0, 20))
        cut = int(rng.integers(0, 20)) if length > 40 else 0
        out = np.concatenate([base[start:start + length // 2], base[start + length // 2 + cut:]])[:length].copy()
        hit = rng.random(length) < 0.25
        out[hit] = rng.integers(0, letters + 1, int(hit.sum()))           # code 20 among them
        return out
    return copy(n), copy(m)


def check(what, pairs, **kw):
    """one call of all pairs against the restatement of each"""
    ref, ro, mob, mo = ar.flatten(pairs)
    timing = {}
    got = seqalign.seqalign_arrays(ref, ro, mob, mo, timing=timing, **kw)
    rule = dict(S=kw.get("matrix"), gap_open=kw.get("gap_open", 20), gap_extend=kw.get("gap_extend", 1), free_ends=int(kw.get("free_ends", True)))
    for k, (a, b) in enumerate(pairs):
        want = ar.restate(a, b, **rule)
        assert same_bytes(got.counts[k], want["counts"]), (what, k, len(a), len(b), got.counts[k].tolist(), want["counts"].tolist())
        mine = got.align[ro[k]:ro[k + 1]]
        assert same_bytes(mine, want["align"]), (what, k, len(a), len(b), np.nonzero(mine != want["align"])[0][:8].tolist())
    print(f"{what}: {len(pairs)} pairs exact; fill {timing['fill_ms']:.3f} ms, trace {timing['trace_ms']:.3f} ms")
    return got


def test_fixture_every_case_and_setting(gpu, golden):
    names = [str(n) for n in golden["cases"]]
    assert len(names) >= 24 and [str(s) for s in golden["settings"]] == list(ar.SETTINGS)
    ref, ro, mob, mo = ar.flatten([(golden[f"{n}_ref"], golden[f"{n}_model"]) for n in names])
    for setting, (table, gap_open, gap_extend, free_ends) in ar.SETTINGS.items():
        got = seqalign.seqalign_arrays(ref, ro, mob, mo, table(), gap_open, gap_extend, bool(free_ends), device=gpu)
        for k, n in enumerate(names):
            assert same_bytes(got.counts[k], golden[f"{n}_{setting}_counts"]), (setting, n, got.counts[k].tolist(), golden[f"{n}_{setting}_counts"].tolist())
            assert same_bytes(got.align[ro[k]:ro[k + 1]], golden[f"{n}_{setting}_align"]), (setting, n)
    free = seqalign.seqalign_arrays(ref, ro, mob, mo, device=gpu)                 # the defaults are the first setting
    for name, (score, _, aligned) in ar.TABLE.items():
        assert free.counts[names.index(name)].tolist()[2:4] == [score, aligned], name


def test_lengths_around_every_boundary(gpu):
    assert (STRIP, ROWS, PANEL) == (seqalign._STRIP, seqalign._LANES, seqalign._STRIP * seqalign._LANES)
    rng = np.random.default_rng(950)
    columns = (1, 7, 8, 9, 63, 64, 65, PANEL - 1, PANEL, PANEL + 1)
    rows = (1, 2, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS, 2 * ROWS + 1)
    sizes = [(n, m) for n in rows for m in columns if (n in (1, ROWS + 1) or m in (1, 65, PANEL + 1))]
    sizes += [(PANEL + 1, 1), (PANEL, PANEL - 1), (5, 300), (300, 5), (70, 2 * PANEL), (70, 2 * PANEL + 1), (ROWS + 2, 2 * PANEL + 9)]
    pairs = [related(n, m, rng, letters=20 if k % 2 else 3) for k, (n, m) in enumerate(sizes)]
    assert [(len(a), len(b)) for a, b in pairs] == sizes
    got = check("boundaries, free ends", pairs, device=gpu)
    assert (got.counts[:, 3] > 0).sum() > len(pairs) // 2 and (got.counts[:, 6] > 0).sum() >= 5       # real alignments with real gaps
    check("boundaries, charged ends", pairs, free_ends=False, device=gpu)
    check("boundaries, identity table 3 / 1", pairs, matrix=ar.identity_matrix(), gap_open=3, gap_extend=1, device=gpu)
    check("boundaries, equal costs 2 / 2", pairs, matrix=ar.identity_matrix(), gap_open=2, gap_extend=2, free_ends=False, device=gpu)


def test_700_by_900_and_three_panels(gpu):
    rng = np.random.default_rng(709)
    pairs = [related(700, 900, rng), related(900, 700, rng, letters=4), related(130, 2 * PANEL + 270, rng, letters=4)]
    assert seqalign.trace_bytes(700, 900) > 160 * 1024                           # more than a compute unit's LDS: the bits live in device memory
    got = check("700 x 900", pairs, device=gpu)
    assert got.counts[0, 3] > 600 and got.counts[0, 6] >= 2
    check("700 x 900, charged ends", pairs, free_ends=False, device=gpu)
    # the largest scores the ABI admits: 4096 identities of 127, and a border of 32767 per residue
    top = np.full((21, 21), -127, np.int32)
    top[np.arange(21), np.arange(21)] = 127
    a = rng.integers(0, 20, 4096).astype(np.uint8)
    far = seqalign.seqalign_arrays(np.concatenate([a, a[:9]]), [0, 4096, 4105], np.concatenate([a, np.zeros(0, np.uint8)]), [0, 4096, 4096], top, 32767, 32767,
                                   False, device=gpu)
    assert far.counts.tolist() == [[4096, 4096, 4096 * 127, 4096, 4096, 4096, 0, 0], [9, 0, -9 * 32767, 0, 0, 0, 0, 0]]
    assert far.align[:4096].tolist() == list(range(4096)) and (far.align[4096:] == -1).all()


def test_a_pair_s_bytes_do_not_depend_on_its_place(gpu):
    rng = np.random.default_rng(40)
    lengths = [0, 1, 5, 8, 9, 30, 64, 76, 100, 129, 200, 300, PANEL + 7]
    sizes = [(int(rng.choice(lengths)), int(rng.choice(lengths))) for _ in range(36)] + [(0, 0), (0, 50), (50, 0), (PANEL + 7, 64)]
    pairs = [related(n, m, rng, letters=20 if k % 3 else 2) for k, (n, m) in enumerate(sizes)]
    assert len(pairs) == 40 and sum(1 for a, b in pairs if len(a) == 0 or len(b) == 0) >= 3
    whole = check("ragged batch", pairs, device=gpu)
    ro = np.concatenate([[0], np.cumsum([len(a) for a, _ in pairs])])
    order = rng.permutation(40)
    assert (order != np.arange(40)).sum() > 30
    shuffled = seqalign.seqalign_arrays(*ar.flatten([pairs[k] for k in order]), device=gpu)
    at = 0
    for place, k in enumerate(order):
        n = len(pairs[k][0])
        assert same_bytes(shuffled.counts[place], whole.counts[k]) and same_bytes(shuffled.align[at:at + n], whole.align[ro[k]:ro[k + 1]]), (place, k)
        at += n
    first, second = (seqalign.seqalign_arrays(*ar.flatten(part), device=gpu) for part in (pairs[:17], pairs[17:]))
    assert same_bytes(np.concatenate([first.counts, second.counts]), whole.counts) and same_bytes(np.concatenate([first.align, second.align]), whole.align)
    again = seqalign.seqalign_arrays(*ar.flatten(pairs), device=gpu)
    assert same_bytes(again.align, whole.align) and same_bytes(again.counts, whole.counts)


def test_abi_errors_return_einval_and_leave_the_outputs_untouched(gpu, lib, golden):
    ref, ro, mob, mo = ar.flatten([(golden["deletion_ref"], golden["deletion_model"]), (golden["one_many_ref"], golden["one_many_model"])])
    matrix = ar.default_matrix()
    good = (ref, ro, mob, mo, matrix)
    for what, change in bad_calls(*good).items():
        out = fresh()
        rc, ms = abi_call(lib, gpu, out, good, **change)
        assert rc == _lib.TH_EINVAL, what
        assert b"th_seqalign" in lib.th_last_error(), what
        assert (out["align"] == 12345).all() and (out["counts"] == 12345).all() and ms == [-1.0, -1.0], what
    out = fresh()
    rc, ms = abi_call(lib, gpu, out, good)
    want = seqalign.seqalign_arrays(ref, ro, mob, mo, device=gpu)
    assert rc == _lib.TH_OK and ms[0] > 0 and ms[1] > 0
    assert same_bytes(out["align"][:len(ref)], want.align) and (out["align"][len(ref):] == 12345).all() and same_bytes(out["counts"], want.counts)
    assert lib.th_seqalign(gpu, None, 0, None, None, 0, None, 0, None, 20, 1, 1, None, None, None) == _lib.TH_OK                    # n_pairs = 0
    empty = seqalign.seqalign_arrays(np.zeros(0, np.uint8), [0, 0], np.zeros(0, np.uint8), [0, 0], device=gpu)                       # a pair of nothing
    assert empty.counts.tolist() == [[0] * 8] and empty.align.size == 0


def test_files_and_cli_end_to_end(gpu, tmp_path, capsys, monkeypatch):
    import analyse_models
    from design_utils import analyse_utils
    protein = ar.write_ubq_files(tmp_path)
    ubq = ar.ubq_sequence()
    monkeypatch.chdir(tmp_path)                                                 # relative paths: the tables do not name the directory
    listed = [("native.pdb", os.path.join("models", f"{name}.pdb")) for name in ("copy", "deleted", "moved")]
    stats = {}
    results = seqalign.align(listed, device=gpu, stats=stats)
    assert stats["submissions"] == 1 and stats["files_parsed"] == 4 and stats["kernel_ms"] > 0
    assert [(r.error, r.n_ref, r.n_model, r.score, r.n_aligned, r.n_gaps, r.n_gap_residues) for r in results] == [
        (None, 76, 76, 762, 76, 0, 0), (None, 76, 70, 681, 70, 1, 6), (None, 76, 76, 762, 76, 0, 0)]
    assert results[0].model_index.tolist() == list(range(76)) and results[1].reference_index.tolist() == list(range(22)) + list(range(28, 76))
    deleted = ubq[:22] + ubq[28:]
    assert analyse_utils.align_sequences(ubq, deleted, device=gpu) == (ubq, ubq[:22] + "-" * 6 + ubq[28:], 681)
    (text,) = seqalign.align_strings([(ubq, deleted)], device=gpu)
    assert same_bytes(text.reference_index, results[1].reference_index) and text.score == 681
    # the command line
    parser = analyse_models.build_parser()
    common = ["--path_to_reference", "native.pdb", "--device", str(gpu)]
    models, same = common + ["--path_to_models", "models"], common + ["--path_to_models", "same"]

    def read(folder, name):
        with open(tmp_path / folder / name, newline="") as f:
            return list(csv.reader(f))
    # without the new flags no alignment is made, and the tables hold the bytes the parent commit wrote for these files
    with monkeypatch.context() as patched:
        patched.setattr(seqalign, "align", None)
        patched.setattr(seqalign, "seqalign_arrays", None)
        analyse_models.main(parser.parse_args(models + ["--path_to_output", "plain", "--lddt", "--tmscore"]))
    golden_dir = os.path.join(ar.ROOT, "tests", "golden")
    for name in ("model_scores.csv", "residue_deviation.csv", "model_lddt.csv", "model_tmscore.csv"):
        with open(os.path.join(golden_dir, "seqalign_parent_" + name), "rb") as f:
            assert (tmp_path / "plain" / name).read_bytes() == f.read(), name
    assert "length mismatch" in read("plain", "model_scores.csv")[2][-1]
    analyse_models.main(parser.parse_args(models + ["--path_to_output", "out", "--seqalign"]))
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["model_scores.csv", "model_seqalign.csv", "residue_deviation.csv", "residue_seqalign.csv"]
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (tmp_path / "out" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes()
    rows = read("out", "model_seqalign.csv")
    assert rows[0] == analyse_models.SEQALIGN_COLUMNS and [r[0] for r in rows[1:]] == ["copy.pdb", "deleted.pdb", "moved.pdb"]
    assert rows[2][3:] == ["76", "70", "681", "70", "1.0", "1.0", "1", "6", repr(70 / 76), "1.0", ""]
    mine = [r for r in read("out", "residue_seqalign.csv")[1:] if r[0] == "deleted.pdb"]
    assert len(mine) == 76 and [r[2] for r in mine if not r[5]] == [protein[k].number for k in range(22, 28)]        # the six unaligned
    assert all(r[3] == r[6] and r[2] == r[5] for r in mine if r[5])
    # on pairs of one sequence the self alignment is the identity (checked above): the same bytes as pairing by position
    analyse_models.main(parser.parse_args(same + ["--path_to_output", "by_position", "--pair_by", "position", "--lddt"]))
    analyse_models.main(parser.parse_args(same + ["--path_to_output", "by_sequence", "--pair_by_seqalign", "--lddt"]))
    for name in ("model_scores.csv", "residue_deviation.csv", "model_lddt.csv", "residue_lddt.csv"):
        assert (tmp_path / "by_sequence" / name).read_bytes() == (tmp_path / "by_position" / name).read_bytes(), name
    assert len(read("by_position", "model_scores.csv")) == 3 and all(r[-1] == "" for r in read("by_position", "model_scores.csv")[1:])
    # the deleted-loop model, a length mismatch by position, is scored over its 70 aligned residues by every scorer
    analyse_models.main(parser.parse_args(models + ["--path_to_output", "sa", "--pair_by_seqalign", "--lddt", "--tmscore"]))
    row = dict(zip(*[read("sa", "model_scores.csv")[k] for k in (0, 2)]))
    assert row["error"] == "" and row["n_valid"] == "70" and (row["unpaired_reference"], row["unpaired_model"]) == ("6", "0")
    assert float(row["rmsd_fit_all"]) < 1e-6 and row["sequence_identity"] == "1.0"
    ld = dict(zip(*[read("sa", "model_lddt.csv")[k] for k in (0, 2)]))
    tm = dict(zip(*[read("sa", "model_tmscore.csv")[k] for k in (0, 2)]))
    assert ld["error"] == "" and ld["n_valid"] == "70" and float(ld["lddt"]) == 1.0
    assert tm["error"] == "" and (tm["n_valid"], tm["norm_length"]) == ("70", "76") and abs(float(tm["tm_score"]) - 70 / 76) < 1e-6
    with pytest.raises(SystemExit):
        analyse_models.main(parser.parse_args(models + ["--path_to_output", "bad", "--pair_by_seqalign", "--pair_by_cealign"]))
    capsys.readouterr()
