"""TM-score without a GPU: the NumPy restatement (tests/tmscore_restatement.py) against the committed fixture and against itself in
long double; the seed schedule and d0; the Python layer's argument checks, its byte budget and analyse_models.py --tmscore with the
kernel call replaced by the restatement; the header prototype, the ctypes entry and the build list."""
import csv
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import superpose_restatement as sr  # noqa: E402
import tmscore_restatement as tr  # noqa: E402
from test_superpose_host import restated_arrays as restated_superpose  # noqa: E402
from timed_hip import _lib, pdbio, superpose, tmscore  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHRASE = "PARITY UNPINNED AGAINST THE TM-score PROGRAM"


@pytest.fixture(scope="module")
def cases():
    return sr.ubq_cases()


@pytest.fixture(scope="module")
def restated(cases):
    """the float64 and the long double restatement of the five cases: computed once, shared, never changed"""
    return {name: (tr.restate(*cases[name]), tr.restate(*cases[name], dtype=np.longdouble)) for name in sr.CASES}


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restated_arrays(ref_xyz, mob_xyz, offsets, norm_len=None, rounds=20, device=0, timing=None, transform=False, dist=True):
    """tmscore.tmscore_arrays with the GPU call replaced by the restatement"""
    ref_xyz, mob_xyz = np.asarray(ref_xyz, np.float64).reshape(-1, 3), np.asarray(mob_xyz, np.float64).reshape(-1, 3)
    parts = [tr.restate(ref_xyz[lo:hi], mob_xyz[lo:hi], None if norm_len is None else norm_len[k], rounds)
             for k, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:]))]
    return tmscore.TmTables(np.array([[p["tm"], p["d0"]] for p in parts], np.float64).reshape(-1, 2),
                            np.array([p["counts"] for p in parts], np.int64).reshape(-1, 4),
                            np.concatenate([p["dist"] for p in parts] + [np.zeros(0)]) if dist else None,
                            np.array([p["transform"] for p in parts], np.float64).reshape(-1, 3, 4) if transform else None)


def test_restatement_reproduces_the_fixture_and_the_figures_of_the_rule(cases, restated):
    assert os.path.getsize(tr.GOLDEN) < 64 * 1024
    golden = np.load(tr.GOLDEN)
    assert str(golden["sha256"]) == sr.inputs_sha256(cases) == str(np.load(sr.GOLDEN)["sha256"])            # the inputs of the superposition fixture
    again = tr.golden_arrays(cases)
    assert sorted(golden.files) == sorted(again)
    for key in golden.files:
        assert same_bytes(golden[key], np.asarray(again[key])), key
    text = open(os.path.join(ROOT, "tests", "golden", "make_tmscore_golden.py")).read()
    assert "NOT by the kernel" in text and PHRASE in text
    want = {"rigid": (1.0, 239, 477), "noise": (0.93252, 239, 537), "hinge": (0.90386, 239, 520), "mirror": (0.30830, 239, 1205),
            "invalid": (0.88510, 230, 526)}
    for name, (tm, n_seeds, n_fits) in want.items():
        assert abs(float(golden[f"{name}_tm"]) - tm) < 5e-6 and golden[f"{name}_counts"].tolist()[2:] == [n_seeds, n_fits], name
        assert abs(float(golden[f"{name}_d0"]) - 3.08126) < 5e-6 and golden[f"{name}_counts"][1] == 76
    assert golden["invalid_counts"][0] == 73 and float(golden["rigid_tm"]) > 1 - 1e-12
    assert abs(float(golden["hinge_tm_global_fit"]) - 0.66093) < 5e-6 and float(golden["mirror_tm"]) < 0.4


def test_float64_restatement_against_long_double(restated):
    for name, (a, b) in restated.items():
        err = abs(float(np.longdouble(a["tm"]) - b["tm"]))
        print(f"{name}: float64 restatement vs long double, tm error {err:.3e}; nearest edge {a['edge']:.3e}, eigenvalue gap {a['gap']:.3e}")
        assert same_bytes(a["counts"], b["counts"]) and (a["seed"], a["round"]) == (b["seed"], b["round"]), name
        assert err < 1e-13 and a["edge"] > 3.2e-5 and a["gap"] > 8.9e-3, name
        assert np.array_equal(np.isnan(a["dist"]), np.isnan(b["dist"])) and np.nanmax(np.abs(a["dist"] - b["dist"])) < 1e-11


def test_the_search_never_scores_below_the_global_fit(cases, restated):
    for name in sr.CASES:
        whole = float(tr.global_fit_score(*cases[name]))
        best = float(restated[name][0]["tm"])
        assert best >= whole, (name, best, whole)                               # the first seed IS the global fit
        assert best <= 1.0
    assert float(restated["hinge"][0]["tm"]) > 0.85 and float(tr.global_fit_score(*cases["hinge"])) < 0.7
    # the restatement's own parts: the global fit is th_superpose's cycle-0 fit
    once = sr.restate(*cases["hinge"], cycles=0)
    assert float(tr.score_of_distances(once["dist"], 76, np.float64)) == float(tr.global_fit_score(*cases["hinge"]))
    empty = tr.restate(np.full((4, 3), np.nan), np.zeros((4, 3)))
    assert np.isnan(empty["tm"]) and empty["counts"].tolist() == [0, 4, 0, 0] and np.isnan(empty["dist"]).all()
    assert empty["transform"].tolist() == np.eye(3, 4).ravel().tolist()


def test_seed_schedule(restated):
    assert tr.windows(76) == [76, 38, 19, 9, 4] and tr.windows(8) == [8, 4] and tr.windows(7) == [7] and tr.windows(0) == []
    want = {0: 0, 1: 1, 2: 1, 3: 1, 4: 1, 7: 1, 8: 6, 15: 10, 16: 1 + 9 + 13, 73: 230, 76: 239, 300: 1514}
    for m, seeds in want.items():
        assert tr.n_seeds_of(m) == seeds == tmscore.seed_count(m) == len(tr.seeds(m)), m
    for m in range(0, 200):
        assert tr.n_seeds_of(m) == tmscore.seed_count(m)
    assert tmscore.seed_count(4096) == sum(4096 - (4096 >> k) + 1 for k in range(11))
    assert restated["invalid"][0]["counts"][2] == 230
    starts = tr.seeds(9)
    assert starts[0] == (9, 0) and starts[1:] == [(4, s) for s in range(6)]


def test_d0(lib):
    lib.th_tm_d0.restype, lib.th_tm_d0.argtypes = C.c_double, [C.c_int64]
    want = {0: 0.5, 15: 0.5, 16: 0.5, 21: 0.5, 22: 1.24 * 7 ** (1 / 3) - 1.8, 76: 1.24 * 61 ** (1 / 3) - 1.8, 300: 1.24 * 285 ** (1 / 3) - 1.8}
    for L, d0 in want.items():
        assert abs(lib.th_tm_d0(L) - d0) < 1e-14 and abs(float(tr.d0_of(L)) - d0) < 1e-14 and tmscore.d0(L) == lib.th_tm_d0(L), L
    assert 0.57 < want[22] < 0.58 and 3.08 < want[76] < 3.09 and 6.35 < want[300] < 6.37 and 1.24 * 6 ** (1 / 3) - 1.8 < 0.5


def test_python_layer_checks_its_arguments():
    one, two = np.zeros((1, 3)), np.zeros((2, 3))
    with pytest.raises(ValueError, match="positions"):
        tmscore.tmscore_arrays(one, two, [0, 1])
    with pytest.raises(ValueError, match="offsets"):
        tmscore.tmscore_arrays(one, one, [])
    with pytest.raises(ValueError, match="norm_len"):
        tmscore.tmscore_arrays(one, one, [0, 1], norm_len=[1, 1])
    with pytest.raises(ValueError, match="norm_len"):
        tmscore.tmscore_arrays(one, one, [0, 1], norm_len=[1 << 31])
    with pytest.raises(ValueError, match="rounds"):
        tmscore.tmscore([], rounds=-1)
    with pytest.raises(ValueError):
        tmscore.tmscore([(one, one)], pair_by="alignment")
    assert tmscore.tmscore([]) == [] and tmscore.ROUNDS == 20 and tmscore.MAX_POSITIONS == 4096


def test_library_exports_th_tmscore_and_checks_arguments_without_a_gpu(lib):
    n = 5
    xyz = np.zeros((n, 3))
    offsets = np.array([0, n], np.int64)
    tm, counts, dist = np.full((1, 2), 6.5), np.full((1, 4), 77, np.int64), np.full(n, 6.5)
    long_pair = np.zeros((4097, 3))

    def call(ref=xyz, total=n, off=offsets, n_pairs=1, norm=None, rounds=20, t=tm, c=counts):
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)        # noqa: E731
        return lib.th_tmscore(0, p(ref), p(ref), total, p(off), n_pairs, p(norm), rounds, p(t), p(c), p(dist), None, None)
    bad = {"negative total": dict(total=-1), "negative pairs": dict(n_pairs=-1), "too large": dict(total=1 << 31), "rounds": dict(rounds=-1),
           "offsets NULL": dict(off=None), "tm NULL": dict(t=None), "counts NULL": dict(c=None), "lists NULL": dict(ref=None),
           "end": dict(off=np.array([0, n + 1], np.int64)), "start": dict(off=np.array([1, n], np.int64)),
           "decrease": dict(off=np.array([0, n + 1, n], np.int64), n_pairs=2), "norm_len short": dict(norm=np.array([n - 1], np.int32)),
           "4097 positions": dict(ref=long_pair, total=4097, off=np.array([0, 4097], np.int64))}
    for what, kw in bad.items():
        assert call(**kw) == _lib.TH_EINVAL, what
        assert b"th_tmscore" in lib.th_last_error(), what
    assert (tm == 6.5).all() and (counts == 77).all() and (dist == 6.5).all()
    assert lib.th_tmscore(0, None, None, 0, None, 0, None, 20, None, None, None, None, None) == _lib.TH_OK        # no pairs: no launch
    with pytest.raises(_lib.TimedHipError) as err:
        tmscore.tmscore_arrays(long_pair, long_pair, [0, 4097])
    assert err.value.code == _lib.TH_EINVAL and "4096" in str(err.value)


def _layouts(sizes, rng, extra_reference=0):
    out = []
    for n in sizes:
        ref, mob = sr.synthetic_pair(n, rng)
        residues = [pdbio.Residue("A", str(k + 1), "GLY") for k in range(n + extra_reference)]
        longer = np.concatenate([ref, np.zeros((extra_reference, 3))])
        out.append((superpose.AtomLayout(longer, residues), superpose.AtomLayout(mob, residues[:n])))
    return out


def test_batches_are_charged_positions_and_seeds_and_long_pairs_carry_an_error(monkeypatch):
    calls = []

    def counted(ref_xyz, mob_xyz, offsets, norm_len=None, *a, **kw):
        calls.append((len(offsets) - 1, None if norm_len is None else list(norm_len)))
        return restated_arrays(ref_xyz, mob_xyz, offsets, norm_len, *a, **kw)
    monkeypatch.setattr(tmscore, "tmscore_arrays", counted)
    rng = np.random.default_rng(1)
    layouts = _layouts((12, 12, 12, 12, 12), rng)
    stats = {}
    whole = tmscore.tmscore(layouts, stats=stats)
    assert calls == [(5, [12] * 5)] and stats["submissions"] == 1 and stats["files_parsed"] == 0
    one = tmscore.pair_bytes(12, 12)
    assert one == 12 * 60 + tr.n_seeds_of(12) * 12 == 12 * 60 + 8 * 12
    del calls[:]
    split = tmscore.tmscore(layouts, budget_bytes=2 * one + one // 2)           # two pairs fit, three do not
    assert [c[0] for c in calls] == [2, 2, 1]
    del calls[:]
    assert len(tmscore.tmscore(layouts, budget_bytes=2 * 12 * 60 + 50)) == 5 and [c[0] for c in calls] == [1] * 5      # without the seeds two would fit
    for a, b in zip(whole, split):
        assert a.error is None and a.tm == b.tm and same_bytes(a.dist, b.dist) and (a.n_seeds, a.n_fits) == (b.n_seeds, b.n_fits)
        want = tr.restate(*[lay.xyz for lay in layouts[whole.index(a)]])
        assert a.tm == float(want["tm"]) and [a.n_valid, a.norm_length, a.n_seeds, a.n_fits] == want["counts"].tolist() and a.d0 == float(want["d0"])
    # a pair above 4096 positions: its error, and its neighbours are scored
    residues = [pdbio.Residue("A", str(k + 1), "GLY") for k in range(4097)]
    giant = (superpose.AtomLayout(np.zeros((4097, 3)), residues), superpose.AtomLayout(np.zeros((4097, 3)), residues))
    del calls[:]
    first, middle, last = tmscore.tmscore([layouts[0], giant, layouts[1]])
    assert [c[0] for c in calls] == [2] and "4097" in middle.error and "4096" in middle.error and np.isnan(middle.tm) and middle.n_seeds == 0
    assert first.tm == whole[0].tm and last.tm == whole[1].tm
    # the normalisation length is the reference's: residues the model lacks cost score
    del calls[:]
    (short,) = tmscore.tmscore(_layouts((12,), np.random.default_rng(1), extra_reference=8), pair_by="number")
    assert calls == [(1, [20])] and short.norm_length == 20 and short.n_valid == 12 and short.unpaired_reference == 8 and short.tm < whole[0].tm
    assert short.d0 == float(tr.d0_of(20))


def test_analyse_models_writes_model_tmscore(tmp_path, monkeypatch, cases, capsys):
    import analyse_models
    monkeypatch.setattr(superpose, "superpose_arrays", restated_superpose)
    monkeypatch.setattr(tmscore, "tmscore_arrays", restated_arrays)
    ref, hinge = cases["hinge"]
    (tmp_path / "models").mkdir()
    (tmp_path / "native.pdb").write_text(sr.pdb_text(ref))
    (tmp_path / "models" / "hinge.pdb").write_text(sr.pdb_text(hinge))
    (tmp_path / "models" / "short.pdb").write_text(sr.pdb_text(hinge[:70]))
    parser = analyse_models.build_parser()
    common = ["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models", str(tmp_path / "models")]
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "plain")]))
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(tmp_path / "out"), "--tmscore"]))
    assert "3 GPU submission(s)" in capsys.readouterr().out                      # the superposition, the search and the cycle-0 fit
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["model_scores.csv", "residue_deviation.csv"]
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["model_scores.csv", "model_tmscore.csv", "residue_deviation.csv"]
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (tmp_path / "out" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes()
    with open(tmp_path / "out" / "model_tmscore.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == analyse_models.TMSCORE_COLUMNS == ["label", "reference", "model", "n_valid", "norm_length", "d0", "tm_score", "tm_global_fit",
                                                         "n_seeds", "n_fits", "error"]
    assert [r[0] for r in rows[1:]] == ["hinge.pdb", "short.pdb"]
    got = dict(zip(rows[0], rows[1]))
    want = tr.restate(np.round(ref, 3), np.round(hinge, 3))
    assert [int(got[k]) for k in ("n_valid", "norm_length", "n_seeds", "n_fits")] == want["counts"].tolist() and got["error"] == ""
    assert float(got["tm_score"]) == float(want["tm"]) and float(got["d0"]) == float(want["d0"])
    assert abs(float(got["tm_global_fit"]) - float(tr.global_fit_score(np.round(ref, 3), np.round(hinge, 3)))) < 1e-14
    assert float(got["tm_score"]) > 0.85 and float(got["tm_global_fit"]) < 0.7
    assert "length mismatch" in rows[2][-1] and rows[2][3:5] == ["0", "0"] and rows[2][6] == rows[2][7] == "nan"
    by_number = tmp_path / "by_number"
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(by_number), "--tmscore", "--tm_rounds", "0", "--pair_by", "number"]))
    with open(by_number / "model_tmscore.csv", newline="") as f:
        rows = list(csv.reader(f))
    short = dict(zip(rows[0], rows[2]))
    assert short["error"] == "" and (short["n_valid"], short["norm_length"]) == ("70", "76") and short["n_fits"] == short["n_seeds"]
    with pytest.raises(SystemExit):
        analyse_models.main(parser.parse_args(common + ["--path_to_output", str(by_number), "--tmscore", "--tm_rounds", "-1"]))
    args = parser.parse_args(["--pairs", "p.csv"])
    assert (args.tmscore, args.tm_rounds) == (False, 20)


_CTYPES = {"int": "c_int", "int64_t": "c_long", "double": "c_double", "const double*": "c_void_p", "const int64_t*": "c_void_p",
           "const int32_t*": "c_void_p", "int64_t*": "c_void_p", "double*": ("c_void_p", "LP_c_double")}


def test_header_ctypes_build_list_and_the_unpinned_parity_phrase():
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    m = re.search(r"^(\w+) th_tmscore\(([^;]*)\);", header, re.M)
    assert m
    res, args = _lib.PROTOTYPES["th_tmscore"]
    assert res.__name__ == _CTYPES[m.group(1)]
    declared = [re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", a.strip())).strip().rsplit(" ", 1)[0] for a in m.group(2).split(",")]
    assert len(declared) == len(args) == 13, (declared, args)
    for c_type, ct in zip(declared, args):
        want = _CTYPES[c_type]
        assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (c_type, ct)
    before = header[:m.start()]
    section = before[before.rindex("/* ----"):]
    for phrase in (PHRASE, "MIRROR IMAGES", "TH_TM_MAX_POSITIONS", "no fused multiply-add", "bytes per valid position", "per seed"):
        assert phrase in section, phrase
    assert re.search(r"^double th_tm_d0\(int64_t L\);", header, re.M) and "#define TH_TM_MAX_POSITIONS 4096" in header
    assert _lib.PROTOTYPES["th_tm_d0"][0].__name__ == "c_double"
    import __graft_entry__
    assert "tmscore.hip" in __graft_entry__.HIP_SOURCES
    source = open(os.path.join(ROOT, "timed-design_amd", "csrc", "tmscore.hip")).read()
    product = re.sub(r"#if TH_KNOCKOUTS\n.*?#endif\n", "", source, flags=re.S)          # the knock-out build's timing experiment apart
    assert PHRASE in source and '#include "horn_fit.h"' in source and "atomic" not in source.replace("No atomics", "") and "__shared__" not in product
    assert "__shared__" in source and "TH_TM_STAGE" in source
    shared = open(os.path.join(ROOT, "timed-design_amd", "csrc", "horn_fit.h")).read()
    assert "horn_rotation" in shared and "fp contract(off)" in shared
    assert "horn_rotation(const" not in open(os.path.join(ROOT, "timed-design_amd", "csrc", "superpose.hip")).read()      # moved, not copied
    # so are the transform store, the distance under a fit and the two accumulation steps: once in horn_fit.h, in no kernel file
    moved = ("f.cr[x] - ((f.R[3 * x]", "+ f.cr[0]) - ref[0]", "S[x][y] += a[x] * b[y]", "sm[a] += mob[a]")
    old = ("cr[x] - ((R[3 * x]", "+ cr[0]) -", "+ fr[0]) -", "[x][y] += ", "sm[a] +=", "fm[x] +=")
    for text in moved:
        assert shared.count(text) == 1, text
    for unit in ("superpose.hip", "tmscore.hip", "cealign.hip"):
        kernel_file = open(os.path.join(ROOT, "timed-design_amd", "csrc", unit)).read()
        for text in moved + old:
            assert text not in kernel_file, (unit, text)
        assert "store(" in kernel_file and "distance(" in kernel_file and "Fit " in kernel_file, unit
    assert "wave_fit(" in source and "tm_dist" not in source and "bcm" not in source
    import analyse_models
    text = re.sub(r"\s+", " ", analyse_models.build_parser().format_help())
    assert PHRASE in text and "--tmscore" in text and "4096" in text
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert PHRASE in tmscore.__doc__ and PHRASE in readme and "4096" in readme
    assert PHRASE in open(os.path.join(ROOT, "DESIGN.md")).read()
