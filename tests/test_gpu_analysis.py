"""th_analyse_probs (csrc/analysis.hip) on the GPU against the NumPy restatement (tests/analysis_restatement.py) and scipy, and
predict.py --output_analysis end to end (20-class Keras model and the 338-class synthetic rotamer model, plain, CLI and sharded)."""
import ctypes as C
import json
import os
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import analysis_restatement as ar  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _matrix(rng, n, k, dtype):
    """softmax rows with planted exact ties, zeros, all-zero rows, NaN / inf rows, negative entries; returns (x, planted NaN rows)"""
    z = rng.standard_normal((n, k)).astype(np.float32) * 2.5
    x = np.exp(z - z.max(axis=1, keepdims=True))
    x = (x / x.sum(axis=1, keepdims=True)).astype(dtype)
    undefined = np.zeros(n, dtype=bool)
    if n == 0:
        return x, undefined
    rows = rng.permutation(n)
    cut = np.array_split(rows[: max(1, n // 4)], 6)
    for i in cut[0]:                                    # exact ties of the row maximum in another column
        j = int(np.argmax(x[i]))
        x[i, rng.integers(0, k)] = x[i, j]
        x[i, (j + 1 + rng.integers(0, k - 1)) % k if k > 1 else j] = x[i, j]
    for i in cut[1]:                                    # zeros
        x[i, rng.integers(0, k, max(1, k // 3))] = 0
    for i in cut[2]:                                    # all-zero rows
        x[i] = 0
        undefined[i] = True
    for i in cut[3]:                                    # NaN rows (and one infinity among them)
        x[i, rng.integers(0, k)] = np.nan
        undefined[i] = True
    if len(cut[3]):
        x[cut[3][0], 0] = np.inf
    for i in cut[4]:                                    # negative entries
        x[i, rng.integers(0, k)] = -x[i].max() / 2 if x[i].max() > 0 else -1
        undefined[i] = True
    return x, undefined


def _truth(rng, n):
    t = rng.integers(0, 20, n).astype(np.int8)
    t[rng.random(n) < 0.1] = -1
    return t


def _columns(rng, k):
    if k == 20:
        return np.arange(20, dtype=np.int8)
    if k == 338:
        from design_utils import utils
        from timed_hip import analysis
        return analysis.rotamer_columns(utils.get_rotamer_codec()[1])
    return rng.integers(0, 20, k).astype(np.int8)       # interleaved, unordered


def _entropy_scipy(x):
    from scipy.stats import entropy
    out = np.empty(x.shape[0])
    for lo in range(0, x.shape[0], 8192):
        with np.errstate(all="ignore"):
            out[lo:lo + 8192] = entropy(x[lo:lo + 8192].astype(np.float64), base=2, axis=1)
    return out


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("k", [20, 338, 1024])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097, 100_003])
def test_analyse_probs_matches_the_restatement(gpu, n, k, dtype):
    from timed_hip import analysis, textio
    rng = np.random.default_rng(n * 7 + k + (1 if dtype == np.float16 else 0))
    x, undefined = _matrix(rng, n, k, dtype)
    t = _truth(rng, n)
    col = _columns(rng, k)
    got = analysis.analyse_probs(x, t, col, device=gpu)
    pred, rank, ent, tot = ar.restate(x, t, col)
    if n:
        letters = "".join(analysis.RESIDUES[c] for c in col)
        assert np.array_equal(np.frombuffer(analysis.RESIDUES.encode(), dtype="S1")[got.pred], textio.argmax_letters(x, letters))
    assert np.array_equal(got.pred, pred)
    assert np.array_equal(got.rank, rank)
    assert np.array_equal(got.confusion, tot["confusion"]) and np.array_equal(got.rank_hist, tot["rank_hist"])
    assert (got.n_labelled, got.n_nonfinite, got.n_similar) == (tot["n_labelled"], tot["n_nonfinite"], tot["n_similar"])
    assert np.array_equal(np.isnan(got.entropy), undefined)
    want = _entropy_scipy(x)
    ok = ~undefined
    assert np.abs(got.entropy[ok] - want[ok]).max(initial=0) <= 1e-12
    assert np.array_equal(np.isnan(ent), undefined)
    # identical bytes on a second call
    again = analysis.analyse_probs(x, t, col, device=gpu)
    for a, b in zip(got, again):
        assert (a.tobytes() == b.tobytes()) if isinstance(a, np.ndarray) else a == b


def test_staging_blocks_do_not_change_a_byte(gpu, monkeypatch):
    from timed_hip import analysis
    rng = np.random.default_rng(11)
    for k, dtype in ((20, np.float16), (338, np.float16), (1024, np.float32)):
        x, _ = _matrix(rng, 10_007, k, dtype)
        t = _truth(rng, 10_007)
        col = _columns(rng, k)
        monkeypatch.delenv("TH_ANALYSIS_BLOCK_ROWS", raising=False)
        whole = analysis.analyse_probs(x, t, col, device=gpu)
        for rows in ("1000", "4097", "1"):
            if rows == "1" and k != 20:
                continue
            monkeypatch.setenv("TH_ANALYSIS_BLOCK_ROWS", rows)
            blocked = analysis.analyse_probs(x, t, col, device=gpu)
            for a, b in zip(whole, blocked):
                assert (a.tobytes() == b.tobytes()) if isinstance(a, np.ndarray) else a == b, rows


def test_residue_without_a_column_and_outputs_optional(gpu):
    from timed_hip import _lib, analysis
    lib = _lib.load()
    rng = np.random.default_rng(3)
    x, _ = _matrix(rng, 500, 20, np.float32)
    col = np.arange(20, dtype=np.int8)
    col[5] = 6                                          # residue 5 owns no column
    t = _truth(rng, 500)
    got = analysis.analyse_probs(x, t, col, device=gpu)
    pred, rank, _, tot = ar.restate(x, t, col)
    assert np.array_equal(got.rank, rank) and np.all(got.rank[t == 5] == 20)
    assert np.array_equal(got.confusion, tot["confusion"])
    tot2 = analysis.Totals()
    rc = lib.th_analyse_probs(gpu, x.ctypes.data_as(C.c_void_p), _lib.TH_F32, 500, 20, col.ctypes.data_as(C.c_void_p),
                              t.ctypes.data_as(C.c_void_p), None, None, None, C.byref(tot2))
    assert rc == 0 and np.array_equal(np.ctypeslib.as_array(tot2.confusion), got.confusion)


def test_einval_cases(gpu):
    from timed_hip import _lib, analysis
    lib = _lib.load()
    x = np.full((4, 20), 0.05, np.float32)
    t = np.zeros(4, np.int8)
    col = np.arange(20, dtype=np.int8)

    def call(mat=x, dtype=_lib.TH_F32, n=4, k=20, cr=col, tr=t):
        tot = analysis.Totals()
        return lib.th_analyse_probs(gpu, mat.ctypes.data_as(C.c_void_p), dtype, n, k, cr.ctypes.data_as(C.c_void_p),
                                    tr.ctypes.data_as(C.c_void_p), None, None, None, C.byref(tot))
    assert call() == 0
    assert call(dtype=_lib.TH_F64) == _lib.TH_EINVAL
    assert call(dtype=_lib.TH_U8) == _lib.TH_EINVAL
    assert call(k=0) == _lib.TH_EINVAL
    big = np.zeros((1, 1025), np.float32)
    assert call(mat=big, n=1, k=1025, cr=np.zeros(1025, np.int8), tr=t[:1]) == _lib.TH_EINVAL
    bad_col = col.copy(); bad_col[7] = 20
    assert call(cr=bad_col) == _lib.TH_EINVAL
    bad_col[7] = -1
    assert call(cr=bad_col) == _lib.TH_EINVAL
    bad_t = t.copy(); bad_t[2] = 20
    assert call(tr=bad_t) == _lib.TH_EINVAL
    bad_t[2] = -2
    assert call(tr=bad_t) == _lib.TH_EINVAL
    tot = analysis.Totals()
    tot.n_labelled = 99
    assert lib.th_analyse_probs(gpu, None, _lib.TH_F16, 0, 20, col.ctypes.data_as(C.c_void_p), None, None, None, None,
                                C.byref(tot)) == 0
    assert tot.n_labelled == 0 and not np.ctypeslib.as_array(tot.confusion).any()
    with pytest.raises(_lib.TimedHipError):
        analysis.analyse_probs(x, t, bad_col, device=gpu)


def test_analysis_entry_points_of_analyse_utils(gpu, tmp_path):
    from scipy.stats import entropy
    from design_utils import analyse_utils as au
    rng = np.random.default_rng(8)
    x, undefined = _matrix(rng, 300, 20, np.float16)
    x[undefined] = 0.05                                 # the reference's CSVs hold probabilities
    got = au.calculate_prediction_entropy([list(map(float, r)) for r in x])
    np.testing.assert_allclose(got, entropy(x.astype(np.float64), base=2, axis=1), rtol=0, atol=1e-12)
    np.savetxt(tmp_path / "M.csv", x, delimiter=",")
    (tmp_path / "map.txt").write_text("ignore_uncommon False\ninclude_pdbs\n##########\n1abcA 100\n2defB 150\n1abcA 50\n")
    d = au.extract_prediction_entropy_to_dict(tmp_path / "M.csv", tmp_path / "map.txt")
    assert list(d) == ["1abcA", "2defB"]
    full = entropy(x.astype(np.float64), base=2, axis=1)
    np.testing.assert_allclose(d["1abcA"], np.concatenate([full[:100], full[250:]]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(d["2defB"], full[100:250], rtol=0, atol=1e-12)


# ---- predict.py --output_analysis end to end -----------------------------------------------------------------------------------
_ANALYSIS_FILES = ("_analysis.json", "_entropy.csv", "_per_structure.csv")


def _predict(model, data, out, **kw):
    import predict
    out.mkdir(exist_ok=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        predict.load_dataset_and_predict([model], data, batch_size=9, dataset_map_path=out / "datasetmap.txt", path_to_output=out, **kw)


def _rotamer_pack(tmp_path):
    from timed_hip import pack, synth
    cfg, weights = synth.timed_synth(338, widths=(8, 16), side=7, in_channels=5, seed=4, bias_std=0.1)
    mp = tmp_path / "ROT.pack"
    mp.write_bytes(pack.keras_to_pack(cfg, weights))
    return mp


@pytest.mark.parametrize("mode", ["residue", "rotamer"])
def test_predict_output_analysis_end_to_end(gpu, tmp_path, mode):
    from scipy.stats import entropy
    from timed_hip import textio
    data = os.path.join(G, "frames_tiny.hdf5")
    rot = mode == "rotamer"
    model = _rotamer_pack(tmp_path) if rot else Path(os.path.join(G, "keras_tiny.h5"))
    name = model.stem
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    _predict(model, data, plain, predict_rotamers=rot)
    _predict(model, data, flagged, predict_rotamers=rot, output_analysis=True)
    # every file of the run without the flag is byte-identical with it; the flag adds exactly the three analysis files
    before = {f.name for f in plain.iterdir()}
    assert not any(f.endswith(_ANALYSIS_FILES) for f in before)
    assert {f.name for f in flagged.iterdir()} == before | {name + s for s in _ANALYSIS_FILES}
    for fn in before:
        assert (plain / fn).read_bytes() == (flagged / fn).read_bytes(), fn
    m = json.loads((flagged / f"{name}_analysis.json").read_text())
    assert m["model"] == name and m["rotamer_mode"] is rot
    fasta = (flagged / f"{name}.fasta").read_text().split("\n")[1::2]
    real = (flagged / "dataset.fasta").read_text().split("\n")[1::2]
    pred_seq, real_seq = "".join(fasta), "".join(real)
    assert len(pred_seq) == len(real_seq) == 26
    assert m["accuracy_1"] == sum(a == b for a, b in zip(pred_seq, real_seq)) / 26
    assert sum(map(sum, m["confusion_counts"])) == 26 and m["n_labelled"] == 26 and m["n_residues"] == 26
    assert m["accuracy_1"] <= m["accuracy_2"] <= m["accuracy_3"] <= m["accuracy_5"] <= 1
    matrix = textio.loadtxt_f16(flagged / (f"{name}_rot.csv" if rot else f"{name}.csv"))
    assert matrix.shape == (26, 338 if rot else 20)
    want = entropy(matrix.astype(np.float64), base=2, axis=1)
    got = np.loadtxt(flagged / f"{name}_entropy.csv")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert (flagged / f"{name}_entropy.csv").read_bytes() == textio.format_csv(got)
    assert m["mean_entropy"] == pytest.approx(float(want.mean()), abs=1e-12)
    lines = (flagged / f"{name}_per_structure.csv").read_text().splitlines()
    assert lines[0] == "key,n_residues,n_labelled,accuracy,similarity,mean_entropy,std_entropy"
    assert [ln.split(",")[0] for ln in lines[1:]] == ["1ubqA", "2xyz_0A", "2xyz_0B"]
    assert sum(int(ln.split(",")[1]) for ln in lines[1:]) == 26


def test_predict_cli_output_analysis_and_sharded_run(gpu, tmp_path, monkeypatch):
    import predict
    from timed_hip import distributed as td
    data = os.path.join(G, "frames_tiny.hdf5")
    model = os.path.join(G, "keras_tiny.h5")
    cli = tmp_path / "cli"
    cli.mkdir()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        predict.main(predict.build_parser().parse_args(["--path_to_dataset", data, "--path_to_model", model, "--path_to_output",
                                                        str(cli), "--path_to_datasetmap", str(cli / "datasetmap.txt"),
                                                        "--batch_size", "9", "--output_analysis"]))
    for s in _ANALYSIS_FILES:
        assert (cli / f"keras_tiny{s}").exists(), s
    plain, sharded = tmp_path / "plain", tmp_path / "sharded"
    _predict(Path(model), data, plain, output_analysis=True)
    comm = td.RcclGather(td.RcclGather.new_unique_id(), 1, 0, gpu)
    try:
        _predict(Path(model), data, sharded, output_analysis=True, gather=comm, frames_per_call=9)
    finally:
        comm.close()
    for s in _ANALYSIS_FILES:
        assert (plain / f"keras_tiny{s}").read_bytes() == (sharded / f"keras_tiny{s}").read_bytes(), s
        assert (plain / f"keras_tiny{s}").read_bytes() == (cli / f"keras_tiny{s}").read_bytes(), s


def test_predict_output_analysis_on_a_count_map_writes_entropies_only(gpu, tmp_path):
    """a "<pdb> <count>" map carries no true residues: n_labelled 0, every metric null, entropies as usual"""
    data = os.path.join(G, "frames_tiny.hdf5")
    model = Path(os.path.join(G, "keras_tiny.h5"))
    first = tmp_path / "first"
    _predict(model, data, first)
    out = tmp_path / "counts"
    out.mkdir()
    # the same frames through a PDBench-style map of the keys and their row counts (the map predict.py writes as <model>.txt)
    fmap = np.atleast_2d(np.genfromtxt(first / "datasetmap.txt", delimiter=",", dtype=str))
    counts = {}
    for pdb, chain, _r, _res in fmap:
        counts[pdb + chain] = counts.get(pdb + chain, 0) + 1
    import predict
    from design_utils import utils as du
    matrix = np.loadtxt(first / "keras_tiny.csv", delimiter=",").astype(np.float16)
    plan = du.SequencePlan(np.array([[k, str(v)] for k, v in counts.items()]))
    predict._write_analysis(matrix, np.array([[k, str(v)] for k, v in counts.items()]), plan, "keras_tiny", out, False, None, gpu)
    m = json.loads((out / "keras_tiny_analysis.json").read_text())
    assert m["n_labelled"] == 0 and m["accuracy_1"] is None and m["recall"] is None and m["n_residues"] == 26
    assert np.loadtxt(out / "keras_tiny_entropy.csv").shape == (26,)
    lines = (out / "keras_tiny_per_structure.csv").read_text().splitlines()
    assert lines[1].split(",")[2:4] == ["0", "nan"]
