"""th_analyse_classes (csrc/class_analysis.hip) on the GPU: bit equality of every integer output with the NumPy restatement
(tests/class_analysis_restatement.py), the sklearn fixture (tests/golden/class_auc_golden.npz) through analyse_class_matrix at 1e-9,
ABI errors, and the reference-named surface end to end (calculate_rotamer_metrics, analyse_rotamers.py, predict.py --output_auc)."""
import ctypes as C
import json
import os
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_analysis_restatement as cr  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT_KEYS = ("pred", "rank", "confusion", "rank_hist", "scored_count", "pair_u2", "n_labelled", "n_nonfinite", "n_scored")


def _matrix(rng, n, k, dtype):
    """softmax rows with planted exact ties within and across rows, zeros, -0.0, negative entries, NaN and infinite rows"""
    z = rng.standard_normal((n, k)).astype(np.float32) * 2.5
    x = np.exp(z - z.max(axis=1, keepdims=True))
    x = (x / x.sum(axis=1, keepdims=True)).astype(dtype)
    if n == 0:
        return x
    rows = rng.permutation(n)
    cut = np.array_split(rows[: max(1, n // 2)], 8)
    for i in cut[0]:                                    # exact ties of the row maximum in other columns
        j = int(np.argmax(x[i]))
        x[i, rng.integers(0, k)] = x[i, j]
        x[i, (j + 1 + rng.integers(0, k - 1)) % k if k > 1 else j] = x[i, j]
    for i in cut[1]:                                    # zeros and negative zeros
        x[i, rng.integers(0, k, max(1, k // 3))] = 0
        x[i, rng.integers(0, k, max(1, k // 5))] = -0.0
    for i in cut[2]:                                    # few distinct values: ties between rows in every column
        x[i] = np.round(x[i].astype(np.float32) * 8) / 8
    for i in cut[3]:                                    # copies of other rows (they get labels of their own)
        x[i] = x[rows[rng.integers(0, n)]]
    for i in cut[4]:                                    # negative entries
        x[i, rng.integers(0, k, 2)] = -x[i].max() / 2 if x[i].max() > 0 else -1
    for i in cut[5][: max(1, len(cut[5]) // 2)]:        # NaN rows, one of them with the NaN in column 0
        x[i, rng.integers(0, k)] = np.nan
    for i in cut[5][len(cut[5]) // 2:]:                 # infinite rows, both signs
        x[i, rng.integers(0, k)] = np.inf if rng.random() < 0.5 else -np.inf
    if len(cut[5]):
        x[cut[5][0], 0] = np.nan
    return x


def _labels(rng, n, k, mode):
    """~10 % unlabelled; "uniform": every fifth class absent; "skewed": one class holds 90 % of the rows"""
    if mode == "skewed":
        t = np.where(rng.random(n) < 0.9, k // 2, rng.integers(0, k, n))
    else:
        allowed = np.array([c for c in range(k) if k <= 2 or c % 5 != 3])
        t = allowed[rng.integers(0, allowed.size, n)]
    t = t.astype(np.int16)
    t[rng.random(n) < 0.1] = -1
    return t


def _same(got, want, what=""):
    for key in INT_KEYS:
        g, w = (got[key] if isinstance(got, dict) else getattr(got, key)), (want[key] if isinstance(want, dict) else getattr(want, key))
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (key, what)
        else:
            assert g == w, (key, what)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("k", [2, 20, 338, 1024])
@pytest.mark.parametrize("n", [0, 1, 7, 1000, 5000])
def test_analyse_classes_matches_the_restatement_bit_for_bit(gpu, n, k, dtype):
    from timed_hip import analysis
    rng = np.random.default_rng(n * 11 + k + (1 if dtype == np.float16 else 0))
    x = _matrix(rng, n, k, dtype)
    for mode in ("uniform", "skewed"):
        t = _labels(rng, n, k, mode)
        got = analysis.analyse_classes(x, t, device=gpu)
        want = cr.restate(x, t)
        _same(got, want, mode)
        if n >= 1000:                                   # the inputs do hold what they are meant to
            assert got.n_nonfinite > 0 and got.n_scored < got.n_labelled < n and got.pair_u2.any()
            assert k == 2 or mode == "skewed" or (got.scored_count == 0).any()
        assert not np.diag(got.pair_u2).any()
        # a second call gives the same bytes; without the AUC sweep the other outputs are the same bytes
        _same(analysis.analyse_classes(x, t, device=gpu), got, mode)
        plain = analysis.analyse_classes(x, t, device=gpu, auc=False)
        assert plain.pair_u2 is None
        _same(plain._replace(pair_u2=got.pair_u2), got, mode)
        no_rows = analysis.analyse_classes(x, t, device=gpu, rows=False)
        assert no_rows.pred is None and no_rows.rank is None
        _same(no_rows._replace(pred=got.pred, rank=got.rank), got, mode)


def test_default_blocking_across_block_boundaries(gpu, monkeypatch):
    from timed_hip import analysis
    monkeypatch.delenv("TH_ANALYSIS_BLOCK_ROWS", raising=False)
    n, k = 2 * 262144 + 777, 64
    rng = np.random.default_rng(5)
    x = rng.random((n, k), dtype=np.float32).astype(np.float16)
    x[rng.integers(0, n, 500), rng.integers(0, k, 500)] = np.nan
    t = _labels(rng, n, k, "uniform")
    _same(analysis.analyse_classes(x, t, device=gpu), cr.restate(x, t))


def test_staging_blocks_do_not_change_a_byte(gpu, monkeypatch):
    from timed_hip import analysis
    rng = np.random.default_rng(12)
    for n, k, dtype in ((1000, 20, np.float16), (5003, 338, np.float16), (3001, 1024, np.float32)):
        x = _matrix(rng, n, k, dtype)
        t = _labels(rng, n, k, "uniform")
        monkeypatch.delenv("TH_ANALYSIS_BLOCK_ROWS", raising=False)
        whole = analysis.analyse_classes(x, t, device=gpu)
        _same(whole, cr.restate(x, t))
        for rows in ("97", "4096", "1"):
            if rows == "1" and n > 1000:
                continue
            monkeypatch.setenv("TH_ANALYSIS_BLOCK_ROWS", rows)
            _same(analysis.analyse_classes(x, t, device=gpu), whole, rows)


def _fixture_case(name):
    z = np.load(os.path.join(G, "class_auc_golden.npz"))
    x, y = cr.golden_matrix(name)
    assert cr.matrix_sha256(x) == str(z[f"{name}_sha256"]) and np.array_equal(y, z[f"{name}_labels"])
    return z, x, y


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fixture_float32_cases_through_analyse_class_matrix(gpu, name):
    from timed_hip import analysis
    z, x, y = _fixture_case(name)
    m = analysis.analyse_class_matrix(x, y, device=gpu)
    k = x.shape[1]
    print(name, "ovo", m["auc_ovo"], float(z[f"{name}_auc_ovo"]), "ovr", m["auc_ovr"], float(z[f"{name}_auc_ovr"]))
    assert abs(m["auc_ovo"] - float(z[f"{name}_auc_ovo"])) <= 1e-9
    if np.isnan(z[f"{name}_auc_ovr"]):
        assert m["auc_ovr"] is None and m["auc_ovr_present"] is not None and m["n_classes_present"] < k
    else:
        assert abs(m["auc_ovr"] - float(z[f"{name}_auc_ovr"])) <= 1e-9 and m["n_classes_present"] == k
    for kk in range(1, 6):
        assert abs(m[f"accuracy_{kk}"] - float(z[f"{name}_top_k"][kk - 1])) <= 1e-9
    assert 0.05 < m["accuracy_1"] < 0.95
    assert abs(m["precision"] - float(z[f"{name}_precision"])) <= 1e-9 and abs(m["recall"] - float(z[f"{name}_recall"])) <= 1e-9
    assert np.array_equal(np.array(m["confusion_counts"]), z[f"{name}_cm"])
    nz = z[f"{name}_cm_nonzero"]
    for key in ("unweighted", "weighted"):
        want = np.zeros(k * k)
        want[nz] = z[f"{name}_cm_{key}"]
        assert np.abs(np.array(m[f"{key}_cm"]).ravel() - want).max() <= 1e-9, key


def test_fixture_float16_case_through_analyse_class_matrix(gpu):
    from timed_hip import analysis
    z, x, y = _fixture_case("d")
    assert x.dtype == np.float16
    m = analysis.analyse_class_matrix(x, y, device=gpu)
    print("d ovo", m["auc_ovo"], float(z["d_auc_ovo"]))
    assert abs(m["auc_ovo"] - float(z["d_auc_ovo"])) <= 1e-9
    assert np.abs(np.array(m["auc_ovr_per_class"], dtype=np.float64) - z["d_ovr_per_class"]).max() <= 1e-9
    got = analysis.analyse_classes(x, y, device=gpu)
    cnt = got.scored_count.astype(np.float64)
    a, b = z["d_pairs"][:, 0].astype(int), z["d_pairs"][:, 1].astype(int)
    assert np.abs(got.pair_u2[a, b] / (2.0 * cnt[a] * cnt[b]) - z["d_pair_auc"]).max() <= 1e-9
    want = cr.restate(x, y)
    hits = np.cumsum(want["rank_hist"])
    for kk in range(1, 6):
        assert m[f"accuracy_{kk}"] == float(hits[kk - 1]) / want["n_labelled"]


def test_abi_errors_leave_the_device_usable(gpu):
    from timed_hip import _lib, analysis
    lib = _lib.load()
    k = 20
    x = np.full((4, k), 0.05, np.float32)
    t = np.zeros(4, np.int16)

    def call(mat=x, dtype=_lib.TH_F32, n=4, k=k, tr=t, conf=True, hist=True, scored=True, counts=True):
        kk = max(int(k), 1)
        bufs = [np.zeros(kk * kk, np.int64), np.zeros(kk + 1, np.int64), np.zeros(kk, np.int64)]
        cnt = analysis.ClassCounts()
        ptr = [b.ctypes.data_as(C.c_void_p) if on else None for b, on in zip(bufs, (conf, hist, scored))]
        rc = lib.th_analyse_classes(gpu, mat.ctypes.data_as(C.c_void_p), dtype, n, k, tr.ctypes.data_as(C.c_void_p), None, None,
                                    ptr[0], ptr[1], ptr[2], None, C.byref(cnt) if counts else None)
        return rc, lib.th_last_error().decode()
    assert call()[0] == 0
    for kw in (dict(dtype=_lib.TH_F64), dict(dtype=_lib.TH_U8), dict(k=0), dict(conf=False), dict(hist=False), dict(scored=False),
               dict(counts=False), dict(mat=np.zeros((1, 1025), np.float32), n=1, k=1025, tr=t[:1])):
        rc, msg = call(**kw)
        assert rc == _lib.TH_EINVAL and "th_analyse_classes" in msg, kw
    for bad in (k, -2):
        bad_t = t.copy()
        bad_t[2] = bad
        rc, msg = call(tr=bad_t)
        assert rc == _lib.TH_EINVAL and "true_class[2]" in msg
        with pytest.raises(_lib.TimedHipError):
            analysis.analyse_classes(x, bad_t, device=gpu)
    assert call()[0] == 0
    got = analysis.analyse_classes(x, t, device=gpu)
    assert got.n_labelled == 4 and got.confusion[0, 0] == 4


# ---- the reference-named surface, end to end -----------------------------------------------------------------------------------------
def _predict(model, data, out, **kw):
    import predict
    out.mkdir(exist_ok=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        predict.load_dataset_and_predict([model], data, batch_size=9, dataset_map_path=out / "datasetmap.txt", path_to_output=out, **kw)


def _rotamer_run(tmp_path):
    """prediction CSV of the synthetic 338-class model over the tiny frame set, its map, and a generated labels file"""
    from timed_hip import pack, synth
    cfg, weights = synth.timed_synth(338, widths=(8, 16), side=7, in_channels=5, seed=4, bias_std=0.1)
    mp = tmp_path / "ROT.pack"
    mp.write_bytes(pack.keras_to_pack(cfg, weights))
    out = tmp_path / "pred"
    _predict(mp, os.path.join(G, "frames_tiny.hdf5"), out, predict_rotamers=True)
    fmap = np.atleast_2d(np.genfromtxt(out / "datasetmap.txt", delimiter=",", dtype=str))
    rng = np.random.default_rng(2)
    labels = {}
    for pdb, chain, *_ in fmap:
        labels.setdefault(pdb + chain, []).append(int(rng.integers(0, 338)))
    first = next(iter(labels))
    labels[first][0] = None                             # an untagged residue
    lf = tmp_path / "labels.json"
    lf.write_text(json.dumps(labels))
    return out / "ROT_rot.csv", out / "datasetmap.txt", lf, labels


def _check_rotamer_outputs(out, suffix, matrix, flat, gpu):
    from design_utils import utils
    from timed_hip import analysis, textio
    want = analysis.analyse_class_matrix(matrix, flat, categories=utils.get_rotamer_codec()[1], device=gpu)
    got = json.loads((out / f"results_{suffix}.json").read_text())
    assert got == json.loads(json.dumps(want))
    text = (out / f"results_{suffix}.txt").read_text()
    for label in ("Metrics AUC_OVR:", "Metrics AUC_OVO:", "Accuracy:", "accuracy_2:", "accuracy_5:", "Report:", "Bias:"):
        assert label in text, label
    for kind in ("unweighted", "weighted"):
        cm = np.loadtxt(out / f"cm_{suffix}_{kind}.csv", delimiter=",")
        assert np.array_equal(cm, np.array(want[f"{kind}_cm"]))
        assert (out / f"cm_{suffix}_{kind}.csv").read_bytes() == textio.format_csv(np.array(want[f"{kind}_cm"]))


def test_calculate_rotamer_metrics_and_analyse_rotamers_cli_end_to_end(gpu, tmp_path):
    import analyse_rotamers
    from design_utils import analyse_utils as au, utils
    from timed_hip import textio
    csv, dmap, lf, labels = _rotamer_run(tmp_path)
    matrix = textio.loadtxt_f16(csv)
    assert matrix.shape == (26, 338) and matrix.dtype == np.float16
    # rows in the order the keys present them (a key's rows need not be consecutive in the map)
    plan = utils.SequencePlan(np.atleast_2d(np.genfromtxt(dmap, delimiter=",", dtype=str)))
    assert plan.keys == list(labels)
    matrix = matrix[np.concatenate([np.arange(26)[plan.rows(key)] for key in plan.keys])]
    flat = np.array([-1 if v is None else v for key in labels for v in labels[key]], dtype=np.int16)
    # the function, on a dict of lists
    lo, probs = 0, {}
    for key, v in labels.items():
        probs[key] = matrix[lo:lo + len(v)].tolist()
        lo += len(v)
    out = tmp_path / "fn"
    out.mkdir()
    res = au.calculate_rotamer_metrics(probs, {key: [np.nan if v is None else v for v in vals] for key, vals in labels.items()},
                                       utils.get_rotamer_codec()[1], "fn", out)
    assert res["n_labelled"] == 25 and res["n_rows"] == 26
    _check_rotamer_outputs(out, "fn", matrix, flat, gpu)
    # the command line
    cli = tmp_path / "cli"
    analyse_rotamers.main(analyse_rotamers.build_parser().parse_args([
        "--path_to_pred_matrix", str(csv), "--path_to_datasetmap", str(dmap), "--output_path", str(cli),
        "--path_to_rotamer_labels", str(lf), "--device", str(gpu), "--support_old_datasetmap"]))
    _check_rotamer_outputs(tmp_path / "cli_ROT_rot", "ROT_rot_vs_original", matrix, flat, gpu)


def test_predict_output_auc(gpu, tmp_path):
    from timed_hip import analysis, textio
    data = os.path.join(G, "frames_tiny.hdf5")
    model = Path(os.path.join(G, "keras_tiny.h5"))
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    _predict(model, data, plain)
    _predict(model, data, flagged, output_auc=True)
    before = {f.name for f in plain.iterdir()}
    assert "keras_tiny_auc.json" not in before
    assert {f.name for f in flagged.iterdir()} == before | {"keras_tiny_auc.json"}
    for fn in before:
        assert (plain / fn).read_bytes() == (flagged / fn).read_bytes(), fn
    matrix = textio.loadtxt_f16(flagged / "keras_tiny.csv")
    fmap = np.atleast_2d(np.genfromtxt(flagged / "datasetmap.txt", delimiter=",", dtype=str))
    truth = analysis.residue_indices(fmap[:, 3]).astype(np.int16)
    want = cr.restate(matrix, truth)
    auc = analysis.roc_auc_from_pairs(want["pair_u2"], want["scored_count"])
    got = json.loads((flagged / "keras_tiny_auc.json").read_text())
    assert got["n_scored"] == want["n_scored"] == 26
    for key, v in auc.items():
        assert got[key] == v, key
    # rotamer mode points at analyse_rotamers.py
    with pytest.raises(ValueError, match="analyse_rotamers.py"):
        _predict(model, data, tmp_path / "rot", predict_rotamers=True, output_auc=True)
