"""predict.py over a directory of structures (timed_hip/structureset.py): the frames of every call group are voxelised in HBM by one
th_voxelise_batch call.  A directory that holds one file against that file given directly; three files with call groups that start
and end inside structures against the three single-file runs; the charge channel with a 6-channel model, a property map, and the
refusal of a model whose input channels do not fit."""
import gzip
import json
import os
import shutil
import warnings
from pathlib import Path

import numpy as np
import pytest

from timed_hip import pack, structureset, synth, voxeliser

pytestmark = pytest.mark.gpu

UBQ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "1ubq.pdb1.gz")
FILES = ("M.csv", "M.fasta", "M.txt", "dataset.fasta", "datasetmap.txt", "encoded_labels.csv")


def _model(path, channels):
    cfg, weights = synth.timed_synth(20, widths=(8, 16), side=21, in_channels=channels, seed=3)
    path.write_bytes(pack.keras_to_pack(cfg, weights))
    return path


def _predict(model, dataset, out, gpu, **kw):
    import predict
    out.mkdir()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return predict.load_dataset_and_predict([model], dataset, dataset_map_path=out / "datasetmap.txt", path_to_output=out, device=gpu, **kw)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """{input channels: pack}, both called M"""
    return {c: _model(tmp_path_factory.mktemp(f"model{c}") / "M.pack", c) for c in (5, 6)}


@pytest.fixture(scope="module")
def three_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("structures")
    shutil.copy(UBQ, d / "1ubq.pdb1.gz")
    with gzip.open(UBQ, "rt") as f:
        text = f.read()
    (d / "cut40.pdb").write_text("".join(ln + "\n" for ln in text.splitlines() if ln.startswith("ATOM") and 1 <= int(ln[22:26]) <= 40) + "END\n")
    shutil.copy(UBQ, d / "zcopy.pdb.gz")
    return d


def test_a_directory_of_one_file_equals_the_file(gpu, models, tmp_path):
    d = tmp_path / "one"
    d.mkdir()
    shutil.copy(UBQ, d / "1ubq.pdb1.gz")
    _predict(models[5], d, tmp_path / "a", gpu, batch_size=16, frames_per_call=32)
    _predict(models[5], UBQ, tmp_path / "b", gpu, batch_size=16, frames_per_call=32)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(FILES)
    for fn in FILES:
        assert (tmp_path / "a" / fn).read_bytes() == (tmp_path / "b" / fn).read_bytes(), fn
    assert (tmp_path / "a" / "M.txt").read_text().endswith("1ubqA 76\n")


def test_three_files_with_groups_that_cut_through_structures(gpu, models, three_files, tmp_path, monkeypatch):
    seen = []
    real = structureset.StructureSet.device_batch

    def spy(self, rows, device, pool):
        X, y = real(self, rows, device, pool)
        seen.append((tuple(str(v) for v in rows[0][:3]), X.buffer.download(X.shape, X.dtype), X.device))
        return X, y
    monkeypatch.setattr(structureset.StructureSet, "device_batch", spy)
    res = _predict(models[5], three_files, tmp_path / "set", gpu, batch_size=16, frames_per_call=64)
    names = ("1ubq.pdb1.gz", "cut40.pdb", "zcopy.pdb.gz")
    singles = [tmp_path / f"single{k}" for k in range(3)]
    for name, out in zip(names, singles):
        _predict(models[5], three_files / name, out, gpu, batch_size=16, frames_per_call=64)
    out = tmp_path / "set"
    assert sorted(p.name for p in out.iterdir()) == sorted(FILES)
    assert [len(res[1][k]) for k in ("1ubqA", "cut40A", "zcopyA")] == [76, 40, 76]
    for fn in ("datasetmap.txt", "dataset.fasta"):
        assert (out / fn).read_text() == "".join((s / fn).read_text() for s in singles), fn
    head = "ignore_uncommon False\ninclude_pdbs\n##########\n"
    assert (out / "M.txt").read_text() == head + "".join((s / "M.txt").read_text()[len(head):] for s in singles)
    got = np.loadtxt(out / "M.csv", delimiter=",")
    want = np.concatenate([np.loadtxt(s / "M.csv", delimiter=",") for s in singles])
    assert got.shape == want.shape == (192, 20)
    step = np.spacing(np.maximum(want, 2.0 ** -14).astype(np.float16)).astype(np.float64)
    print(f"M.csv: {float(np.mean(got == want)):.4f} of the values equal, worst difference in float16 steps {float((np.abs(got - want) / step).max()):.2f}")
    assert np.all(np.abs(got - want) <= step) and np.mean(got == want) > 0.99
    # three groups of 64 frames: 1ubq ends at 76, cut40 at 116 — and each group's frames, as they lay in HBM, are voxelise_pdb's
    flat = [r for name in names for r in voxeliser.voxelise_pdb(three_files / name, device=gpu)[2]]
    frames = np.concatenate([voxeliser.voxelise_pdb(three_files / name, device=gpu)[0] for name in names])
    assert [len(x) for _, x, _ in seen] == [64, 64, 64] and all(dev == gpu for _, _, dev in seen)
    assert [first for first, _, _ in seen] == [flat[k][:3] for k in (0, 64, 128)]
    assert np.concatenate([x for _, x, _ in seen]).tobytes() == frames.tobytes()


def test_charge_channel_with_a_six_channel_model(gpu, models, three_files, tmp_path):
    import predict
    out = tmp_path / "native"
    out.mkdir()
    args = predict.build_parser().parse_args(["--path_to_dataset", UBQ, "--path_to_model", str(models[6]), "--path_to_output", str(out),
                                              "--path_to_datasetmap", str(out / "datasetmap.txt"), "--property", "charge", "--batch_size", "16",
                                              "--device", str(gpu)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        predict.main(args)
    fasta = (out / "M.fasta").read_text().split("\n")
    assert fasta[0] == ">1ubqA" and len(fasta[1]) == 76
    native = np.loadtxt(out / "M.csv", delimiter=",")
    assert native.shape == (76, 20) and np.all(np.abs(native.sum(1) - 1.0) < 2e-2)
    # residue 1 (MET, charge 0) set to +1: its own frame changes
    values = [0] * 76
    from design_utils import utils as du
    values[:] = du.convert_seq_to_property((out / "dataset.fasta").read_text().split("\n")[1], "charge")
    assert values[0] == 0
    values[0] = 1
    (tmp_path / "map.json").write_text(json.dumps({"1ubq": values}))
    _predict(models[6], UBQ, tmp_path / "mapped", gpu, batch_size=16, property="charge", property_map=str(tmp_path / "map.json"))
    mapped = np.loadtxt(tmp_path / "mapped" / "M.csv", delimiter=",")
    assert (mapped[0] != native[0]).any()
    assert (tmp_path / "mapped" / "dataset.fasta").read_bytes() == (out / "dataset.fasta").read_bytes()
    # a file given without a property afterwards is the plain single-file dataset again
    _predict(models[5], UBQ, tmp_path / "plain", gpu, batch_size=16)
    assert np.loadtxt(tmp_path / "plain" / "M.csv", delimiter=",").shape == (76, 20)
    # channels that do not fit: refused before a frame is built
    built = []
    real = voxeliser.voxelise_batch
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(voxeliser, "voxelise_batch", lambda *a, **kw: built.append(1) or real(*a, **kw))
        for model, kw in ((models[5], dict(property="charge")), (models[6], {})):
            with pytest.raises(ValueError) as err:
                _predict(model, three_files, tmp_path / f"refused{len(kw)}", gpu, batch_size=16, **kw)
            print(err.value)
            assert "5" in str(err.value) and "6" in str(err.value) and "channels" in str(err.value)
    assert not built
