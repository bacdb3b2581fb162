"""th_voxelise_batch, the property channel and structure sets without a GPU: the header prototype against the ctypes entry, every
refusal of the call and of th_voxelise, its one-structure case (all decided on the host), the charge / polarity tables against what the reference pins, the property-aware
preparation of 1ubq, property-map validation, a set of three files, and predict.py over a directory with the batch call replaced by
its restatement (tests/voxel_weight_restatement.py) and a model double."""
import ctypes as C
import gzip
import json
import os
import re
from pathlib import Path

import numpy as np
import pytest

import voxel_cases as vc
import voxel_weight_restatement as vw
from design_utils import amino_acids, utils as du
from oracle import voxel_oracle
from timed_hip import _lib, pdbio, structureset, voxeliser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UBQ = os.path.join(ROOT, "tests", "golden", "1ubq.pdb1.gz")
UBQ_SEQ = "MQIFVKTLTGKTITLEVEPSDTIENVKAKIQDKEGIPPDQQRLIFAGKQLEDGRTLSDYNIQKESTLHLVLRLRGG"      # tests/test_voxeliser.py:138
PHRASE = "PARITY UNPINNED AGAINST AMPAL AND APOSTERIORI"


def cut_ubq(path, lo, hi):
    """ATOM lines of residues lo..hi of 1ubq as a plain .pdb"""
    with gzip.open(UBQ, "rt") as f:
        lines = [ln for ln in f if ln.startswith("ATOM") and lo <= int(ln[22:26]) <= hi]
    Path(path).write_text("".join(lines) + "END\n")
    return path


@pytest.fixture(scope="module")
def ubq():
    return pdbio.read_pdb(UBQ)[0]


# ---- 1. prototype ----------------------------------------------------------------------------------------------------------------
_CTYPES = {"int": "c_int", "int64_t": "c_long", "float": "c_float", "const float*": "c_void_p", "const int32_t*": "c_void_p",
           "const int64_t*": "c_void_p", "void*": "c_void_p", "double*": ("c_void_p", "LP_c_double")}


def test_header_prototype_ctypes_entry_build_list_and_phrase(lib):
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    m = re.search(r"^(\w+) th_voxelise_batch\(([^;]*)\);", header, re.M)
    assert m
    res, args = _lib.PROTOTYPES["th_voxelise_batch"]
    assert res.__name__ == _CTYPES[m.group(1)]
    declared = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in m.group(2).split(",")]
    assert len(declared) == len(args) == 18, (declared, args)
    for c_type, ct in zip(declared, args):
        want = _CTYPES[c_type]
        assert ct.__name__ in (want if isinstance(want, tuple) else (want,)), (c_type, ct)
    before = header[:m.start()]
    block = re.sub(r"[\s*]+", " ", before[before.rindex("/* ----"):])
    for words in (PHRASE, "weight (w / total)", "byte for byte", "no float atomics", "no device-wide synchronise", "TH_EUNSUP", "2048"):
        assert words in block, words
    assert hasattr(lib, "th_voxelise_batch")
    import __graft_entry__
    # one unit holds the one kernel and the one host path of th_voxelise and th_voxelise_batch
    csrc = os.path.join(ROOT, "timed-design_amd", "csrc")
    assert "voxelise_batch.hip" not in __graft_entry__.HIP_SOURCES and "voxelise.hip" in __graft_entry__.HIP_SOURCES
    assert "voxelise_batch.hip" not in os.listdir(csrc) and hasattr(lib, "th_voxelise")
    source = open(os.path.join(csrc, "voxelise.hip")).read()
    assert source.count("__global__") == 1 and "hipDeviceSynchronize" not in source and "hipStreamNonBlocking" in source
    # the only atomics are on integers in LDS (plane counts) and on the overflow flag: none on frame data
    assert sorted(set(re.findall(r"atomic\w+\([^,]*,", source))) == ["atomicAdd(&Ps[((Li[e] >> 18) & 511) + 1],", "atomicMax(p.overflow,"]
    assert "__shared__ int Ps[" in source and "int* overflow" in source
    readme = open(os.path.join(ROOT, "README.md")).read()
    for text in (voxeliser.__doc__, structureset.__doc__, readme, open(amino_acids.__file__).read(), du.convert_seq_to_property.__doc__):
        assert PHRASE in re.sub(r"\s+", " ", text)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_decided_without_a_gpu(lib):
    xyz, chn, sig, wgt = np.zeros((4, 3), np.float32), np.zeros(4, np.int32), np.ones(4, np.float32), np.ones(4, np.float32)
    off, fst = np.array([0, 3, 4], np.int64), np.array([0, 1, 1], np.int32)
    frt = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (3, 1))
    out = np.full((3, 3, 3, 3, 2), 7, np.float32)
    nan, inf = float("nan"), float("inf")

    def call(xyz=xyz, chn=chn, sig=sig, wgt=None, n_atoms=4, off=off, n_str=2, frt=frt, fst=fst, n_frames=3, V=3, edge=3.0, channels=2, gaussian=1,
             out=out):
        ms = C.c_double(-1.0)
        rc = lib.th_voxelise_batch(0, _lib.ptr(xyz), _lib.ptr(chn), _lib.ptr(sig), _lib.ptr(wgt), n_atoms, _lib.ptr(off), n_str, _lib.ptr(frt),
                                   _lib.ptr(fst), n_frames, V, edge, channels, gaussian, _lib.ptr(out), 0, C.byref(ms))
        return rc

    def weights(v):
        w = wgt.copy()
        w[2] = v
        return w
    einval = {"xyz NULL": dict(xyz=None), "channel NULL": dict(chn=None), "sigma NULL, Gaussian": dict(sig=None), "offsets NULL": dict(off=None),
              "frames_rt NULL": dict(frt=None), "frame_structure NULL": dict(fst=None), "out NULL": dict(out=None),
              "negative atoms": dict(n_atoms=-1), "negative structures": dict(n_str=-1), "negative frames": dict(n_frames=-1),
              "offsets start": dict(off=np.array([1, 3, 4], np.int64)), "offsets decrease": dict(off=np.array([0, 5, 4], np.int64)),
              "offsets end": dict(off=np.array([0, 3, 5], np.int64)), "offsets end before n_atoms": dict(off=np.array([0, 3, 3], np.int64)),
              "structure -1": dict(fst=np.array([0, -1, 1], np.int32)), "structure 2 of 2": dict(fst=np.array([0, 1, 2], np.int32)),
              "weights with boolean frames": dict(wgt=wgt, gaussian=0), "weight nan": dict(wgt=weights(nan)), "weight inf": dict(wgt=weights(inf)),
              "weight -inf": dict(wgt=weights(-inf)), "even side": dict(V=4), "side 0": dict(V=0), "side 513": dict(V=513),
              "edge 0": dict(edge=0.0), "edge negative": dict(edge=-3.0), "edge nan": dict(edge=nan)}
    for what, kw in einval.items():
        assert call(**kw) == _lib.TH_EINVAL, what
        assert b"th_voxelise_batch" in lib.th_last_error(), what
    for channels in (0, 9, -1):
        assert call(channels=channels) == _lib.TH_EUNSUP, channels
        assert b"th_voxelise_batch" in lib.th_last_error()
    assert not (out != 7).any()                                           # nothing was written
    # zero frames: TH_OK without a launch, with and without atoms
    assert call(n_frames=0, frt=None, fst=None, out=None) == _lib.TH_OK
    assert call(n_frames=0, frt=None, fst=None, out=None, n_atoms=0, xyz=None, chn=None, sig=None, off=np.array([0], np.int64), n_str=0) == _lib.TH_OK
    # sigma may be NULL for boolean frames, and the Python wrapper refuses disagreeing lengths itself
    assert call(n_frames=0, frt=None, fst=None, out=None, sig=None, gaussian=0) == _lib.TH_OK
    with pytest.raises(ValueError, match="lengths disagree"):
        voxeliser.voxelise_batch(xyz, chn, sig, wgt[:3], off, frt, fst, 3, 3.0, 2)


def test_th_voxelise_refuses_on_the_host_under_its_own_name(lib):
    """the one-structure entry point shares the batch call's refusals, all of them before the first HIP call"""
    xyz, chn, sig = np.zeros((4, 3), np.float32), np.zeros(4, np.int32), np.ones(4, np.float32)
    frt = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], np.float32)
    out = np.full((1, 3, 3, 3, 2), 7, np.float32)
    nan = float("nan")

    def call(xyz=xyz, chn=chn, sig=sig, n_atoms=4, frt=frt, n_res=1, V=3, edge=3.0, channels=2, gaussian=1, out=out):
        return lib.th_voxelise(0, _lib.ptr(xyz), _lib.ptr(chn), _lib.ptr(sig), n_atoms, _lib.ptr(frt), n_res, V, edge, channels, gaussian,
                               _lib.ptr(out), 0)
    einval = {"even side": dict(V=4), "side 0": dict(V=0), "side 513": dict(V=513), "edge 0": dict(edge=0.0), "edge negative": dict(edge=-3.0),
              "edge nan": dict(edge=nan), "negative atoms": dict(n_atoms=-1), "negative frames": dict(n_res=-1), "frames_rt NULL": dict(frt=None),
              "out NULL": dict(out=None), "xyz NULL": dict(xyz=None), "channel NULL": dict(chn=None), "sigma NULL, Gaussian": dict(sig=None),
              "2^31 frames": dict(n_res=2 ** 31)}
    for what, kw in einval.items():
        assert call(**kw) == _lib.TH_EINVAL, what
        assert b"th_voxelise" in lib.th_last_error() and b"th_voxelise_batch" not in lib.th_last_error(), what
    for channels in (0, 9):
        assert call(channels=channels) == _lib.TH_EUNSUP, channels
        assert b"th_voxelise" in lib.th_last_error() and b"th_voxelise_batch" not in lib.th_last_error()
    assert not (out != 7).any()                                           # nothing was written
    assert call(n_res=0) == _lib.TH_OK and call(n_res=0, frt=None, out=None) == _lib.TH_OK
    assert call(n_res=0, sig=None, gaussian=0) == _lib.TH_OK
    assert not (out != 7).any()


# ---- 3, 4. tables ----------------------------------------------------------------------------------------------------------------
def test_tables_agree_with_what_the_reference_pins():
    pinned = {0: "A", 1: "K", -1: "D"}                                    # reference design_utils/utils.py:86
    for value, letter in pinned.items():
        assert amino_acids.residue_charge[letter] == value
    assert amino_acids.residue_polarity["A"] == 0 and amino_acids.residue_polarity["K"] == 1
    assert {r for r, v in amino_acids.residue_charge.items() if v == -1} == set("DECY")
    assert {r for r, v in amino_acids.residue_charge.items() if v == 1} == set("KRH")
    assert {r for r, v in amino_acids.residue_polarity.items() if v == 1} == set("RDEHK")
    assert {r for r, v in amino_acids.polarity_Zimmerman.items() if v >= 20} == set("RDEHK")
    for table in (amino_acids.residue_charge, amino_acids.residue_polarity, amino_acids.polarity_Zimmerman):
        assert sorted(table) == sorted(amino_acids.standard_amino_acids)


def test_convert_seq_to_property_on_ubiquitin():
    charge = du.convert_seq_to_property(UBQ_SEQ, "charge")
    assert len(charge) == 76 and charge.count(1) == 12 and charge.count(-1) == 12 and charge.count(0) == 52
    assert UBQ_SEQ[58] == "Y" and charge[58] == -1                        # Y59
    polar = du.convert_seq_to_property(UBQ_SEQ, "polarity")
    assert sum(polar) == 23 and set(polar) == {0, 1}
    assert du.convert_seq_to_property("AXK", "polarity") == [0, 0, 1]
    with pytest.raises(KeyError):
        du.convert_seq_to_property("AXK", "charge")
    with pytest.raises(AssertionError, match="Property hydrophobicity not found among \\['polarity', 'charge'\\]"):
        du.convert_seq_to_property("A", "hydrophobicity")


# ---- 5, 6. preparation and maps ---------------------------------------------------------------------------------------------------
def test_property_preparation_of_1ubq(ubq):
    xyz0, ch0, sg0, frt0, rows0 = voxeliser.prepare_structure(ubq)
    xyz, ch, sg, wt, frt, rows = voxeliser.prepare_structure_with_property(ubq, "charge")
    extra = ch == 5
    assert int(extra.sum()) == 24 and len(xyz) == len(xyz0) + 24
    assert np.array_equal(xyz[~extra], xyz0) and np.array_equal(ch[~extra], ch0) and np.array_equal(sg[~extra], sg0)
    assert np.array_equal(frt, frt0) and rows == rows0 and np.all(wt[~extra] == 1)
    native = np.array(du.convert_seq_to_property(UBQ_SEQ, "charge"))
    assert wt[extra].tolist() == native[native != 0].astype(float).tolist() and np.all(sg[extra] == np.float32(0.85))
    # each sits at its residue's CA, directly behind the residue's own atoms (N, CA, C, O, CB)
    charged = [r for r in ubq.residues if not r.hetero and native[int(r.number) - 1] != 0]
    assert np.array_equal(xyz[extra], np.array([r.atoms["CA"] for r in charged], np.float32))
    where = np.nonzero(extra)[0]
    assert np.all(ch[where - 1] == 4) and np.array_equal(xyz[where], xyz[where - 4])
    # a map of zeros adds none; a map of ones adds one per frame; without a property the weights are all 1
    zero = voxeliser.prepare_structure_with_property(ubq, "charge", [0] * 76)
    assert np.array_equal(zero[0], xyz0) and np.array_equal(zero[1], ch0) and np.all(zero[3] == 1) and zero[5] == rows0
    ones = voxeliser.prepare_structure_with_property(ubq, "polarity", [1] * 76)
    assert int((ones[1] == 5).sum()) == 76 and np.array_equal(ones[0][ones[1] == 5], frt0[:, 9:])
    plain = voxeliser.prepare_structure_with_property(ubq)
    assert np.array_equal(plain[0], xyz0) and np.all(plain[3] == 1) and len(plain[3]) == len(xyz0)
    assert voxeliser.property_encoder("charge") == ("C", "N", "O", "CA", "CB", "Q") and voxeliser.property_encoder("polarity")[-1] == "P"


def test_property_maps_are_validated_and_read(ubq, tmp_path):
    for bad, words in (([0] * 75, ("1ubq", "75", "76")), ([0] * 75 + [2], ("1ubq", "2", "75")), ([1.0] * 76, ("1ubq",))):
        with pytest.raises(ValueError) as err:
            voxeliser.prepare_structure_with_property(ubq, "charge", bad, name="1ubq")
        assert all(w in str(err.value) for w in words), err.value
    with pytest.raises(ValueError, match="-1"):
        voxeliser.prepare_structure_with_property(ubq, "polarity", [-1] + [0] * 75, name="1ubq")
    voxeliser.prepare_structure_with_property(ubq, "charge", [-1] + [0] * 75, name="1ubq")
    (tmp_path / "a.json").write_text(json.dumps({"1ubq": [1] * 76, "other": [0]}))
    (tmp_path / "b.json").write_text(json.dumps([0] * 76))
    both = voxeliser.read_property_map(tmp_path / "a.json")
    assert voxeliser.map_of(both, "1ubq") == [1] * 76 and voxeliser.map_of(both, "absent") is None
    assert voxeliser.map_of(voxeliser.read_property_map(tmp_path / "b.json"), "anything") == [0] * 76
    (tmp_path / "c.json").write_text("3")
    with pytest.raises(ValueError):
        voxeliser.read_property_map(tmp_path / "c.json")
    # boolean frames carry no weight
    with pytest.raises(ValueError, match="Gaussian"):
        voxeliser.voxelise_pdb(UBQ, gaussian=False, property="charge")
    with pytest.raises(ValueError, match="Gaussian"):
        structureset.StructureSet(UBQ, property="charge", gaussian=False)


def test_restatement_equals_the_oracle_at_unit_weights():
    case = vc.sweep_gaussian(9, 12.5, 8)
    want = voxel_oracle.voxelise(*case.cloud, case.V, case.edge, case.C, True)
    got, mass = vw.voxelise_weighted(*case.cloud[:3], None, case.cloud.frt, case.V, case.edge, case.C)
    print("bytes equal:", got.tobytes() == want.tobytes())
    assert want.any() and np.array_equal(got != 0, want != 0)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    assert np.array_equal(got, mass)


# ---- 7. a set of three files ------------------------------------------------------------------------------------------------------
@pytest.fixture
def three_files(tmp_path):
    d = tmp_path / "set"
    d.mkdir()
    cut_ubq(d / "zeta.pdb", 30, 45)
    cut_ubq(d / "alpha.pdb", 1, 20)
    with gzip.open(d / "mid.pdb.gz", "wt") as f:
        f.write(Path(cut_ubq(tmp_path / "tmp.pdb", 50, 60)).read_text())
    return d


def test_structure_set_of_three_files(three_files, tmp_path, monkeypatch):
    monkeypatch.setattr(voxeliser, "voxelise_batch",
                        lambda xyz, ch, sg, wt, off, frt, fst, V, edge, C_, g, dev: np.zeros((len(frt), V, V, V, C_), np.float32))
    sset = structureset.StructureSet(three_files)
    assert sset.codes == ["alpha", "mid", "zeta"] and sset.n_channels == 5 and sset.frame_dims == (21, 21, 21, 5)
    rows = []
    for name in ("alpha.pdb", "mid.pdb.gz", "zeta.pdb"):
        rows += voxeliser.voxelise_pdb(three_files / name)[2]
    assert [tuple(r) for r in sset.flat_map.tolist()] == rows and len(rows) == 20 + 11 + 16
    assert sset.labels.shape == (47, 20) and np.all(sset.labels.sum(1) == 1)
    assert sset.row_offsets.tolist() == [0, 20, 31, 47] and sset.atom_offsets.tolist() == [0, 100, 155, 235]
    # the arrays of one call: only the structures the rows touch, frames in the order asked for
    got = sset.batch_arrays(np.array([40, 3, 41]))
    assert got["atom_offsets"].tolist() == [0, 100, 180] and got["frame_structure"].tolist() == [1, 0, 1]
    assert np.array_equal(got["frames_rt"], sset.frt[[40, 3, 41]]) and got["atom_weight"] is None
    assert np.array_equal(got["atoms_xyz"], np.concatenate([sset.xyz[:100], sset.xyz[155:]]))
    assert sset.rows_of(sset.flat_map[18:33]).tolist() == list(range(18, 33))
    assert sset.rows_of(sset.flat_map[[5, 46, 20]]).tolist() == [5, 46, 20]
    # the same through design_utils
    assert du.structure_set_of(three_files / "alpha.pdb") is None
    fmap, pdbs = du.create_flat_dataset_map(three_files)
    assert fmap == rows and pdbs == {"alpha", "mid", "zeta"}
    assert np.array_equal(du.flat_dataset_map_array(three_files), sset.flat_map)
    # two files with one code
    cut_ubq(three_files / "mid.pdb", 1, 5)
    with pytest.raises(ValueError) as err:
        structureset.StructureSet(three_files)
    assert "mid.pdb.gz" in str(err.value) and "mid.pdb " in str(err.value) + " "
    (three_files / "mid.pdb").unlink()
    with pytest.raises(ValueError, match="single structure"):
        structureset.StructureSet(three_files, property="charge", property_map=[0] * 20)
    with pytest.raises(ValueError, match="alpha.*19.*20"):
        structureset.StructureSet(three_files, property="charge", property_map={"alpha": [0] * 19})


# ---- 8. predict.py over a directory ----------------------------------------------------------------------------------------------
class _Ticket:
    def __init__(self, X):
        s = np.asarray(X, np.float64).reshape(len(X), -1).sum(axis=1)
        rows = np.cos(np.arange(1, 21)[None, :] * s[:, None]) ** 2 + 1e-3
        self.value = (rows / rows.sum(axis=1, keepdims=True)).astype(np.float32)

    def result(self):
        return self.value


class Double:
    """a model without a device: the loader hands it host frames"""
    n_classes = 20
    shapes = []

    def __init__(self, path, device=0):
        pass

    def predict_async(self, X):
        assert isinstance(X, np.ndarray)
        Double.shapes.append(X.shape)
        return _Ticket(X)

    def close(self):
        pass


def _restated_batch(atoms_xyz, atom_channel, atom_sigma, atom_weight, atom_offsets, frames_rt, frame_structure, voxels_per_side=21,
                    frame_edge_length=21.0, n_channels=5, gaussian=True, device=0, d_out=None, timing=None):
    assert d_out is None
    return vw.batch(atoms_xyz, atom_channel, atom_sigma, atom_weight, atom_offsets, frames_rt, frame_structure, voxels_per_side,
                    frame_edge_length, n_channels, gaussian)[0]


def test_predict_py_over_a_directory(three_files, tmp_path, monkeypatch):
    import predict
    parser = predict.build_parser()
    args = parser.parse_args(["--path_to_dataset", str(three_files), "--property", "charge", "--path_to_property_map", "m.json"])
    assert args.property == "charge" and args.path_to_property_map == "m.json" and parser.parse_args([]).property is None
    with pytest.raises(SystemExit):
        parser.parse_args(["--property", "mass"])
    assert PHRASE in re.sub(r"\s+", " ", parser.format_help())
    monkeypatch.setattr(voxeliser, "voxelise_batch", _restated_batch)
    files = ("M.csv", "M.fasta", "M.txt", "dataset.fasta", "datasetmap.txt", "encoded_labels.csv")

    def run(name, **kw):
        out = tmp_path / name
        out.mkdir()
        Double.shapes = []
        res = predict.load_dataset_and_predict([Path("M.pack")], three_files, batch_size=4, frames_per_call=12, path_to_output=out,
                                               dataset_map_path=out / "datasetmap.txt", model_loader=Double, **kw)
        assert sorted(p.name for p in out.iterdir()) == sorted(files)
        return out, res
    out, res = run("plain")
    sset = du.structure_set_of(three_files)
    assert [s[0] for s in Double.shapes] == [12, 12, 12, 11] and all(s[1:] == (21, 21, 21, 5) for s in Double.shapes)
    assert (out / "datasetmap.txt").read_text() == "".join(",".join(r) + "\n" for r in sset.flat_map.tolist())
    assert (out / "dataset.fasta").read_text() == f">alphaA\n{UBQ_SEQ[:20]}\n>midA\n{UBQ_SEQ[49:60]}\n>zetaA\n{UBQ_SEQ[29:45]}\n"
    assert (out / "M.txt").read_text().endswith("alpha 20\nmid 11\nzetaA 16\n")      # (the chain is appended to four-letter codes only)
    assert np.array_equal(np.loadtxt(out / "encoded_labels.csv", delimiter=","), sset.labels)
    # groups of 12 start and end inside structures: the rows equal those of every structure voxelised alone
    alone = np.concatenate([_Ticket(vw.voxelise_weighted(sset.xyz[a:b], sset.chn[a:b], sset.sig[a:b], None, sset.frt[r:s])[0]).value
                            for a, b, r, s in zip(sset.atom_offsets[:-1], sset.atom_offsets[1:], sset.row_offsets[:-1], sset.row_offsets[1:])])
    assert np.array_equal(np.loadtxt(out / "M.csv", delimiter=",").astype(np.float16), alone.astype(np.float16))
    assert list(res[1]) == ["alphaA", "midA", "zetaA"] and [len(v) for v in res[1].values()] == [20, 11, 16]
    # a charge channel: six channels reach the model, labels and sequences keep the native residues, a map changes its rows only
    out_q, _ = run("charge", property="charge")
    assert all(s[1:] == (21, 21, 21, 6) for s in Double.shapes)
    flipped = {"mid": [1] * 11}
    (tmp_path / "map.json").write_text(json.dumps(flipped))
    out_m, _ = run("mapped", property="charge", property_map=str(tmp_path / "map.json"))
    for fn in ("dataset.fasta", "datasetmap.txt", "encoded_labels.csv", "M.txt"):
        assert (out_q / fn).read_bytes() == (out / fn).read_bytes() == (out_m / fn).read_bytes(), fn
    plain, native, mapped = (np.loadtxt(o / "M.csv", delimiter=",") for o in (out, out_q, out_m))
    assert (plain != native).any(axis=1).sum() > 30
    changed = (native != mapped).any(axis=1)
    assert changed[20:31].all() and changed.sum() == 11                   # every frame of mid sees new atoms, no frame of another structure does
    # refusals
    with pytest.raises(ValueError, match="nmr"):
        predict.load_dataset_and_predict([Path("M.pack")], three_files, is_consensus=True, path_to_output=tmp_path, model_loader=Double)
    with pytest.raises(ValueError, match="property"):
        predict.load_dataset_and_predict([Path("M.pack")], three_files, property_map={"mid": [1] * 11}, path_to_output=tmp_path, model_loader=Double)
    with pytest.raises(ValueError, match="needs structures"):
        predict.load_dataset_and_predict([Path("M.pack")], os.path.join(ROOT, "tests", "golden", "frames_tiny.hdf5"), property="charge",
                                         path_to_output=tmp_path, model_loader=Double)
