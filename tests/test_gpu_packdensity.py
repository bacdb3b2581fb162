"""th_packing_density on the GPU: per-atom int32 and per-residue float64 outputs equal, AS BYTES, to the reference's own output
(tests/golden/packdensity_golden.npz) and to the NumPy restatement; batching, repeatability, radii, ABI errors; the Python API, the
reference-named functions of design_utils.analyse_utils and analyse_properties.py end to end.  No tolerance anywhere: counts are
integers and the half-average of small integers is exact in float64."""
import csv
import ctypes as C
import gzip
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packdensity_restatement as pr  # noqa: E402
from timed_hip import _lib, pdbio, structure  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
UBQ = os.path.join(G, "1ubq.pdb1.gz")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "packdensity_golden.npz"))


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(pr.GOLDEN_CASES))
def test_golden_cases_as_bytes(gpu, golden, name):
    chains = pr.golden_structure(name)
    assert pr.coords_sha256(chains) == str(golden[f"{name}_sha256"])
    for radius in pr.RADII:
        for atom_filter in pr.FILTERS:
            xyz, group, selected, n_groups = pr.flatten(chains, atom_filter)
            density, residue = structure.contact_numbers(xyz, [0, len(xyz)], radius, group, selected, n_groups, device=gpu)
            print(name, radius, atom_filter, "atoms", len(density), "differing", int((density != golden[f"{name}_density_r{radius}"]).sum()))
            assert same_bytes(density, golden[f"{name}_density_r{radius}"]), (name, radius)
            assert same_bytes(residue, golden[f"{name}_res_{atom_filter}_r{radius}"]), (name, radius, atom_filter)


def test_all_golden_cases_in_one_batch(gpu, golden):
    names = list(pr.GOLDEN_CASES)
    for atom_filter in pr.FILTERS:
        parts = [pr.flatten(pr.golden_structure(n), atom_filter) for n in names]
        offsets = np.cumsum([0] + [len(p[0]) for p in parts])
        res_lo = np.cumsum([0] + [p[3] for p in parts])
        xyz = np.concatenate([p[0] for p in parts])
        group = np.concatenate([np.where(p[1] >= 0, p[1] + res_lo[k], -1) for k, p in enumerate(parts)]).astype(np.int32)
        selected = np.concatenate([p[2] for p in parts])
        density, residue = structure.contact_numbers(xyz, offsets, 7.0, group, selected, int(res_lo[-1]), device=gpu)
        for k, n in enumerate(names):
            assert same_bytes(density[offsets[k]:offsets[k + 1]], golden[f"{n}_density_r7.0"]), n
            assert same_bytes(residue[res_lo[k]:res_lo[k + 1]], golden[f"{n}_res_{atom_filter}_r7.0"]), (n, atom_filter)


def test_1ubq_through_the_python_api(gpu, golden):
    model = pdbio.read_pdb(UBQ)[0]
    for radius in pr.RADII:
        for atom_filter in pr.FILTERS:
            (res,) = structure.packing_density([model], radius=radius, atom_filter=atom_filter, device=gpu)
            assert same_bytes(res.atom_density, golden[f"ubq_density_r{radius}"])
            assert same_bytes(res.residue_density, golden[f"ubq_res_{atom_filter}_r{radius}"])
            assert len(res.residues) == 76
    by_path, calpha = structure.packing_density([UBQ, model], atom_filter="calpha", device=gpu)
    assert same_bytes(by_path.residue_density, calpha.residue_density)
    lay = calpha.layout
    ca_atoms = np.flatnonzero(lay.selected)
    assert same_bytes(calpha.residue_density, golden["ubq_density_r7.0"][ca_atoms].astype(np.float64))     # one atom per residue


def _random_structure(rng, n):
    half = max(3.0, (n * 20.0) ** (1 / 3) / 2)
    return np.round(rng.uniform(-half, half, (n, 3)), 3)


def _random_groups(rng, sizes):
    """residues of 1..12 consecutive atoms, some atoms neighbours only, about half of the grouped atoms selected"""
    group, n_groups = [], 0
    for n in sizes:
        i = 0
        while i < n:
            m = int(min(rng.integers(1, 13), n - i))
            if rng.random() < 0.15:
                group += [-1] * m
            else:
                group += [n_groups] * m
                n_groups += 1
            i += m
    group = np.array(group, dtype=np.int32)
    selected = ((rng.random(len(group)) < 0.5) & (group >= 0)).astype(np.uint8)
    return group, selected, n_groups


@pytest.fixture(scope="module")
def mixed_batch():
    """sizes 0 .. 20 011 atoms across several tile boundaries and 2 700 + work items: more than the device holds at once (256 CUs
    x 8 workgroups of 256 threads)"""
    rng = np.random.default_rng(23)
    sizes = [0, 1, 2, 255, 256, 257, 0, 511, 512, 513, 1000, 20011, 3, 767, 769] + [520] * 900 + [0, 2049]
    coords = [_random_structure(rng, n) for n in sizes]
    xyz = np.concatenate(coords)
    offsets = np.cumsum([0] + sizes).astype(np.int64)
    group, selected, n_groups = _random_groups(rng, sizes)
    items = sum((n + pr.TILE - 1) // pr.TILE for n in sizes)
    assert items > 2048 * 1.3
    want_density = pr.restate_density(xyz, offsets, 7.0)
    want_residue = pr.restate_residues(want_density, group, selected, n_groups)
    return sizes, xyz, offsets, group, selected, n_groups, want_density, want_residue


def test_mixed_batch_equals_the_restatement(gpu, mixed_batch):
    sizes, xyz, offsets, group, selected, n_groups, want_density, want_residue = mixed_batch
    density, residue = structure.contact_numbers(xyz, offsets, 7.0, group, selected, n_groups, device=gpu)
    print("atoms", len(xyz), "differing", int((density != want_density).sum()), "residues", n_groups, "differing", int((residue != want_residue).sum()))
    assert same_bytes(density, want_density) and same_bytes(residue, want_residue)
    again, residue_again = structure.contact_numbers(xyz, offsets, 7.0, group, selected, n_groups, device=gpu)
    assert same_bytes(again, density) and same_bytes(residue_again, residue)                   # two calls, the same bytes
    none, residue_only = structure.contact_numbers(xyz, offsets, 7.0, group, selected, n_groups, device=gpu, atoms=False)
    assert none is None and same_bytes(residue_only, residue)                                  # per-atom counts are optional
    atoms_only, empty = structure.contact_numbers(xyz, offsets, 7.0, device=gpu)
    assert same_bytes(atoms_only, density) and empty.shape == (0,)


def test_a_structure_alone_gives_the_bytes_it_gives_in_the_batch(gpu, mixed_batch):
    sizes, xyz, offsets, group, selected, n_groups, want_density, want_residue = mixed_batch
    for s in (1, 3, 4, 5, 9, 11, 13, 20, len(sizes) - 1):
        lo, hi = offsets[s], offsets[s + 1]
        g = group[lo:hi]
        used = g[g >= 0]
        g_lo, g_n = (int(used.min()), int(used.max() - used.min() + 1)) if used.size else (0, 0)
        local = np.where(g >= 0, g - g_lo, -1).astype(np.int32)
        density, residue = structure.contact_numbers(xyz[lo:hi], [0, hi - lo], 7.0, local, selected[lo:hi], g_n, device=gpu)
        assert same_bytes(density, want_density[lo:hi]), sizes[s]
        assert same_bytes(residue, want_residue[g_lo:g_lo + g_n]), sizes[s]


@pytest.mark.parametrize("radius", [7.0, 4.5, 6.3, 1.1, 0.0, -2.0, 1e9, float("inf"), float("nan")])
def test_radii(gpu, radius):
    chains = pr.golden_structure("mix")
    xyz, group, selected, n_groups = pr.flatten(chains, "backbone")
    density, residue = structure.contact_numbers(xyz, [0, len(xyz)], radius, group, selected, n_groups, device=gpu)
    want = pr.restate_density(xyz, [0, len(xyz)], radius)
    assert same_bytes(density, want)
    assert same_bytes(residue, pr.restate_residues(want, group, selected, n_groups))
    finite = np.isfinite(xyz).all(axis=1)
    if not radius > 0:
        assert (density == -1).all() and (residue == -1.0).all()
    if radius >= 1e9:
        assert (density[finite] == finite.sum() - 1).all() and (density[~finite] == -1).all()


def _raw_call(lib, xyz, total, offsets, n_structures, radius, group, selected, n_groups, density, residue):
    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    return lib.th_packing_density(0, ptr(xyz), total, ptr(offsets), n_structures, radius, ptr(group), ptr(selected), n_groups,
                                  ptr(density), ptr(residue), None)


def test_abi_errors_return_einval_and_leave_the_outputs_untouched(gpu, lib):
    rng = np.random.default_rng(2)
    xyz = _random_structure(rng, 10)
    offsets = np.array([0, 4, 10], np.int64)
    group = np.array([0, 0, 1, 1, -1, 2, 2, 2, 3, 3], np.int32)
    selected = np.ones(10, np.uint8)
    bad_calls = {
        "offsets NULL": dict(offsets=None),
        "xyz NULL": dict(xyz=None),
        "negative total": dict(total=-1),
        "negative structures": dict(n_structures=-1),
        "negative groups": dict(n_groups=-1),
        "offsets decrease": dict(offsets=np.array([0, 11, 10], np.int64)),
        "offsets start": dict(offsets=np.array([1, 4, 10], np.int64)),
        "offsets end": dict(offsets=np.array([0, 4, 9], np.int64)),
        "group too large": dict(group=np.array([0, 0, 1, 1, -1, 2, 2, 2, 3, 4], np.int32)),
        "group below -1": dict(group=np.array([0, 0, 1, 1, -2, 2, 2, 2, 3, 3], np.int32)),
        "group not contiguous": dict(group=np.array([0, 0, 1, 1, -1, 2, 2, 0, 3, 3], np.int32)),
        "group split by a neighbour": dict(group=np.array([0, 0, 1, 1, 2, -1, 2, 2, 3, 3], np.int32)),
        "group NULL": dict(group=None),
        "selected NULL": dict(selected=None),
        "residue_out NULL": dict(residue=None),
    }
    for what, change in bad_calls.items():
        density = np.full(10, 12345, np.int32)
        residue = np.full(4, 6.5)
        kw = dict(xyz=xyz, total=10, offsets=offsets, n_structures=2, radius=7.0, group=group, selected=selected, n_groups=4,
                  density=density, residue=residue)
        kw.update(change)
        assert _raw_call(lib, **kw) == _lib.TH_EINVAL, what
        assert b"th_packing_density" in lib.th_last_error(), what
        assert (density == 12345).all() and (residue == 6.5).all(), what
    density = np.full(10, 12345, np.int32)
    residue = np.full(4, 6.5)
    assert _raw_call(lib, xyz, 10, offsets, 2, 7.0, group, selected, 4, density, residue) == _lib.TH_OK
    want = pr.restate_density(xyz, offsets, 7.0)
    assert same_bytes(density, want) and same_bytes(residue, pr.restate_residues(want, group, selected, 4))
    with pytest.raises(_lib.TimedHipError) as err:
        structure.contact_numbers(xyz, [0, 5, 4, 10], device=gpu)
    assert err.value.code == _lib.TH_EINVAL


def test_nothing_to_launch(gpu, lib):
    residue = np.full(3, 6.5)
    zero = np.zeros(1, np.int64)
    assert _raw_call(lib, None, 0, zero, 0, 7.0, None, None, 3, None, residue) == _lib.TH_OK and (residue == -1.0).all()
    density, residue = structure.contact_numbers(np.zeros((0, 3)), [0, 0, 0, 0], device=gpu)
    assert density.shape == (0,) and residue.shape == (0,)
    assert structure.packing_density([], device=gpu) == []
    (res,) = structure.packing_density([pdbio.Model(1, [])], device=gpu)
    assert res.atom_density.shape == (0,) and res.residue_density.shape == (0,) and res.residues == []


def test_reference_named_functions_on_1ubq(gpu, golden):
    from design_utils import analyse_utils as au
    for atom_filter in pr.FILTERS:
        got = au.extract_packdensity_from_ampal(UBQ, atom_filter=atom_filter, device=gpu)
        assert got == [golden[f"ubq_res_{atom_filter}_r7.0"].tolist()]
    model = pdbio.read_pdb(UBQ)[0]
    assert au.extract_packdensity_from_ampal(model, load_pdb=False) == [golden["ubq_res_ca_r7.0"].tolist()]          # default "ca"
    with pytest.raises(ValueError, match="Atom Filter"):
        au.extract_packdensity_from_ampal(UBQ, atom_filter="sidechain")
    b = au.extract_bfactor_from_ampal(UBQ)
    assert len(b) == 1 and len(b[0]) == 76


def _read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_analyse_properties_end_to_end(gpu, golden, tmp_path, capsys):
    import analyse_properties as ap
    d = tmp_path / "structures"
    (d / "af2").mkdir(parents=True)
    cases = {"n255.pdb": "n255", "af2/n256.ent": "n256", "af2/1abcA.pdb.gz": "n257", "n2.pdb1": "n2"}
    for rel, name in cases.items():
        if rel.endswith(".gz"):
            pr.write_pdb(pr.golden_structure(name), tmp_path / "plain.pdb")
            with open(tmp_path / "plain.pdb", "rb") as src, gzip.open(d / rel, "wb") as dst:
                shutil.copyfileobj(src, dst)
        else:
            pr.write_pdb(pr.golden_structure(name), d / rel)
    (d / "README.txt").write_text("not a structure\n")
    # a prediction matrix whose dataset map names one of the structures by its file stem
    rng = np.random.default_rng(4)
    probs = rng.dirichlet(np.ones(20), 12)
    np.savetxt(tmp_path / "M.csv", probs, delimiter=",")
    (tmp_path / "map.txt").write_text("ignore_uncommon False\ninclude_pdbs\n##########\n1abcA 7\n2defB 5\n")
    expected = {"1ubq.pdb1.gz": "ubq", "af2/1abcA.pdb.gz": "n257", "af2/n256.ent": "n256", "n2.pdb1": "n2", "n255.pdb": "n255"}
    for atom_filter, batch_mb, submissions in (("all", 256.0, 1), ("ca", 0.02, 3)):
        out = tmp_path / f"out_{atom_filter}"
        args = ap.build_parser().parse_args(["--path_to_pdb", str(d), UBQ, "--path_to_output", str(out), "--atom_filter_function", atom_filter,
                                             "--workers", "3", "--batch_mb", str(batch_mb), "--device", str(gpu),
                                             "--path_to_pred_matrix", str(tmp_path / "M.csv"), "--path_to_datasetmap", str(tmp_path / "map.txt")])
        ap.main(args)
        assert f"in {submissions} GPU submission(s)" in capsys.readouterr().out
        head, rows = _read_csv(out / "residue_properties.csv")
        assert head == ["structure", "chain", "residue_number", "residue_name", "packing_density", "bfactor"]
        head_s, rows_s = _read_csv(out / "structure_properties.csv")
        assert head_s == ["structure", "atoms", "residues", "packing_density_mean", "packing_density_std", "bfactor_mean", "bfactor_std",
                          "entropy_mean", "entropy_std"]
        assert [r[0] for r in rows_s] == ["af2/1abcA.pdb.gz", "af2/n256.ent", "n2.pdb1", "n255.pdb", "1ubq.pdb1.gz"]
        for label, atoms, residues, d_mean, d_std, b_mean, b_std, e_mean, e_std in rows_s:
            name = expected[label]
            want = golden[f"{name}_res_{atom_filter}_r7.0"]
            mine = [r for r in rows if r[0] == label]
            assert int(atoms) == len(golden[f"{name}_density_r7.0"]) and int(residues) == len(want) == len(mine)
            assert np.array([float(r[4]) for r in mine]).tobytes() == want.tobytes(), (label, atom_filter)
            assert float(d_mean) == np.mean(want) and float(d_std) == np.std(want)
            if name == "ubq":
                bfac = np.array(structure.residue_bfactors(pdbio.read_pdb(UBQ)[0])[0])
                assert [r[1] for r in mine] == ["A"] * 76 and mine[0][2:4] == ["1", "MET"]
            else:
                first_chain = pr.golden_structure(name)[0]
                bfac = np.array([pr.bfactor_of(r) for r in first_chain])
                assert [r[2] for r in mine] == [str(r["number"]) for r in first_chain]
            assert [float(r[5]) for r in mine] == bfac.tolist()
            assert float(b_mean) == np.mean(bfac) and float(b_std) == np.std(bfac)
            if label == "af2/1abcA.pdb.gz":
                from design_utils.analyse_utils import calculate_prediction_entropy
                e = calculate_prediction_entropy(probs[:7])
                assert float(e_mean) == np.mean(e) and float(e_std) == np.std(e)
            else:
                assert e_mean == "nan" and e_std == "nan"
