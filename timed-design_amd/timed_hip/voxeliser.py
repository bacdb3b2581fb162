"""GPU voxeliser: PDB structure -> per-residue 21x21x21xC frames.

Replaces the producer of the reference's input: ``aposteriori.make_frame_dataset`` as the reference invokes it
(ui.py:73-86: frame_edge_length=21.0, voxels_per_side=21, codec=Codec.CNOCACB(), voxels_as_gaussian=True,
voxelise_all_states=False; README.md:83-97: ``make-frame-dataset ... -cb True -ae CNOCBCA -g True``), and writes what
predict.py consumes (a frame pack, timed_hip/framepack.py, or device-resident frames for th_predict_device) — so a
structure goes PDB -> frames -> probabilities without the HDF5 round trip.

    *** PARITY UNPINNED ***  aposteriori==2.4.0 is an external package whose source is neither in /root/reference nor
    in this image, and the reference has no test at this boundary.  What IS fixed by the reference tree: the dataset
    layout and attributes (design_utils/utils.py:238-251), the frame geometry the UI asks for (ui.py:73-86), the atom
    encoder names, and the idealised C-beta position (-0.741287356, -0.53937931, -1.224287356) quoted at utils.py:247.
    Everything else below is this module's own specification, written from aposteriori's documented behaviour; a model
    trained on aposteriori's frames must be validated on frames from here before the two are mixed.  The oracle
    (oracle/voxel_oracle.py) restates exactly this specification and the GPU kernel is tested against it.

Specification
  1. Atoms: ATOM records (HETATM only for residues of UNCOMMON_RESIDUE_DICT, mapped to their parent amino acid); first
     alternate location; model 1 unless ``all_states``.
  2. Encoded atoms ("keep backbone, add C-beta"): N, CA, C, O of every residue of every chain, plus — with
     ``encode_cb`` — ONE idealised C-beta per residue that has N, CA and C, at CB_LOCAL in that residue's own frame
     (real C-beta and all side-chain atoms are dropped).  Channels follow ``atom_encoder`` (default C, N, O, CA, CB).
  3. Residue frame (aposteriori's align_to_residue_plane): origin at CA; +y along CA->N; C in the xy half-plane x > 0;
     z = x cross y.  local = R (p - CA) with R = rows (e_x, e_y, e_z), evaluated in float32 as
     (R_i0*dx + R_i1*dy) + R_i2*dz with separate multiplies and adds.
  4. Grid: voxel edge a = frame_edge_length / voxels_per_side; index_k = floor(local_k / a + 0.5) + voxels_per_side//2;
     an atom is encoded iff all three indices are inside [0, voxels_per_side).  The decision is taken on the floored
     float32 value, before any conversion to an integer: an atom whose local coordinate is not finite in some component
     (NaN or infinite coordinates, or a frames_rt row that holds such a value), or whose floor(local_k / a + 0.5) lies
     outside [-(voxels_per_side//2), voxels_per_side - 1 - voxels_per_side//2] for some k, is not encoded.  A frame
     whose frames_rt row holds a non-finite value is therefore all zeros.
  5. Boolean frames (voxels_as_gaussian=False): frame[index][channel] = 1 (uint8).
  6. Gaussian frames: the atom is spread over the 3x3x3 block of voxels around its own voxel with weights
     w = exp(-r^2 / (2 sigma^2)), r = distance from the voxel centre to the atom, sigma = sigma_scale * vdW radius
     (C 1.70, N 1.55, O 1.52 Angstrom; sigma_scale 0.5), normalised so that the 27 weights sum to 1 (weight falling
     outside the frame is lost); contributions are added in atom order, float32, no clipping.
  7. One frame per residue that has N, CA, C and a standard (or mapped) name; label = one-hot over
     ``standard_amino_acids`` order; dataset-map rows (pdb_code, chain, residue number, label) in file order with
     residues sorted numerically per chain, as create_flat_dataset_map would list them.
  8. Property channel (``property`` "polarity" or "charge": the sixth channel of the reference's TIMED_polar / TIMED_charge,
     codecs CNOCBCAP / CNOCBCAQ, reference README.md:91, ui.py:734-746).
         *** PARITY UNPINNED AGAINST AMPAL AND APOSTERIORI ***  The tables (design_utils/amino_acids.py) stand in for
         ampal's, which is not available here; where aposteriori puts the property value, and with which width, is this
         module's own reading like the rest of it.  The reference only pins A -> 0, K -> +1, D -> -1 (utils.py:86).
     The atom encoder gains a last name, "P" or "Q" (channel 5 with the default encoder: C, N, O, CA, CB, Q).  Every residue
     that has a CA and whose value v is not 0 contributes ONE extra atom at the CA's coordinates, in the property channel, with
     carbon's sigma (0.5 x 1.70) and weight v, appended after the residue's own atoms; a value of 0 emits nothing.  A Gaussian
     contribution of an atom of weight v is v * (w / total), the product rounded to float32 before it is added (item 6 is
     v = 1).  Property channels need Gaussian frames.  v is the value of the residue's own name (charge: D, E, C, Y -1; K, R, H
     +1; polarity: R, D, E, H, K 1; everything else 0) unless a PROPERTY MAP says otherwise: one integer per frame of the
     structure in dataset-map order (item 7), from {0, 1} for polarity and {-1, 0, 1} for charge.  Residues that get no frame
     always carry their own value.  The map replaces the reference's renaming of residues to ALA / LYS / ASP
     (modify_pdb_with_input_property, utils.py:60-110): labels keep the native residues, backbone-only frames do not depend on
     the name.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, pdbio

CB_LOCAL = np.array([-0.741287356, -0.53937931, -1.224287356])     # reference design_utils/utils.py:247
DEFAULT_ENCODER = ("C", "N", "O", "CA", "CB")
VDW_RADIUS = {"C": 1.70, "N": 1.55, "O": 1.52}
SIGMA_SCALE = 0.5
BACKBONE = ("N", "CA", "C", "O")


def residue_frame(n: np.ndarray, ca: np.ndarray, c: np.ndarray) -> Optional[np.ndarray]:
    """3x3 rotation (rows e_x, e_y, e_z) of spec item 3, float64; None for degenerate geometry."""
    ey = n - ca
    ny = np.linalg.norm(ey)
    if ny < 1e-6:
        return None
    ey = ey / ny
    cp = c - ca
    cp = cp - np.dot(cp, ey) * ey
    nx = np.linalg.norm(cp)
    if nx < 1e-6:
        return None
    ex = cp / nx
    ez = np.cross(ex, ey)
    return np.stack([ex, ey, ez])


PROPERTY_ATOM = {"polarity": "P", "charge": "Q"}       # the codec letters of the reference's CNOCBCAP / CNOCBCAQ


def property_encoder(property: Optional[str], atom_encoder: Sequence[str] = DEFAULT_ENCODER) -> Tuple[str, ...]:
    """the atom encoder with the property's name last (spec item 8); unchanged without a property"""
    if property is None:
        return tuple(atom_encoder)
    if property not in PROPERTY_ATOM:
        raise AssertionError(f"Property {property} not found among {list(PROPERTY_ATOM)}")
    return tuple(atom_encoder) + (PROPERTY_ATOM[property],)


def check_property_map(property: str, values, n_frames: int, name: str) -> np.ndarray:
    """a property map of one structure as int64 [n_frames]; ValueError naming the structure and the two numbers otherwise"""
    from design_utils.amino_acids import PROPERTY_VALUES
    allowed = PROPERTY_VALUES[property]
    arr = np.asarray(values)
    if arr.ndim != 1 or arr.shape[0] != n_frames:
        raise ValueError(f"{name}: the {property} map has {arr.size if arr.ndim == 1 else arr.shape} values, the structure has {n_frames} frames")
    if arr.size and (arr.dtype.kind not in "iub" or not np.isin(arr, allowed).all()):
        bad = next(i for i, v in enumerate(arr.tolist()) if v not in allowed or isinstance(v, float))
        raise ValueError(f"{name}: the {property} map holds {arr[bad]} at frame {bad}; allowed values are {list(allowed)}")
    return arr.astype(np.int64)


def read_property_map(path):
    """A property map file: a JSON object {pdb_code: [ints]} (structures that are not named keep their native values) or, for a
    single structure, a bare JSON list.  Returned as it is; prepare_structure_with_property validates the values."""
    import json
    with open(path) as f:
        got = json.load(f)
    if not isinstance(got, (dict, list)):
        raise ValueError(f"{path}: a property map is a JSON object {{pdb_code: [ints]}} or a JSON list")
    return got


def map_of(property_map, code: str):
    """the map of structure ``code`` out of what read_property_map returns (None: native values)"""
    if isinstance(property_map, dict):
        return property_map.get(code)
    return property_map


def prepare_structure(model: pdbio.Model, encode_cb: bool = True, atom_encoder: Sequence[str] = DEFAULT_ENCODER,
                      uncommon: Optional[dict] = None):
    """Host-side preparation of one model: (atoms_xyz f32 [n,3], atom_channel i32 [n], atom_sigma f32 [n],
    frames_rt f32 [n_res,12], rows [(chain, number, three-letter label)])."""
    xyz, ch, sg, _wt, frt, rows = _prepare(model, encode_cb, atom_encoder, uncommon, None, None, "")
    return xyz, ch, sg, frt, rows


def prepare_structure_with_property(model: pdbio.Model, property: Optional[str] = None, property_map=None, encode_cb: bool = True,
                                    atom_encoder: Sequence[str] = DEFAULT_ENCODER, uncommon: Optional[dict] = None, name: str = "structure"):
    """prepare_structure with the property atoms of spec item 8: (atoms_xyz, atom_channel, atom_sigma, atom_weight f32 [n],
    frames_rt, rows).  ``atom_encoder`` is the encoder WITHOUT the property name (it is appended here); ``property_map``: one
    integer per frame in the order of ``rows``, or None for every residue's own value.  Without a property the weights are all 1."""
    return _prepare(model, encode_cb, atom_encoder, uncommon, property, property_map, name)


def _prepare(model, encode_cb, atom_encoder, uncommon, property, property_map, name):
    """the one loop behind prepare_structure and prepare_structure_with_property"""
    from design_utils.amino_acids import PROPERTY_TABLE, UNCOMMON_RESIDUE_DICT, standard_amino_acids
    uncommon = UNCOMMON_RESIDUE_DICT if uncommon is None else uncommon
    standard = set(standard_amino_acids.values())
    one_letter = {three: one for one, three in standard_amino_acids.items()}
    atom_encoder = property_encoder(property, atom_encoder)
    table = PROPERTY_TABLE[property] if property is not None else None
    chan = {name_: i for i, name_ in enumerate(atom_encoder)}
    xyz: List[np.ndarray] = []
    ch: List[int] = []
    sg: List[float] = []
    wt: List[float] = []
    slot: dict = {}                       # id(residue) -> index of its property atom
    frames: List[np.ndarray] = []
    rows: List[Tuple[str, str, str]] = []
    per_chain: dict = {}
    framed: list = []                     # the residues that get a frame, in the order of ``rows``
    for res in model.residues:
        label = res.name if res.name in standard else uncommon.get(res.name)
        if label is None or (res.hetero and res.name not in uncommon):
            continue
        R = None
        if all(a in res.atoms for a in ("N", "CA", "C")):
            R = residue_frame(res.atoms["N"], res.atoms["CA"], res.atoms["C"])
        for a in BACKBONE:
            if a in res.atoms and a in chan:
                xyz.append(res.atoms[a]); ch.append(chan[a]); sg.append(SIGMA_SCALE * VDW_RADIUS[a[0]]); wt.append(1.0)
        if R is not None and encode_cb and "CB" in chan:
            xyz.append(res.atoms["CA"] + R.T @ CB_LOCAL); ch.append(chan["CB"]); sg.append(SIGMA_SCALE * VDW_RADIUS["C"]); wt.append(1.0)
        if table is not None and "CA" in res.atoms:
            # the residue's own value; a property map overwrites it below, once the frames have their order.  Zeros are dropped there
            slot[id(res)] = len(xyz)
            xyz.append(res.atoms["CA"]); ch.append(len(atom_encoder) - 1); sg.append(SIGMA_SCALE * VDW_RADIUS["C"])
            wt.append(float(table[one_letter[label]]))
        if R is not None:
            per_chain.setdefault(res.chain, []).append((res, R, label))
    for chain, items in per_chain.items():
        def key(it):
            digits = "".join(c for c in it[0].number if c.isdigit() or c == "-")
            return (int(digits) if digits not in ("", "-") else 0, it[0].number)
        for res, R, label in sorted(items, key=key):
            frames.append(np.concatenate([R.reshape(9), res.atoms["CA"]]))
            rows.append((chain, res.number, label))
            framed.append(res)
    xyz_a = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    ch_a, sg_a, wt_a = np.asarray(ch, dtype=np.int32), np.asarray(sg, dtype=np.float32), np.asarray(wt, dtype=np.float32)
    if table is not None:
        if property_map is not None:
            for res, v in zip(framed, check_property_map(property, property_map, len(framed), name).tolist()):
                wt_a[slot[id(res)]] = v
        keep = wt_a != 0                  # a value of 0 emits nothing
        xyz_a, ch_a, sg_a, wt_a = xyz_a[keep], ch_a[keep], sg_a[keep], wt_a[keep]
    return xyz_a, ch_a, sg_a, wt_a, np.asarray(frames, dtype=np.float32).reshape(-1, 12), rows


def voxelise(atoms_xyz, atom_channel, atom_sigma, frames_rt, voxels_per_side: int = 21, frame_edge_length: float = 21.0,
             n_channels: int = 5, gaussian: bool = True, device: int = 0, d_out: Optional[int] = None) -> Optional[np.ndarray]:
    """The frames of one structure (th_voxelise: the one-structure, unit-weight case of th_voxelise_batch).  Returns frames
    [n_res, V, V, V, C] (float32 for Gaussian, uint8 for boolean frames), or None when ``d_out`` (a device address with room for them) is given: the frames then stay in HBM for
    th_predict_device."""
    lib = _lib.load()
    xyz = np.ascontiguousarray(atoms_xyz, dtype=np.float32)
    chn = np.ascontiguousarray(atom_channel, dtype=np.int32)
    sig = np.ascontiguousarray(atom_sigma, dtype=np.float32)
    frt = np.ascontiguousarray(frames_rt, dtype=np.float32)
    n_res, V = frt.shape[0], int(voxels_per_side)
    out = None
    if d_out is None:
        out = np.empty((n_res, V, V, V, n_channels), dtype=np.float32 if gaussian else np.uint8)
    if n_res:
        _lib.check(lib.th_voxelise(device, xyz.ctypes.data, chn.ctypes.data, sig.ctypes.data, xyz.shape[0], frt.ctypes.data, n_res,
                                   V, float(frame_edge_length), n_channels, 1 if gaussian else 0,
                                   C.c_void_p(d_out) if d_out is not None else out.ctypes.data, 1 if d_out is not None else 0))
    return out


def voxelise_batch(atoms_xyz, atom_channel, atom_sigma, atom_weight, atom_offsets, frames_rt, frame_structure, voxels_per_side: int = 21,
                   frame_edge_length: float = 21.0, n_channels: int = 5, gaussian: bool = True, device: int = 0,
                   d_out: Optional[int] = None, timing: Optional[dict] = None) -> Optional[np.ndarray]:
    """The frames of many structures in one launch (th_voxelise_batch): structure s owns the atoms
    [atom_offsets[s], atom_offsets[s + 1]) of the flat arrays, frame r is built from the atoms of structure frame_structure[r]
    alone and the row frames_rt[r].  ``atom_weight``: float32 per atom, or None (every atom counts 1; the frames then equal
    ``voxelise``'s byte for byte).  Returns frames [n_frames, V, V, V, C], or None when ``d_out`` (a device address with room
    for them) is given.  ``timing``: a dict whose ``kernel_ms`` the call adds to."""
    lib = _lib.load()
    xyz = np.ascontiguousarray(atoms_xyz, dtype=np.float32)
    chn = np.ascontiguousarray(atom_channel, dtype=np.int32)
    sig = np.ascontiguousarray(atom_sigma, dtype=np.float32)
    wgt = None if atom_weight is None else np.ascontiguousarray(atom_weight, dtype=np.float32)
    off = np.ascontiguousarray(atom_offsets, dtype=np.int64)
    frt = np.ascontiguousarray(frames_rt, dtype=np.float32)
    fst = np.ascontiguousarray(frame_structure, dtype=np.int32)
    n_frames, V = frt.shape[0], int(voxels_per_side)
    if fst.shape[0] != n_frames or off.ndim != 1 or off.shape[0] < 1 or chn.shape[0] != xyz.shape[0] or sig.shape[0] != xyz.shape[0] or \
            (wgt is not None and wgt.shape[0] != xyz.shape[0]):
        raise ValueError("voxelise_batch: array lengths disagree")
    out = None
    if d_out is None:
        out = np.empty((n_frames, V, V, V, n_channels), dtype=np.float32 if gaussian else np.uint8)
    ms = C.c_double(0.0)
    _lib.check(lib.th_voxelise_batch(device, _lib.ptr(xyz), _lib.ptr(chn), _lib.ptr(sig), _lib.ptr(wgt), xyz.shape[0], _lib.ptr(off),
                                     off.shape[0] - 1, _lib.ptr(frt), _lib.ptr(fst), n_frames, V, float(frame_edge_length), n_channels,
                                     1 if gaussian else 0, C.c_void_p(d_out) if d_out is not None else _lib.ptr(out),
                                     1 if d_out is not None else 0, C.byref(ms) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + ms.value
    return out


def voxelise_pdb(path, voxels_per_side: int = 21, frame_edge_length: float = 21.0, encode_cb: bool = True,
                 atom_encoder: Sequence[str] = DEFAULT_ENCODER, gaussian: bool = True, all_states: bool = False, device: int = 0,
                 property: Optional[str] = None, property_map=None):
    """PDB file -> (frames, labels [n,20] uint8, flat dataset map rows (pdb_code, chain, residue number, label)).
    The pdb code is the file name up to ".pdb"; with ``all_states`` every model is voxelised as "<code>_<k>"
    (aposteriori's voxelise_all_states), otherwise model 1 only.  ``property`` ("polarity" / "charge", spec item 8) adds the
    property channel behind ``atom_encoder``'s; ``property_map``: one integer per frame (or {pdb_code: [ints]}), None for the
    residues' own values."""
    from design_utils.amino_acids import standard_amino_acids
    three = list(standard_amino_acids.values())
    code = os.path.basename(str(path)).split(".pdb")[0]
    if property is not None and not gaussian:
        raise ValueError(f"a {property} channel needs Gaussian frames (boolean frames carry no weight)")
    n_channels = len(property_encoder(property, atom_encoder))
    models = pdbio.read_pdb(path)
    if not models:
        raise ValueError(f"{path}: no ATOM records")
    if not all_states:
        models = models[:1]
    frames, labels, flat = [], [], []
    for k, model in enumerate(models):
        name = f"{code}_{k}" if all_states else code
        xyz, ch, sg, wt, frt, rows = prepare_structure_with_property(model, property, map_of(property_map, name), encode_cb=encode_cb,
                                                                     atom_encoder=atom_encoder, name=name)
        frames.append(voxelise_batch(xyz, ch, sg, wt if property is not None else None, [0, len(xyz)], frt, np.zeros(len(frt), np.int32),
                                     voxels_per_side, frame_edge_length, n_channels, gaussian, device))
        for chain, number, label in rows:
            flat.append((name, chain, number, label))
            onehot = np.zeros(20, np.uint8)
            onehot[three.index(label)] = 1
            labels.append(onehot)
    X = np.concatenate(frames) if frames else np.empty((0,) + (voxels_per_side,) * 3 + (n_channels,), np.float32)
    return X, np.asarray(labels, dtype=np.uint8).reshape(-1, 20), flat


PROVENANCE = "timed_hip.voxeliser (in-house GPU voxeliser; parity with aposteriori 2.4.0 NOT pinned by a golden file)"


def write_frame_pack(stem, frames: np.ndarray, labels: np.ndarray, flat_map, gaussian: bool, source: str = ""):
    """Store voxelised frames as a frame pack that predict.py accepts wherever it accepts an .hdf5 path."""
    import json
    stem = os.fspath(stem)
    np.save(stem + ".frames.npy", frames)
    np.save(stem + ".labels.npy", labels)
    np.savetxt(stem + ".map.txt", np.asarray(flat_map), delimiter=",", fmt="%s")
    with open(stem + ".meta.json", "w") as f:
        json.dump(dict(frame_dims=list(frames.shape[1:]), voxels_as_gaussian=bool(gaussian), n_frames=int(frames.shape[0]),
                       source=source, make_frame_dataset_ver="timed_hip.voxeliser (unpinned vs aposteriori 2.4.0)",
                       frame_provenance=PROVENANCE), f)


def write_hdf5(path, frames: np.ndarray, labels: np.ndarray, flat_map, gaussian: bool, atom_encoder: Sequence[str] = DEFAULT_ENCODER,
               frame_edge_length: float = 21.0, encode_cb: bool = True, compression: Optional[str] = "gzip"):
    """Store voxelised frames in aposteriori's own layout (reference design_utils/utils.py:238-251) — pdb_code / chain /
    residue number datasets with `label` and `encoded_residue` attributes, file attributes as make-frame-dataset writes
    them — with timed_hip.h5write, so that h5py, the reference's predict.py and this repo's readers all open it.  Frames
    are stored as float64 (Gaussian) or bool like the reference's loader expects (utils.py:518-521)."""
    from design_utils.amino_acids import standard_amino_acids
    from . import h5write
    with h5write.File(path) as f:
        f.attrs["make_frame_dataset_ver"] = "2.4.0"        # the layout version the reference's checks accept (utils.py:271-280)
        # ... but these frames did NOT come from aposteriori: a separate attribute lets any downstream tool tell them apart
        f.attrs["frame_provenance"] = PROVENANCE
        f.attrs["frame_dims"] = np.asarray(frames.shape[1:], dtype=np.int64)
        f.attrs["atom_encoder"] = list(atom_encoder)
        f.attrs["encode_cb"] = bool(encode_cb)
        f.attrs["atom_filter_fn"] = "timed_hip.voxeliser: backbone + idealised C-beta (unpinned vs aposteriori)"
        f.attrs["residue_encoder"] = list(standard_amino_acids.keys())
        f.attrs["frame_edge_length"] = float(frame_edge_length)
        f.attrs["voxels_as_gaussian"] = bool(gaussian)
        groups: dict = {}
        for i, (pdb, chain, number, label) in enumerate(flat_map):
            g = groups.get((pdb,))
            if g is None:
                g = groups[(pdb,)] = f.create_group(str(pdb))
            c = groups.get((pdb, chain))
            if c is None:
                c = groups[(pdb, chain)] = g.create_group(str(chain))
            data = frames[i].astype(np.float64) if gaussian else frames[i].astype(bool)
            c.create_dataset(str(number), data, compression=compression,
                             attrs={"label": str(label), "encoded_residue": labels[i].astype(np.float64)})
