"""A folder of structures as a dataset (no reference counterpart: the reference needs an aposteriori .hdf5 of the frames first).

A *structure set* is a directory searched with ``pdbio.find_structures`` — or a single structure file when a property channel is
asked for.  Every file is parsed once on host threads (``batching.parse_each``) and prepared (``voxeliser`` spec items 1-4, 7, 8);
what stays in memory is the flat arrays of every structure, about 130 bytes per residue, never a frame.  The flat dataset map is
the structures in sorted order, each as ``voxeliser.voxelise_pdb`` lists it; the pdb code of a file is ``pdbio.stem_of`` its name.
Model 1 only.

Frames are built per request: ``device_batch`` gathers the atoms of the structures the requested rows touch, makes ONE
``th_voxelise_batch(out_on_device=1)`` call and hands out ``engine.DeviceFrames`` — the frames are born in HBM and never cross
PCIe; ``load_batch`` is the same call with the frames downloaded (``design_utils.utils.load_batch``'s contract).

PARITY UNPINNED AGAINST AMPAL AND APOSTERIORI: see timed_hip/voxeliser.py (the frames) and design_utils/amino_acids.py (the
charge and polarity tables)."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

from . import batching, pdbio, voxeliser


def is_structure_set(path, property: Optional[str] = None) -> bool:
    """a directory; with a property also a single structure file"""
    from . import framepack
    p = os.fspath(path)
    return os.path.isdir(p) or (property is not None and framepack.is_structure(p))


def _prepare_file(item):
    label, path, code, property, property_map = item
    models = pdbio.read_pdb(path)
    if not models:
        raise ValueError(f"{path}: no ATOM records")
    return voxeliser.prepare_structure_with_property(models[0], property, voxeliser.map_of(property_map, code), name=code)


class StructureSet:
    def __init__(self, path, property: Optional[str] = None, property_map=None, gaussian: bool = True, voxels_per_side: int = 21,
                 frame_edge_length: float = 21.0, workers: Optional[int] = None):
        from design_utils.amino_acids import standard_amino_acids
        if property is not None and not gaussian:
            raise ValueError(f"a {property} channel needs Gaussian frames (boolean frames carry no weight)")
        import warnings
        warnings.warn(f"{os.fspath(path)}: frames are built by {voxeliser.PROVENANCE}; expect small differences from a "
                      "make-frame-dataset .hdf5 of the same structures", stacklevel=2)
        self.path, self.property, self.gaussian = os.fspath(path), property, bool(gaussian)
        self.voxels_per_side, self.frame_edge_length = int(voxels_per_side), float(frame_edge_length)
        self.atom_encoder = voxeliser.property_encoder(property)
        self.n_channels = len(self.atom_encoder)
        found = pdbio.find_structures([path])
        by_code: dict = {}
        for label, p in found:
            code = pdbio.stem_of(label)
            if code in by_code:
                raise ValueError(f"{self.path}: {by_code[code]} and {p} are both structure {code}")
            by_code[code] = p
        if isinstance(property_map, list) and len(found) != 1:
            raise ValueError(f"{self.path}: a bare list is the property map of a single structure, this set holds {len(found)}; "
                             "name the structures: {pdb_code: [ints]}")
        order = sorted(by_code)
        if workers is None:
            from . import _lib
            workers = int(_lib.load().th_host_cpus())
        prepared = batching.parse_each(_prepare_file, [(c, by_code[c], c, property, property_map) for c in order], workers)
        three = list(standard_amino_acids.values())
        self.codes = order
        n_atoms = [len(p[0]) for p in prepared]
        n_rows = [len(p[4]) for p in prepared]
        self.atom_offsets = np.concatenate([[0], np.cumsum(n_atoms)]).astype(np.int64)
        self.row_offsets = np.concatenate([[0], np.cumsum(n_rows)]).astype(np.int64)

        def cat(k, dtype, tail=()):
            parts = [p[k] for p in prepared]
            return np.concatenate(parts) if parts else np.empty((0, *tail), dtype)
        self.xyz, self.chn, self.sig = cat(0, np.float32, (3,)), cat(1, np.int32), cat(2, np.float32)
        self.wgt = cat(3, np.float32) if property is not None else None
        self.frt = cat(4, np.float32, (12,))
        self.structure_of_row = np.repeat(np.arange(len(order), dtype=np.int64), n_rows)
        flat = [(code, chain, number, label) for code, p in zip(order, prepared) for chain, number, label in p[5]]
        self.flat_map = np.asarray(flat, dtype=str).reshape(-1, 4)
        self.labels = np.zeros((len(flat), 20), np.uint8)
        if flat:
            self.labels[np.arange(len(flat)), [three.index(r[3]) for r in flat]] = 1
        self._index = None
        self._cursor = 0

    def __len__(self):
        return self.flat_map.shape[0]

    @property
    def frame_dims(self):
        return (self.voxels_per_side,) * 3 + (self.n_channels,)

    def rows_of(self, data_point_batch) -> np.ndarray:
        """indices into the set's map of the rows of ``data_point_batch``; a contiguous slice of the map (what predict.py's loader
        asks for) is found from its first row and confirmed with one comparison"""
        n = len(data_point_batch)
        if n == 0:
            return np.empty(0, np.int64)
        rows = np.asarray(data_point_batch)
        if rows.ndim == 2 and rows.shape[1] >= 3:
            first = tuple(str(x) for x in rows[0, :3])
            for guess in (self._cursor, 0):
                if guess + n <= len(self) and tuple(self.flat_map[guess, :3]) == first and \
                        np.array_equal(self.flat_map[guess:guess + n, :3], rows[:, :3].astype(str)):
                    self._cursor = guess + n
                    return np.arange(guess, guess + n, dtype=np.int64)
        if self._index is None:
            self._index = {(p, c, r): i for i, (p, c, r, _l) in enumerate(self.flat_map.tolist())}
        return np.array([self._index[(str(p), str(c), str(r))] for p, c, r, *_ in data_point_batch], dtype=np.int64)

    def batch_arrays(self, idx: np.ndarray) -> dict:
        """the arguments of one th_voxelise_batch call for the map rows ``idx``: the atoms of the structures they touch, nothing else"""
        touched = np.unique(self.structure_of_row[idx])
        spans = [(int(self.atom_offsets[s]), int(self.atom_offsets[s + 1])) for s in touched]

        def take(a):
            return np.concatenate([a[lo:hi] for lo, hi in spans]) if spans else a[:0]
        return dict(atoms_xyz=take(self.xyz), atom_channel=take(self.chn), atom_sigma=take(self.sig),
                    atom_weight=None if self.wgt is None else take(self.wgt),
                    atom_offsets=np.concatenate([[0], np.cumsum([hi - lo for lo, hi in spans])]).astype(np.int64),
                    frames_rt=self.frt[idx], frame_structure=np.searchsorted(touched, self.structure_of_row[idx]).astype(np.int32))

    def _voxelise(self, idx, device, d_out=None):
        return voxeliser.voxelise_batch(**self.batch_arrays(idx), voxels_per_side=self.voxels_per_side,
                                        frame_edge_length=self.frame_edge_length, n_channels=self.n_channels, gaussian=self.gaussian,
                                        device=device, d_out=d_out)

    def load_batch(self, data_point_batch, device: int = 0):
        """design_utils.utils.load_batch's contract: (frames on the host, y [n, 20] float)"""
        idx = self.rows_of(data_point_batch)
        return self._voxelise(idx, device), self.labels[idx].astype(float)

    def device_batch(self, data_point_batch, device: int, pool):
        """(engine.DeviceFrames in a buffer of ``pool`` — acquire(nbytes, device) / release(buffer) —, y [n, 20] float): one
        th_voxelise_batch call on ``device``, nothing is downloaded"""
        from . import engine
        idx = self.rows_of(data_point_batch)
        dtype = np.dtype(np.float32 if self.gaussian else np.uint8)
        nbytes = max(1, len(idx) * int(np.prod(self.frame_dims)) * dtype.itemsize)
        buf = pool.acquire(nbytes, device)
        try:
            self._voxelise(idx, device, d_out=buf.ptr)
        except BaseException:
            pool.release(buf)
            raise
        return engine.DeviceFrames(buf, (len(idx), *self.frame_dims), dtype, on_release=pool.release), self.labels[idx].astype(float)
