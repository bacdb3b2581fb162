"""The oracle's Gaussian loop (oracle/voxel_oracle.py, spec item 6 of timed_hip/voxeliser.py) with a weight per atom (item 8): a
contribution is float32(weight * float32(w / total)), added in atom order.  Plain helper, no tests.  It returns the weighted frames
and the frames of |weight|: where contributions of both signs meet, only the second says how large the sums were that a difference
was rounded from.

The 27 weights of one atom are evaluated as one float32 array instead of one by one (the same float32 operations element by
element, the total still summed in the oracle's fixed order); tests/test_voxelise_batch_host.py holds the result against the
oracle at unit weights.

``batch(...)`` restates th_voxelise_batch on top of it: frame r from the atoms of structure frame_structure[r] alone."""
import numpy as np

from oracle import voxel_oracle

_OFFSETS = np.array([(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], np.int64)     # the oracle's order


def voxelise_weighted(atoms_xyz, atom_channel, atom_sigma, atom_weight, frames_rt, voxels_per_side=21, frame_edge_length=21.0, n_channels=5):
    f32 = np.float32
    xyz = np.asarray(atoms_xyz, dtype=f32).reshape(-1, 3)
    chn = np.asarray(atom_channel)
    sig = np.asarray(atom_sigma, dtype=f32)
    wgt = np.ones(len(xyz), f32) if atom_weight is None else np.asarray(atom_weight, dtype=f32)
    frt = np.asarray(frames_rt, dtype=f32).reshape(-1, 12)
    V = int(voxels_per_side)
    a = f32(frame_edge_length) / f32(V)
    centre = V // 2
    out = np.zeros((frt.shape[0], V, V, V, n_channels), dtype=f32)
    out_abs = np.zeros_like(out)
    for r in range(frt.shape[0]):
        loc, idx, inside = voxel_oracle.locate(xyz, frt[r], V, frame_edge_length)
        for k in np.nonzero(inside)[0]:                                   # atom order
            c = int(chn[k])
            if not 0 <= c < n_channels:
                continue
            inv2s2 = f32(1.0) / (f32(2.0) * sig[k] * sig[k])
            v = idx[k][None, :] + _OFFSETS
            e = (v - centre).astype(f32) * a - loc[k][None, :]
            r2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            w = np.exp(-(r2 * inv2s2), dtype=f32)
            total = f32(0.0)
            for val in w:                                                 # fixed order: dz, dy, dx
                total = f32(total + val)
            part = (wgt[k] * (w / total).astype(f32)).astype(f32)         # the quotient rounded, then the product
            ok = np.all((v >= 0) & (v < V), axis=1)
            i0, i1, i2 = v[ok, 0], v[ok, 1], v[ok, 2]                     # 27 different voxels: one addition each
            out[r, i0, i1, i2, c] = out[r, i0, i1, i2, c] + part[ok]
            out_abs[r, i0, i1, i2, c] = out_abs[r, i0, i1, i2, c] + np.abs(part[ok])
    return out, out_abs


def batch(atoms_xyz, atom_channel, atom_sigma, atom_weight, atom_offsets, frames_rt, frame_structure, voxels_per_side=21,
          frame_edge_length=21.0, n_channels=5, gaussian=True):
    """th_voxelise_batch restated: (frames, frames of |weight|) for Gaussian frames, (uint8 frames, None) for boolean ones"""
    xyz, chn, sig = np.asarray(atoms_xyz, np.float32).reshape(-1, 3), np.asarray(atom_channel), np.asarray(atom_sigma, np.float32)
    wgt = None if atom_weight is None else np.asarray(atom_weight, np.float32)
    frt, off = np.asarray(frames_rt, np.float32).reshape(-1, 12), np.asarray(atom_offsets)
    V = int(voxels_per_side)
    out = np.zeros((len(frt), V, V, V, n_channels), np.float32 if gaussian else np.uint8)
    out_abs = np.zeros_like(out) if gaussian else None
    for r, s in enumerate(np.asarray(frame_structure).tolist()):
        lo, hi = int(off[s]), int(off[s + 1])
        if gaussian:
            out[r], out_abs[r] = (x[0] for x in voxelise_weighted(xyz[lo:hi], chn[lo:hi], sig[lo:hi], None if wgt is None else wgt[lo:hi],
                                                                  frt[r:r + 1], V, frame_edge_length, n_channels))
        else:
            out[r] = voxel_oracle.voxelise(xyz[lo:hi], chn[lo:hi], sig[lo:hi], frt[r:r + 1], V, frame_edge_length, n_channels, False)[0]
    return out, out_abs
