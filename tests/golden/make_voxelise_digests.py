"""Writes tests/golden/voxelise_digests.json: shape, dtype and SHA-256 of the frames ``voxeliser.voxelise`` (th_voxelise) returns for
the cases of tests/voxel_cases.py::digest_cases and for the 76 five-channel frames of 1ubq, together with the commit, the HIP
version and the device they were recorded on.

The committed file was recorded at commit 51dee49, the last one at which th_voxelise had a kernel of its own (k_voxelise, the
all-atoms gather): tests/test_gpu_voxelise_batch.py holds both th_voxelise and th_voxelise_batch, which share one kernel since, to
those bytes.

The boolean digests can never move.  The Gaussian ones carry the device library's expf: if a ROCm upgrade moves them while the
oracle tests (tests/test_gpu_voxelise_sweep.py, tests/test_voxeliser.py) still pass, this file is regenerated and the commit says so.

    python tests/golden/make_voxelise_digests.py --commit HASH [--out FILE] [--device 0]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "timed-design_amd"), os.path.join(ROOT, "tests")]


def hip_version():
    try:
        import torch
        if torch.version.hip:
            return "torch.version.hip " + torch.version.hip
    except ImportError:
        pass
    import subprocess
    return subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True).stdout.strip()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "voxelise_digests.json"))
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import voxel_cases as vc
    from timed_hip import _lib, pdbio, voxeliser
    cases = {}
    for case_id, cloud, V, edge, C, gaussian in vc.digest_cases():
        cases[case_id] = vc.digest(voxeliser.voxelise(*cloud, V, edge, C, gaussian, device=a.device))
    xyz, ch, sg, frt, _rows = voxeliser.prepare_structure(pdbio.read_pdb(os.path.join(HERE, "1ubq.pdb1.gz"))[0])
    cases[vc.UBQ_DIGEST] = vc.digest(voxeliser.voxelise(xyz, ch, sg, frt, device=a.device))
    name, arch, _cus = _lib.device_info(a.device)
    head = dict(commit=a.commit, entry_point="th_voxelise (voxeliser.voxelise)", hip=hip_version(),
                device=f"{name.strip() or 'no marketing name reported'} ({arch})")
    write(head, cases, a.out)
    print(f"{len(cases)} digests -> {a.out}")


def write(head, cases, path):
    """one case per line"""
    lines = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in cases.items())
    with open(path, "w") as f:
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": {\n' + lines + "\n }\n}\n")


if __name__ == "__main__":
    main()
