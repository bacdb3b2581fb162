"""Rate of the voxeliser on --copies copies of tests/golden/1ubq.pdb1.gz (64 copies: 4864 frames of 21^3 x 5, Gaussian), frames left
in device memory:

  (a) one ``voxeliser.voxelise(..., d_out=...)`` call per structure (th_voxelise: the only way before th_voxelise_batch);
  (b) ``th_voxelise_batch``, at most --frames-per-call frames per call: wall time of the calls and the kernels' own time
      (events inside the call);
  (c) ``predict.py`` end to end with TIMED-synth (5 channels): on the directory of the copies (frames voxelised in HBM group by
      group) against a frame pack of the same frames (frames read from disk and copied over PCIe).  Skipped with --no-predict.

    python tools/bench_voxelise.py [--copies 64] [--frames-per-call 4096] [--reps 5] [--no-predict]

One JSON line per part.  (b) is expected to take no more wall time per frame than (a); (c) is a record, not a condition."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
UBQ = os.path.join(ROOT, "tests", "golden", "1ubq.pdb1.gz")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--frames-per-call", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-predict", action="store_true")
    a = ap.parse_args()
    from timed_hip import engine, pack, pdbio, structureset, synth, voxeliser
    work = tempfile.mkdtemp(prefix="bench_voxelise_")
    try:
        folder = os.path.join(work, "structures")
        os.mkdir(folder)
        for k in range(a.copies):
            shutil.copy(UBQ, os.path.join(folder, f"u{k:03d}.pdb1.gz"))
        xyz, ch, sg, frt, _rows = voxeliser.prepare_structure(pdbio.read_pdb(UBQ)[0])
        per, n = len(frt), len(frt) * a.copies
        frame_bytes = 21 ** 3 * 5 * 4
        d_out = engine.DeviceBuffer(min(n, max(per, a.frames_per_call)) * frame_bytes, a.device)
        voxeliser.voxelise(xyz, ch, sg, frt, device=a.device, d_out=d_out.ptr)                  # warm-up: module load
        walls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _k in range(a.copies):
                voxeliser.voxelise(xyz, ch, sg, frt, device=a.device, d_out=d_out.ptr)
            walls.append(time.perf_counter() - t0)
        wall_a = float(np.median(walls))
        print(json.dumps(dict(what="(a) th_voxelise, one call per structure", structures=a.copies, frames=n, reps=a.reps,
                              wall_ms_median=round(wall_a * 1e3, 3), wall_ms_min=round(min(walls) * 1e3, 3), us_per_frame=round(wall_a / n * 1e6, 3),
                              frames_per_s=float(f"{n / wall_a:.4g}"))), flush=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sset = structureset.StructureSet(folder)
        assert len(sset) == n
        spans = [(lo, min(lo + a.frames_per_call, n)) for lo in range(0, n, a.frames_per_call)]
        calls = [sset.batch_arrays(np.arange(lo, hi)) for lo, hi in spans]
        voxeliser.voxelise_batch(**calls[0], device=a.device, d_out=d_out.ptr)
        walls, kernels, gathers = [], [], []
        for _ in range(a.reps):
            timing = {}
            t0 = time.perf_counter()
            for kw in calls:
                voxeliser.voxelise_batch(**kw, device=a.device, d_out=d_out.ptr, timing=timing)
            walls.append(time.perf_counter() - t0)
            kernels.append(timing["kernel_ms"] / 1e3)
            t0 = time.perf_counter()
            for lo, hi in spans:
                sset.batch_arrays(np.arange(lo, hi))
            gathers.append(time.perf_counter() - t0)
        wall_b, kern_b = float(np.median(walls)), float(np.median(kernels))
        print(json.dumps(dict(what="(b) th_voxelise_batch", structures=a.copies, frames=n, calls=len(calls), frames_per_call=a.frames_per_call,
                              reps=a.reps, wall_ms_median=round(wall_b * 1e3, 3), wall_ms_min=round(min(walls) * 1e3, 3),
                              kernel_ms_median=round(kern_b * 1e3, 3), host_gather_ms_median=round(float(np.median(gathers)) * 1e3, 3),
                              us_per_frame=round(wall_b / n * 1e6, 3), us_per_frame_kernel=round(kern_b / n * 1e6, 3),
                              frames_per_s=float(f"{n / wall_b:.4g}"), wall_a_over_wall_b=round(wall_a / wall_b, 2),
                              no_slower_than_a=bool(wall_b <= wall_a))), flush=True)
        d_out.free()
        if a.no_predict:
            return
        import predict
        cfg, weights = synth.timed_synth(20, in_channels=5)
        model = os.path.join(work, "TIMED5.pack")
        with open(model, "wb") as f:
            f.write(pack.keras_to_pack(cfg, weights))
        stem = os.path.join(work, "frames")
        frames = np.lib.format.open_memmap(stem + ".frames.npy", mode="w+", dtype=np.float32, shape=(n, 21, 21, 21, 5))
        for lo, hi in spans:
            frames[lo:hi] = voxeliser.voxelise_batch(**sset.batch_arrays(np.arange(lo, hi)), device=a.device)
        frames.flush()
        del frames
        np.save(stem + ".labels.npy", sset.labels)
        np.savetxt(stem + ".map.txt", sset.flat_map, delimiter=",", fmt="%s")
        with open(stem + ".meta.json", "w") as f:
            json.dump(dict(frame_dims=[21, 21, 21, 5], voxels_as_gaussian=True, n_frames=n, source="bench", make_frame_dataset_ver=""), f)
        result = {}
        for name, dataset in (("directory", folder), ("frame_pack", stem + ".framepack")):
            times = []
            for rep in range(3):
                out = os.path.join(work, f"out_{name}_{rep}")
                os.mkdir(out)
                t0 = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    predict.load_dataset_and_predict([__import__("pathlib").Path(model)], dataset, dataset_map_path=os.path.join(out, "datasetmap.txt"),
                                                     path_to_output=out, device=a.device, frames_per_call=a.frames_per_call)
                times.append(time.perf_counter() - t0)
            result[name] = times
        same = open(os.path.join(work, "out_directory_0", "TIMED5.csv"), "rb").read() == open(os.path.join(work, "out_frame_pack_0", "TIMED5.csv"), "rb").read()
        print(json.dumps(dict(what="(c) predict.py, TIMED-synth 5 channels, every file written", frames=n, frames_per_call=a.frames_per_call,
                              directory_s=[round(t, 3) for t in result["directory"]], frame_pack_s=[round(t, 3) for t in result["frame_pack"]],
                              directory_frames_per_s=float(f"{n / min(result['directory']):.4g}"),
                              frame_pack_frames_per_s=float(f"{n / min(result['frame_pack']):.4g}"), same_csv_bytes=bool(same),
                              note="the directory run parses and prepares the structures inside the timed call")), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
