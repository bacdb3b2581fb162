#!/usr/bin/env python
"""A/B of the split Winograd GEMM variants (k_wino_gemm_b3, TH_WINO_B3VAR) in ONE process: one-layer models (5^3, 3x3x3 'same',
Conv -> ELU -> BN) loaded once per variant, timed alternately (the variant order reversed every other repeat) on the same random
frames; the GEMM plan step's device time per 4096 frames from the per-step HIP events.

    python tools/bench_wino_b3.py [--vars 0,2] [--reps 3] [--frames 8192] [--iters 4] 64:128 128:128 128:256 256:338"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
from timed_hip import engine, synth


def gemm_ms(m):
    return sum(s["ms"] for s in m.steps() if "k_wino_gemm_b3" in s["label"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vars", default="0,2")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=4, help="forward passes per timed sample")
    ap.add_argument("shapes", nargs="*", default=["64:128", "128:128", "128:256", "256:338"])
    args = ap.parse_args()
    variants = args.vars.split(",")
    n = args.frames
    rows = []
    for shape in args.shapes:
        cin, cout = (int(x) for x in shape.split(":"))
        b = synth.KerasGraphBuilder((5, 5, 5, cin), seed=1)
        x = b.batchnorm(b.elu(b.conv3d(b.input_name, cout, 3, padding="same")))
        cfg, w = b.finish(b.softmax(b.gap(x)))
        fr = np.random.default_rng(0).random((n, 5, 5, 5, cin), dtype=np.float32)
        d_in = engine.DeviceBuffer(fr.nbytes); d_in.upload(fr)
        d_out = engine.DeviceBuffer(n * cout * 4)
        models = {}
        for v in variants:
            os.environ["TH_WINO_B3VAR"] = v                       # read once, at load
            m = engine.HipFrameModel.from_keras(cfg, w)
            m.set_chunk(4096)
            assert any("k_wino_gemm_b3" in s["label"] for s in m.steps()), "no split Winograd GEMM in the plan"
            m.profile(1)
            for _ in range(2):                                    # warm-up
                m.predict_device(d_in.ptr, n, d_out.ptr)
            models[v] = m
        os.environ.pop("TH_WINO_B3VAR", None)
        samples = {v: [] for v in variants}
        for r in range(args.reps):
            for v in (variants if r % 2 == 0 else variants[::-1]):
                m = models[v]
                t0 = gemm_ms(m)
                for _ in range(args.iters):
                    m.predict_device(d_in.ptr, n, d_out.ptr)
                samples[v].append((gemm_ms(m) - t0) / args.iters * 4096 / n)
        for v in variants:
            s = sorted(samples[v])
            row = dict(cin=cin, cout=cout, var=v, ms_per_4096=s, median=s[len(s) // 2])
            rows.append(row)
            print(json.dumps(row), flush=True)
        for m in models.values():
            m.close()
    print("\n| layer | " + " | ".join(f"B3VAR={v} ms / 4096 (min-max)" for v in variants) + " | new / old |")
    print("|---|" + "---|" * (len(variants) + 1))
    for shape in args.shapes:
        cin, cout = (int(x) for x in shape.split(":"))
        rs = {r["var"]: r for r in rows if (r["cin"], r["cout"]) == (cin, cout)}
        cells = [f"{rs[v]['median']:.3f} ({min(rs[v]['ms_per_4096']):.3f}-{max(rs[v]['ms_per_4096']):.3f})" for v in variants]
        ratio = " / ".join(f"{rs[v]['median'] / rs[variants[0]]['median']:.3f}" for v in variants[1:])
        print(f"| {cin} -> {cout} | " + " | ".join(cells) + f" | {ratio} |")


if __name__ == "__main__":
    main()
