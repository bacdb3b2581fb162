#!/usr/bin/env python
"""Generate tests/golden/plan_snapshot.json — runs ONLY on the GPU box (plans are made at load, on the device).

Pins what the load-time planner (csrc/planner.hip, plan) produces: for every (model, load flags, knob set) of the corpus below,
each plan step's label, own FLOPs, issued FLOPs, bytes and direct-form FLOPs per frame, and the model's cost() totals.  All of
these are host arithmetic on shapes, so tests/test_gpu_plan_snapshot.py asserts exact equality.  Loads run with TH_GUARD=0:
the guard keeps its own tests.

The corpus: the eight CASES of tests/test_gpu_cnn.py under its five load modes and TH_LOAD_KEEP_ALL; every topology of
tools/plan_report.py at the default knobs; the four full-size topologies under each single-knob A/B row and the guard's
direct knob set.  The generator fails when the corpus misses a planner branch (MARKERS).

The file keeps each distinct step once ("steps": [label, flops, exec_flops, bytes, direct_flops]) and every record lists
indices into that table, so rows that share most of their plan stay small.

Usage:  python tests/golden/make_plan_snapshot.py
"""
import contextlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "timed-design_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from timed_hip import _lib, engine, synth  # noqa: E402

PATH = os.path.join(HERE, "plan_snapshot.json")
FULL = ["timed", "timed_rotamer", "densecpd", "prodconn"]
CNN_MODES = [("fused_mfma", 0, {}), ("fused_mfma_no_winograd", 0, {"TH_WINOGRAD": "0"}),
             ("fused_direct", _lib.TH_LOAD_NO_MFMA, {}),
             ("unfused_direct", _lib.TH_LOAD_NO_FUSE | _lib.TH_LOAD_NO_MFMA, {}),
             ("unfused_mfma", _lib.TH_LOAD_NO_FUSE, {}), ("keep_all", _lib.TH_LOAD_KEEP_ALL, {})]
KNOB_ROWS = [{"TH_WINOGRAD": "0"}, {"TH_WINOGRAD": "2"}, {"TH_WINO_SPLIT": "0"}, {"TH_WFUSED": "0"}, {"TH_WF_SPLIT": "0"},
             {"TH_FIRST_WINO": "0"}, {"TH_FIRST_SPLIT": "0"}, {"TH_CONV_GL": "0"}, {"TH_CONV_GL": "2"}, {"TH_DENSE_GEMM": "0"},
             {"TH_WF_NOBLK": "1"}, {"TH_WINO_NOMID": "1"}, {"TH_NO_TAIL_FUSE": "1"}, {"TH_NO_POOL_FIRST": "1"},
             {"TH_CONV_NOTAIL": "1"},
             # the load-time guard's reference plan (csrc/runtime.hip, guard_check)
             {"TH_WINO_SPLIT": "0", "TH_FIRST_SPLIT": "0", "TH_WF_SPLIT": "0", "TH_WINOGRAD": "0", "TH_WFUSED": "0",
              "TH_FIRST_WINO": "0"}]
# every branch of the planner shows up in at least one label
MARKERS = ["k_wino_in", "k_wino_gemm_b3", "k_wino_gemm]", "k_wino_mid", "wino_out + global_avg_pool", "[k_wino_out]",
           "k_conv_wfs", "k_conv_wf<", "k_conv_first5", "k_conv_first_w<", "k_conv_first<", "k_conv_first_b3",
           "k_conv_pw", "k_conv_gl", "conv3d_direct", "k_dense_gemm", ": dense", "k_tail_dense", "k_gap_softmax",
           "(input chunk-blocked)", "(output chunk-blocked)", "(direct form:"]


def _cnn_meta():
    z = np.load(os.path.join(HERE, "cnn_golden.npz"))
    return json.loads(str(z["meta"]))


def build_model(model):
    """(model_config, weights) of a corpus entry: "cnn:<case>" (tests/test_gpu_cnn.py) or "topo:<name>" (tools/plan_report.py)"""
    kind, name = model.split(":", 1)
    if kind == "cnn":
        m = next(x for x in _cnn_meta() if x["name"] == name)
        return getattr(synth, m["builder"])(**m["kwargs"])
    import plan_report
    return plan_report.variants()[name]()


def corpus():
    """[(model, flags, knobs)] in a fixed order"""
    out = []
    for m in _cnn_meta():
        for _, flags, knobs in CNN_MODES:
            out.append((f"cnn:{m['name']}", flags, knobs))
    import plan_report
    for name in plan_report.variants():
        out.append((f"topo:{name}", 0, {}))
    for knobs in KNOB_ROWS:
        for name in FULL:
            out.append((f"topo:{name}", 0, knobs))
    return out


@contextlib.contextmanager
def knob_env(knobs):
    """exactly these TH_* knobs (plus TH_GUARD=0) while a model loads; the caller's environment afterwards"""
    keep = {k: v for k, v in os.environ.items() if k.startswith("TH_") and k != "TH_GUARD_CACHE"}
    for k in keep:
        del os.environ[k]
    os.environ.update({"TH_GUARD": "0", **knobs})
    try:
        yield
    finally:
        for k in [k for k in os.environ if k.startswith("TH_") and k != "TH_GUARD_CACHE"]:
            del os.environ[k]
        os.environ.update(keep)


def plan_of(model, flags, knobs, device=0):
    """what the planner made: the cost() totals and one (label, flops, exec_flops, bytes, direct_flops) per step"""
    cfg, w = build_model(model)
    with knob_env(knobs):
        h = engine.HipFrameModel.from_keras(cfg, w, device=device, flags=flags)
    try:
        c = h.cost()
        steps = [[s["label"], s["flops"], s["exec_flops"], s["bytes"], s["direct_flops"]] for s in h.steps()]
    finally:
        h.close()
    return [c["algo_flops"], c["exec_flops"], c["n_steps"]], steps


def main():
    table, index, records = [], {}, []
    for model, flags, knobs in corpus():
        cost, steps = plan_of(model, flags, knobs)
        ids = []
        for s in steps:
            key = json.dumps(s)
            if key not in index:
                index[key] = len(table)
                table.append(s)
            ids.append(index[key])
        records.append(dict(model=model, flags=flags, knobs=knobs, cost=cost, steps=ids))
        print(f"{model:28s} flags {flags} {' '.join(f'{k}={v}' for k, v in knobs.items()) or '-':40s} {len(steps):3d} steps")
    missing = [mk for mk in MARKERS if not any(mk in s[0] for s in table)]
    if not any(re.search(r"\] x\d+ \+ conv_", s[0]) for s in table):
        missing.append("mfma step with a tail block")
    text = json.dumps(dict(steps=table, records=records), separators=(",", ":"))
    print(f"{len(records)} records, {len(table)} distinct steps, {len(text) / 1024:.0f} KB")
    with open(PATH, "w") as f:
        f.write(text + "\n")
    print(f"wrote {PATH}")
    if missing:
        raise SystemExit(f"the corpus misses planner branches: {missing}")


if __name__ == "__main__":
    main()
