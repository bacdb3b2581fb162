"""The load-time guard (csrc/guard.hip, guard_check; include/timed_hip.h th_model_guard_info) and the per-handle knobs.

Every th_model_load checks the plan it built — Cook-Toom / Winograd layers, the bf16x3-split GEMMs — against a direct fp32-MFMA
plan of the same pack on four internally generated frames; logits must agree to 1e-5 x max(1, max |logit|), otherwise fast
features are dropped until they do.  Why: parity is unpinned against TensorFlow and real `.h5` weights have never been seen
(reference predict.py:121), so the error figures of the fast forms come from synthetic weights only."""
import json
import os
import re

import numpy as np
import pytest

from oracle import cnn_oracle
from timed_hip import _lib, engine, synth

pytestmark = pytest.mark.gpu
TIGHT = 5e-6


def _labels(model):
    return [s["label"] for s in model.steps()]


def _fast(labels):
    """the steps that run a minimal-filtering or split-operand kernel, judged by the bracketed kernel name that ends each label
    (a label starts with the user's layer name, which may look like a kernel's)"""
    kernels = [re.search(r"\[([^\]]+)\]\s*$", l) for l in labels]
    return [l for l, k in zip(labels, kernels)
            if k and k.group(1).startswith(("k_wino_", "k_conv_wf", "k_conv_first_w", "k_conv_first_b3"))]


def test_guard_passes_on_the_benchmark_topologies(gpu):
    """default plans of the three BASELINE topologies: the guard ran, passed, and measured a distance far inside its bound"""
    for build in (lambda: synth.timed_synth(20), lambda: synth.timed_synth(338), lambda: synth.densecpd_synth(20)):
        cfg, w = build()
        model = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
        g = model.guard()
        assert g["state"] == 1 and (g["note"].startswith("[") or "earlier load" in g["note"]), g     # passed: timing (or a remembered pass) only
        assert g["logit_scale"] > 0
        assert g["max_dlogit"] <= 1e-5 * max(1.0, g["logit_scale"]), g
        assert _fast(_labels(model)), "the default plan has fast steps to guard"
        assert model.knobs() == ""
        model.close()


def test_guard_off_and_nothing_to_check(gpu, monkeypatch):
    cfg, w = synth.timed_synth(20)
    monkeypatch.setenv("TH_GUARD", "0")
    model = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
    assert model.guard()["state"] == 0 and "TH_GUARD=0" in model.knobs()
    model.close()
    monkeypatch.delenv("TH_GUARD")
    monkeypatch.setenv("TH_WINOGRAD", "0")
    monkeypatch.setenv("TH_WFUSED", "0")
    monkeypatch.setenv("TH_FIRST_WINO", "0")
    model = engine.HipFrameModel.from_keras(cfg, w, device=gpu)            # a direct plan: no fast step, the guard has nothing to do
    assert model.guard()["state"] == 0 and not _fast(_labels(model))
    model.close()
    # the same direct plan with a convolution whose name reads like a fast kernel's: layer names do not make a plan "fast"
    named = json.loads(json.dumps(cfg).replace('"conv3d"', '"k_conv_first5_x"'))
    wn = {("k_conv_first5_x" if k == "conv3d" else k): v for k, v in w.items()}
    model = engine.HipFrameModel.from_keras(named, wn, device=gpu)
    labels = _labels(model)
    assert any(l.startswith("k_conv_first5_x: ") for l in labels), labels
    assert model.guard()["state"] == 0 and not _fast(labels)
    model.close()


@pytest.mark.parametrize("classes", [20, 338])
def test_forced_trip_falls_back_to_the_direct_plan_and_keeps_parity(gpu, cnn_golden, monkeypatch, classes):
    """an impossible tolerance trips the guard on every stage: the handle that comes back runs the direct fp32 kernels, says so,
    and still meets the fixture bound"""
    monkeypatch.setenv("TH_GUARD_TOL", "1e-12")
    z, meta = cnn_golden
    name = f"timed{classes}"
    m = next(x for x in meta if x["name"] == name)
    cfg, weights = getattr(synth, m["builder"])(**m["kwargs"])
    frames = synth.synthetic_frames(m["n"], **m["frame_kwargs"])
    model = engine.HipFrameModel.from_keras(cfg, weights, device=gpu)
    g = model.guard()
    assert g["state"] == 2, g
    for key in ("TH_WINO_SPLIT=0", "TH_FIRST_SPLIT=0", "TH_WINOGRAD=0", "TH_WFUSED=0", "TH_FIRST_WINO=0"):
        assert key in g["note"], g
    assert "guard:" in model.knobs()
    assert not _fast(_labels(model)), _labels(model)
    probs = model.predict(frames)
    np.testing.assert_allclose(probs, z[f"{name}__torch64"], atol=TIGHT, rtol=0)
    np.testing.assert_allclose(model.predict(frames, logits=True), z[f"{name}__logits64"], atol=TIGHT, rtol=0)
    model.close()


def test_partial_trip_drops_only_what_is_needed(gpu, monkeypatch):
    """a tolerance between the split GEMM's distance from the direct plan and zero... is not constructible portably, so the
    staging is exercised through the knobs instead: with the split GEMM already off the first fallback stage is skipped"""
    monkeypatch.setenv("TH_GUARD_TOL", "1e-12")
    monkeypatch.setenv("TH_WINO_SPLIT", "0")
    cfg, w = synth.timed_synth(20)
    model = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
    g = model.guard()
    assert g["state"] == 2 and "TH_WINO_SPLIT=0 " not in g["note"].split("->")[1], g
    model.close()


def _adversarial_timed(seed):
    """TIMED-synth with badly scaled parameters: every convolution kernel gets a per-tap gain spread over three decades
    (1e-2 .. 1e1, renormalised to the He scale), every BatchNorm gamma / beta pair is scaled per channel over four decades
    (1e-2 .. 1e2): channels of very different magnitude meet in every following convolution"""
    cfg, w = synth.timed_synth(20)
    rng = np.random.default_rng(seed)
    for k in sorted(w):
        arrs = w[k]
        if k.startswith("conv3d") and arrs[0].ndim == 5:
            gain = 10.0 ** rng.uniform(-2, 1, size=arrs[0].shape[:3] + (1, 1))
            arrs[0] = (arrs[0] * gain / np.sqrt(np.mean(gain ** 2))).astype(np.float32)
        if k.startswith("batch_normalization"):
            g = 10.0 ** rng.uniform(-2, 2, size=arrs[0].shape)
            arrs[0] = (arrs[0] * g).astype(np.float32)               # gamma
            arrs[1] = (arrs[1] * g).astype(np.float32)               # beta
    return cfg, w


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_adversarial_weights_stay_within_the_bound_whatever_the_guard_decides(gpu, seed):
    """kernels with a 1e3 dynamic range across taps and BatchNorm gammas over four decades: whatever plan the guard keeps, its
    logits are within TIGHT x max(1, max |logit|) of the float64 oracle, and a trip is reported with its measurements"""
    cfg, w = _adversarial_timed(seed)
    frames = synth.synthetic_frames(4, seed=seed)
    model = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
    g = model.guard()
    assert g["state"] in (1, 2)
    if g["state"] == 2:
        assert g["note"] and "kept with" in g["note"], g
    ref = cnn_oracle.forward(cfg, w, frames, np.float64, return_all=True)
    logit_layer = [k for k in ref if "global_average" in k][-1]
    want = ref[logit_layer]
    got = model.predict(frames, logits=True)
    scale = max(1.0, float(np.abs(want).max()))
    assert np.isfinite(want).all()
    np.testing.assert_allclose(got, want, atol=TIGHT * scale, rtol=0)
    # and the kept plan is as close to the direct plan as the guard says
    assert g["max_dlogit"] <= 1e-5 * max(1.0, g["logit_scale"]) or g["state"] == 2
    model.close()


def test_knobs_belong_to_the_handle_not_to_the_process(gpu, monkeypatch):
    """TH_* knobs are read once, by th_model_load, into the handle: a model loaded under TH_WINOGRAD=0 keeps its direct kernels
    after the variable is gone, a model loaded afterwards gets the default plan, and neither changes when the environment does"""
    cfg, w = synth.timed_synth(20)
    frames = synth.synthetic_frames(3, seed=5)
    monkeypatch.setenv("TH_WINOGRAD", "0")
    monkeypatch.setenv("TH_WF_RESIDENT", "7")
    a = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
    monkeypatch.delenv("TH_WINOGRAD")
    monkeypatch.delenv("TH_WF_RESIDENT")
    b = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
    assert "TH_WINOGRAD=0" in a.knobs() and "TH_WF_RESIDENT=7" in a.knobs() and b.knobs() == ""
    assert not any("conv_wino" in l for l in _labels(a)) and any("conv_wino" in l for l in _labels(b))
    pa, pb = a.predict(frames), b.predict(frames)
    monkeypatch.setenv("TH_WINOGRAD", "0")               # a later change reaches neither handle
    monkeypatch.setenv("TH_WFUSED", "0")                 # (it would change b's plan and bits if it reached b)
    assert np.array_equal(a.predict(frames), pa) and np.array_equal(b.predict(frames), pb)
    np.testing.assert_allclose(pa, pb, atol=TIGHT, rtol=0)
    a.close(); b.close()


KNOCKOUT_VARS = ("TH_WF_DBG", "TH_FIRST_DBG", "TH_WINO_DBG", "TH_CONV_DBG", "TH_PW_DBG")


def test_the_product_library_refuses_knockout_variables(gpu, monkeypatch):
    """the timing knock-outs live in a build of their own (tools/build_knockouts.py): the product library has none, and a model
    load under a set TH_*_DBG variable fails, naming it, instead of timing the whole kernels; unset, empty or 0 loads as ever"""
    cfg, w = synth.timed_synth(20, widths=(4,), side=5, in_channels=2)
    for var in KNOCKOUT_VARS:
        monkeypatch.setenv(var, "1")
        with pytest.raises(_lib.TimedHipError) as e:
            engine.HipFrameModel.from_keras(cfg, w, device=gpu)
        assert e.value.code == _lib.TH_EINVAL and var in str(e.value), (var, str(e.value))
        for ok in ("0", "", None):
            monkeypatch.setenv(var, ok) if ok is not None else monkeypatch.delenv(var)
            model = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
            assert model.knobs() == "", (var, ok, model.knobs())
            model.close()


def test_a_pass_is_remembered_for_the_same_pack_knobs_and_device(gpu):
    """the second load of the same pack under the same knobs costs a hash, not a second plan: the verdict and its measurements
    are the first load's; other knobs, or another model, are measured on their own"""
    cfg, w = synth.timed_synth(20, seed=999)                   # a pack no other test loads
    a = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
    ga = a.guard()
    b = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
    gb = b.guard()
    assert ga["state"] == gb["state"] == 1 and "earlier load" not in ga["note"] and "earlier load" in gb["note"]
    assert gb["max_dlogit"] == ga["max_dlogit"] and gb["logit_scale"] == ga["logit_scale"]
    frames = synth.synthetic_frames(2, seed=4)
    assert np.array_equal(a.predict(frames), b.predict(frames))
    a.close(); b.close()
    os.environ["TH_WINO_SPLIT"] = "0"
    try:
        c = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
        assert "earlier load" not in c.guard()["note"]
        c.close()
    finally:
        del os.environ["TH_WINO_SPLIT"]


DISK_WORKER = """
import os, sys
sys.path.insert(0, os.path.join({root!r}, "timed-design_amd"))
from timed_hip import engine, synth
cfg, w = synth.timed_synth(20, seed=998)
m = engine.HipFrameModel.from_keras(cfg, w, device=0)
g = m.guard()
print("GUARD", g["state"], repr(g["max_dlogit"]), repr(g["logit_scale"]), "|", g["note"])
"""


def test_a_pass_is_remembered_across_processes_in_a_verdict_file(gpu, tmp_path):
    """predict.py loads one model per process: the second PROCESS that loads the same pack under the same knobs, on the same
    device, with the same build of the library reads the verdict from $TH_GUARD_CACHE instead of building a second plan;
    other knobs miss; TH_GUARD_CACHE=0 writes nothing; a damaged file is a miss, not an error"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "w.py"
    script.write_text(DISK_WORKER.format(root=root))
    cache = tmp_path / "verdicts"

    def run(**env):
        e = dict(os.environ, TH_GUARD_CACHE=str(cache))
        e.update(env)
        r = subprocess.run([sys.executable, str(script)], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
        line = [l for l in r.stdout.splitlines() if l.startswith("GUARD")][0]
        head, note = line.split("|", 1)
        return head.split()[1:], note

    a, na = run()
    files = sorted(cache.iterdir())
    assert a[0] == "1" and "earlier" not in na and len(files) == 1 and files[0].name.startswith("guard-")
    b, nb = run()
    assert b == a and "earlier process" in nb and sorted(cache.iterdir()) == files
    c, nc = run(TH_WINO_SPLIT="0")                                  # other knobs: measured on their own, a second file
    assert "earlier" not in nc and len(list(cache.iterdir())) == 2
    files[0].write_text("garbage\n")
    d, nd = run()
    assert d == a and "earlier" not in nd                           # damaged: measured again (and rewritten)
    e, ne = run()
    assert "earlier process" in ne
    off = tmp_path / "off"
    f, nf = run(TH_GUARD_CACHE="0", XDG_CACHE_HOME=str(off))
    assert "earlier" not in nf and not (off / "timed_hip").exists()      # (the ROCm runtime may create XDG_CACHE_HOME itself)
