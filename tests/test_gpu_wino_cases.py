"""Every GEMM x scheme cell of csrc/conv_wino.hip on the GPU: the rows of tests/wino_cases.py (tests/test_wino_cases_host.py shows
without a GPU that they reach every chunk count, column block, row block, idle wave and ragged workgroup of the four GEMM kernels,
k_wino_gemm — the fp32-input GEMM of TH_WINO_SPLIT=0 — among them).  Per row, under its environment:
  * the GEMM step of the row's layer carries the row's markers (the bracketed kernel name, the scheme, the padded K), the handle's
    knobs are the row's, and the load-time guard PASSED: a wrong fast kernel trips the guard, the model then runs the direct plan
    and every comparison below would hold on a kernel that never ran;
  * `keep` rows: the layer's tensor against cnn_oracle.forward in float64, with the bounds of tests/test_gpu_wino.py (per element
    1e-5 max(1, max|y|), rms 3e-6, probabilities 5e-6; F(5,3): 1e-4, 1.5e-5, 2e-5), at most 8 frames;
  * `gap` / `mid` rows: probabilities against the oracle, and the same bits as the plan without the fusion (TH_NO_TAIL_FUSE=1 /
    TH_WINO_NOMID=1);
  * more than 8 frames: all of them against the direct plan (TH_WINOGRAD=0) at the probability bound;
  * a frame's result does not depend on its neighbours: predict(frames[perm]) == predict(frames)[perm] and the same bits under
    set_chunk(c) with a c that does not divide n.
Each row prints its measured errors (profiles/conv_wino_cases.txt)."""
import os
import sys

import numpy as np
import pytest

from oracle import cnn_oracle
from timed_hip import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu


def _gemm_labels(labels, conv):
    return [l for l in labels if l.startswith(conv + ": conv_wino<")]


def _load(cfg, weights, gpu):
    model = engine.HipFrameModel.from_keras(cfg, weights, device=gpu)
    return model, [s["label"] for s in model.steps()]


@pytest.mark.parametrize("r", wc.ROWS, ids=wc.row_id)
def test_wino_row(gpu, monkeypatch, r):
    for k, v in {**wc.env_of(r), **wc.tail_env(r)}.items():
        monkeypatch.setenv(k, v)
    net, frames, mk = wc.build(r), wc.frames(r), wc.markers(r)
    per_element, rms_bound, prob_bound = wc.BOUNDS[r.scheme]
    k = min(r.n, 8)
    ref = cnn_oracle.forward(net.cfg, net.weights, frames[:k], np.float64, return_all=True)
    want_probs = ref[list(ref)[-1]]

    # ---- plan and guard ----
    model, labels = _load(net.cfg, net.weights, gpu)
    gemm = _gemm_labels(labels, net.conv)
    assert len(gemm) == 1 and mk.kernel in gemm[0], labels
    assert all(s in gemm[0] for s in mk.label) and not any(s in gemm[0] for s in mk.no_label), (gemm[0], mk)
    knobs, guard = model.knobs(), model.guard()
    assert guard["state"] == 1 and "guard:" not in knobs, (guard, knobs)
    assert all(s in knobs for s in mk.knobs) and not any(s in knobs for s in mk.no_knobs), (knobs, mk)
    if r.tail == "gap":
        assert any(l.startswith(net.conv + ": wino_out + global_avg_pool") for l in labels), labels
    if r.tail == "mid":
        assert any(l.startswith(net.conv + ": wino_mid") for l in labels) and len(_gemm_labels(labels, net.next_conv)) == 1, labels
        assert not any(l.startswith(net.next_conv + ": wino_in") for l in labels), labels

    # ---- against the float64 oracle ----
    probs = model.predict(frames)
    logits = model.predict(frames, logits=True)
    assert np.isfinite(probs).all() and np.isfinite(logits).all()
    line = f"{r.id:<34} {mk.kernel:<18} F{'(5,3)' if r.scheme == 7 else '(3,3)+F(2,3)':<13}"
    if r.tail == "keep":
        want = ref[net.layer]
        got = model.fetch(net.layer, k, (5, 5, 5, r.cout))
        scale = max(1.0, float(np.abs(want).max()))
        err, rms = float(np.abs(got - want).max()), float(np.sqrt(np.mean((got - want) ** 2)))
        line += f" layer max {err:.3e} = {err / scale:.2e} of {scale:6.3f}  rms {rms:.2e}"
    perr = float(np.abs(probs[:k] - want_probs).max())
    print(f"\n{line}  probs {perr:.2e}  guard dlogit {guard['max_dlogit']:.2e}")
    if r.tail == "keep":
        assert err <= per_element * scale and rms < rms_bound, (err, scale, rms)
    assert perr <= prob_bound, perr

    # ---- a frame's result does not depend on its neighbours ----
    perm = np.random.default_rng(r.n).permutation(r.n)
    assert np.array_equal(model.predict(frames[perm]), probs[perm]) and np.array_equal(model.predict(frames[perm], logits=True), logits[perm])
    c = wc.chunk_for(r.n)
    if c is not None:
        model.set_chunk(c)
        assert np.array_equal(model.predict(frames), probs) and np.array_equal(model.predict(frames, logits=True), logits), c
    model.close()

    # ---- the plan without the fusion: the same bits ----
    if r.tail in ("gap", "mid"):
        monkeypatch.setenv("TH_NO_TAIL_FUSE" if r.tail == "gap" else "TH_WINO_NOMID", "1")
        plain, plabels = _load(net.cfg, net.weights, gpu)
        assert len(_gemm_labels(plabels, net.conv)) == 1 and plain.guard()["state"] == 1, plabels
        assert not any("global_avg_pool (" in l for l in plabels) if r.tail == "gap" else not any("k_wino_mid" in l for l in plabels), plabels
        assert np.array_equal(plain.predict(frames), probs) and np.array_equal(plain.predict(frames, logits=True), logits)
        plain.close()

    # ---- every row block and the ragged last one: against the direct kernels ----
    if r.n > 8:
        monkeypatch.setenv("TH_WINOGRAD", "0")
        direct, dlabels = _load(net.cfg, net.weights, gpu)
        assert not any("conv_wino" in l for l in dlabels), dlabels
        np.testing.assert_allclose(probs, direct.predict(frames), atol=prob_bound, rtol=0)
        direct.close()


@pytest.mark.parametrize("scheme", wc.SCHEMES)
def test_a_narrow_layer_is_no_winograd_layer_without_split_operands(gpu, monkeypatch, scheme):
    """wino_cases.UNREACHABLE: under TH_WINO_SPLIT=0 conv_wino_plan refuses the 128 -> 20 layer that k_wino_gemm_n32 takes by default"""
    r = next(x for x in wc.ROWS if x.gemm == "n32" and x.scheme == scheme and (x.cin, x.cout, x.tail, x.arena) == (128, 20, "keep", "none"))
    for k, v in {**wc.env_of(r), **wc.tail_env(r)}.items():
        monkeypatch.setenv(k, v)
    net = wc.build(r)
    model, labels = _load(net.cfg, net.weights, gpu)
    assert len(_gemm_labels(labels, net.conv)) == 1, labels
    model.close()
    monkeypatch.setenv("TH_WINO_SPLIT", "0")
    assert ("n32", "TH_WINO_SPLIT=0") in wc.UNREACHABLE
    model, labels = _load(net.cfg, net.weights, gpu)
    assert not any("conv_wino" in l or "k_wino" in l for l in labels), labels
    model.close()
