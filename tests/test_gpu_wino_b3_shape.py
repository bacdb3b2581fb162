"""The split Winograd GEMM on v_mfma_f32_16x16x32_bf16 (k_wino_gemm_b3<2>, the default; TH_WINO_B3VAR=0 keeps the 32x32x16 kernel).

The products and the fp32 accumulation are those of variant 0, only the summation order inside the MFMA differs: both variants
are held to the float64 oracle per element at the bounds of tests/test_gpu_wino.py, and to each other.  Shapes: every Cin / Cout
of the wide 5^3 layers (338 columns = 2 x 128 + 82: a padding-only wave), frame counts on both sides of the 64-frame row block,
and a 4096-frame chunk followed by a ragged tail."""
import numpy as np
import pytest

from oracle import cnn_oracle
from timed_hip import engine, synth

pytestmark = pytest.mark.gpu
TIGHT = 5e-6
LAYER = 1e-5          # per element, x max|y| of the layer (tests/test_gpu_wino.py: accumulation noise on dense inputs)
NEW = "2"             # the 16x16x32 variant
VARIANTS = ["0", NEW]


def _one_layer(cin, cout, seed):
    b = synth.KerasGraphBuilder((5, 5, 5, cin), seed=seed)
    x = b.batchnorm(b.elu(b.conv3d(b.input_name, cout, 3, padding="same")))
    name = x
    cfg, w = b.finish(b.softmax(b.gap(x)))
    rng = np.random.default_rng(seed + 1)
    for k, arrs in w.items():                 # the builder's biases are zero: make them count
        if k.startswith("conv3d") and len(arrs) == 2:
            arrs[1] = rng.normal(0, 0.2, arrs[1].shape).astype(np.float32)
    return cfg, w, name


def _frames(n, cin, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 5, 5, 5, cin)) * (rng.random((n, 5, 5, 5, cin)) < 0.5)).astype(np.float32)


def _load(cfg, w, gpu, monkeypatch, var):
    monkeypatch.setenv("TH_WINO_B3VAR", var)
    m = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
    labels = [s["label"] for s in m.steps()]
    assert any("k_wino_gemm_b3" in l for l in labels), labels
    return m


def _check_layer(got, want):
    np.testing.assert_allclose(got, want, atol=LAYER * max(1.0, float(np.abs(want).max())), rtol=0)
    assert float(np.sqrt(np.mean((got - want) ** 2))) < 3e-6


@pytest.mark.parametrize("var", VARIANTS)
@pytest.mark.parametrize("cin,cout,n", [(64, 128, 1), (128, 128, 63), (128, 256, 65), (256, 338, 65), (64, 338, 63),
                                        (256, 128, 1), (256, 256, 63)])
def test_layer_matches_the_float64_oracle(gpu, monkeypatch, var, cin, cout, n):
    """Conv -> ELU -> BN, the layer's tensor per element and the probabilities against the float64 oracle"""
    monkeypatch.setenv("TH_NO_TAIL_FUSE", "1")     # the layer's tensor is fetched below
    cfg, w, layer = _one_layer(cin, cout, seed=cin + cout)
    frames = _frames(n, cin, seed=n)
    m = _load(cfg, w, gpu, monkeypatch, var)
    probs = m.predict(frames)
    k = min(n, 8)
    ref = cnn_oracle.forward(cfg, w, frames[:k], np.float64, return_all=True)
    _check_layer(m.fetch(layer, k, (5, 5, 5, cout)), ref[layer])
    np.testing.assert_allclose(probs[:k], ref[list(ref)[-1]], atol=TIGHT, rtol=0)
    m.close()


@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 256), (256, 338)])
def test_full_chunk_and_ragged_tail(gpu, monkeypatch, cin, cout):
    """4096 + 37 frames (one full chunk, then a 37-frame launch): the tail's layer tensor against the oracle for both variants,
    every frame's probabilities of the new variant against the old"""
    monkeypatch.setenv("TH_NO_TAIL_FUSE", "1")
    cfg, w, layer = _one_layer(cin, cout, seed=3 * cin + cout)
    n = 4096 + 37
    frames = _frames(n, cin, seed=cin)
    ref = cnn_oracle.forward(cfg, w, frames[4096:4096 + 6], np.float64, return_all=True)
    probs = {}
    for var in VARIANTS:
        m = _load(cfg, w, gpu, monkeypatch, var)
        m.set_chunk(4096)
        probs[var] = m.predict(frames)
        _check_layer(m.fetch(layer, 6, (5, 5, 5, cout)), ref[layer])      # the first frames of the LAST chunk: the tail
        np.testing.assert_allclose(probs[var][4096:4096 + 6], ref[list(ref)[-1]], atol=TIGHT, rtol=0)
        m.close()
    np.testing.assert_allclose(probs[NEW], probs["0"], atol=TIGHT, rtol=0)


@pytest.mark.parametrize("cin,cout,n", [(128, 256, 200), (256, 338, 130)])
def test_new_variant_against_the_old(gpu, monkeypatch, cin, cout, n):
    """the layer's whole tensor, new against old: two fp32 summation orders of the same piece products"""
    monkeypatch.setenv("TH_NO_TAIL_FUSE", "1")
    cfg, w, layer = _one_layer(cin, cout, seed=cin + 2 * cout)
    frames = _frames(n, cin, seed=7)
    got = {}
    for var in VARIANTS:
        m = _load(cfg, w, gpu, monkeypatch, var)
        m.predict(frames)
        got[var] = m.fetch(layer, n, (5, 5, 5, cout))
        m.close()
    _check_layer(got[NEW], got["0"].astype(np.float64))


def test_default_is_the_new_variant(gpu, monkeypatch):
    """unset, TH_WINO_B3VAR selects the 16x16x32 kernel: same bits as TH_WINO_B3VAR=2, and 0 differs (the summation order)"""
    cfg, w, _ = _one_layer(128, 256, seed=5)
    frames = _frames(70, 128, seed=5)
    monkeypatch.delenv("TH_WINO_B3VAR", raising=False)
    m = engine.HipFrameModel.from_keras(cfg, w, device=gpu)
    dflt = m.predict(frames, logits=True)
    m.close()
    out = {}
    for var in VARIANTS:
        m = _load(cfg, w, gpu, monkeypatch, var)
        out[var] = m.predict(frames, logits=True)
        m.close()
    assert np.array_equal(dflt, out[NEW])
    assert not np.array_equal(dflt, out["0"])


@pytest.mark.parametrize("name", ["timed20", "timed338"])
def test_timed_fixtures_under_the_default(gpu, cnn_golden, monkeypatch, name):
    """the torch-fp64 fixtures with the default plan (16x16x32 split GEMMs): 5e-6 on probabilities and logits, same argmax, and
    the load-time guard keeps the fast plan (state 1)"""
    monkeypatch.delenv("TH_WINO_B3VAR", raising=False)
    z, meta = cnn_golden
    m = next(x for x in meta if x["name"] == name)
    cfg, weights = getattr(synth, m["builder"])(**m["kwargs"])
    frames = synth.synthetic_frames(m["n"], **m["frame_kwargs"])
    model = engine.HipFrameModel.from_keras(cfg, weights, device=gpu)
    assert any("k_wino_gemm_b3" in s["label"] for s in model.steps())
    assert model.guard()["state"] == 1, model.guard()
    for chunk in (1024, 3):
        model.set_chunk(chunk)
        probs = model.predict(frames)
        np.testing.assert_allclose(probs, z[f"{name}__torch64"], atol=TIGHT, rtol=0)
        assert np.array_equal(probs.argmax(1), z[f"{name}__torch64"].argmax(1))
        logits = model.predict(frames, logits=True)
        np.testing.assert_allclose(logits, z[f"{name}__logits64"], atol=TIGHT, rtol=0)
    model.close()
