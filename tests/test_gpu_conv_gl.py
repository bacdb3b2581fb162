"""Strided and small-volume convolutions as an implicit GEMM with rows across the batch and operands straight from L2
(csrc/conv_gl.hip, v_mfma_f32_16x16x4_f32) against the CPU oracle and the kernels it replaces (TH_CONV_GL=0): stride 2 'same'
(Keras puts the odd padding row behind), 'valid', anisotropic kernels and strides, dilation, 1 .. 128 output channels, row tiles
that straddle frames and a batch whose last tile is ragged, fused bias / activation / BatchNorm.  Serves reference predict.py:142
(ProDCoNN's strided layer and the 'valid' one behind it).
Launches of at least 262 113 rows run two row tiles per wave (conv_gl_row_tiles; ProDCoNN's strided layer at chunk 4096 does):
test_conv_gl_two_row_tiles runs every column-tile count with and without the input prologue at 270 000 .. 351 000 rows in one launch,
each row count with another ragged end, and holds the two-tile kernels bit for bit to the one-tile kernels on the same frames, and
three frames of each to the float64 oracle.  The batch sizes come from th_conv_gl_row_tiles, which the tests call and do not copy."""
import numpy as np
import pytest

from oracle import cnn_oracle
from timed_hip import _lib, engine, synth

pytestmark = pytest.mark.gpu


def _run(cfg, w, x, chunk=None):
    m = engine.HipFrameModel.from_keras(cfg, w)
    if chunk:
        m.set_chunk(chunk)
    got = m.predict(x)
    labels = [s["label"] for s in m.steps()]
    m.close()
    return got, labels


def _net(shape, build, seed):
    b = synth.KerasGraphBuilder(shape, seed=seed, bias_std=0.3)
    return b.finish(b.flatten(build(b, b.input_name)))


# (input shape, conv kwargs, chain, frames)
CASES = [
    ((10, 10, 10, 32), dict(filters=48, kernel_size=3, strides=2, padding="same"), "elu", 7),        # ProDCoNN conv3d_2
    ((5, 5, 5, 48), dict(filters=64, kernel_size=3, padding="valid"), "leaky", 9),                     # ProDCoNN conv3d_3: 27 rows per frame
    ((7, 6, 5, 16), dict(filters=1, kernel_size=(1, 3, 5), strides=(1, 2, 2), padding="same"), "none", 5),
    ((9, 9, 9, 16), dict(filters=100, kernel_size=3, strides=3, padding="valid"), "relu_bn", 3),
    ((8, 8, 8, 32), dict(filters=128, kernel_size=2, strides=2, padding="same"), "tanh", 4),
    ((6, 6, 6, 64), dict(filters=20, kernel_size=3, dilation_rate=2, strides=1, padding="same"), "none", 2),
]


def _build(kw, chain):
    def build(b, x):
        kw2 = dict(kw)
        filters, k = kw2.pop("filters"), kw2.pop("kernel_size")
        x = b.conv3d(x, filters, k, activation="relu" if chain == "relu_bn" else None, **kw2)
        if chain == "relu_bn":
            x = b.batchnorm(x)
        elif chain == "elu":
            x = b.activation(x, "elu")
        elif chain == "tanh":
            x = b.activation(x, "tanh")
        elif chain == "leaky":
            x = b.leaky_relu(x, 0.1)
        return x
    return build


@pytest.mark.parametrize("shape,kw,chain,n", CASES)
def test_conv_gl_per_element(gpu, monkeypatch, shape, kw, chain, n):
    monkeypatch.setenv("TH_CONV_GL", "2")                               # every eligible layer (the default takes strided / <= 64-output ones)
    cfg, w = _net(shape, _build(kw, chain), seed=sum(shape) + kw["filters"])
    x = np.random.default_rng(n).standard_normal((n, *shape)).astype(np.float32)
    want = cnn_oracle.forward(cfg, w, x, np.float64)
    got, labels = _run(cfg, w, x)
    assert any("k_conv_gl" in l for l in labels), labels
    scale = max(1.0, float(np.abs(want).max()))
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= 5e-6 * scale
    got2, _ = _run(cfg, w, x, chunk=2)                                  # other tiles over the same rows: bit-identical
    assert np.array_equal(got, got2)
    monkeypatch.setenv("TH_CONV_GL", "0")
    ref, rl = _run(cfg, w, x)
    assert not any("k_conv_gl" in l for l in rl), rl
    assert float(np.abs(got - ref).max()) <= 3e-6 * scale
    assert float(np.abs(got - want).max()) <= 1.5 * float(np.abs(ref - want).max()) + 2e-7 * scale


@pytest.mark.parametrize("act", ["relu", "elu", None])
def test_conv_gl_input_prologue(gpu, monkeypatch, act):
    """BN -> activation in FRONT of the convolution (DenseCPD's growth layers; here on the model input, where no producer can absorb
    it): applied to the loaded voxels in registers, and the 'same' padding pads the ACTIVATED tensor — zeros, not act(shift)"""
    monkeypatch.setenv("TH_CONV_GL", "2")

    def build(b, x):
        x = b.batchnorm(x)
        if act:
            x = b.activation(x, act)
        return b.conv3d(x, 24, 3, strides=2, padding="same")

    cfg, w = _net((6, 5, 4, 32), build, seed=12)
    x = np.random.default_rng(3).standard_normal((5, 6, 5, 4, 32)).astype(np.float32)
    want = cnn_oracle.forward(cfg, w, x, np.float64)
    got, labels = _run(cfg, w, x)
    assert any("k_conv_gl" in l for l in labels), labels
    assert float(np.abs(got - want).max()) <= 5e-6 * max(1.0, float(np.abs(want).max()))
    monkeypatch.setenv("TH_CONV_GL", "0")
    ref, _ = _run(cfg, w, x)
    assert float(np.abs(got - ref).max()) <= 3e-6 * max(1.0, float(np.abs(ref).max()))


def _row_tiles(rows):
    return int(_lib.load().th_conv_gl_row_tiles(rows))


# The two-row-tile kernels, k_conv_gl<NT, PRE, 2>: launches of at least 262 113 rows, which only a large chunk reaches (ProDCoNN's
# conv3d_2 at chunk 4096).  Here ten to thirteen frames of a 30^3 output volume in ONE launch (set_chunk(n)): 27 000 rows per frame,
# 27 000 mod 32 = 24, so every frame boundary falls inside a wave and often between its two tiles.  Kernel (2, 3, 2), 'same': padding
# on every axis, the extra row of the even axes behind; 12 taps go round the three-block ring more than once.
#   n = 10: 270 000 rows, 16 past the last full wave: that wave's second tile lies wholly past the end, and of the 8 438 waves the
#           last workgroup holds two that return at once      n = 11: 297 000, 8 left over: first tile ragged, second empty
#   n = 12: 324 000, no ragged end                            n = 13: 351 000, 24 left over: second tile ragged
# (id, input shape, conv kwargs, chain behind, what stands in front, frames, TH_CONV_GL, column tiles NT)
_K232 = dict(kernel_size=(2, 3, 2), strides=1, padding="same")
MT2_CASES = [
    ("nt1", (30, 30, 30, 16), dict(filters=7, **_K232), "none", None, 10, "2", 1),            # partial column tile
    ("nt2_elu", (30, 30, 30, 32), dict(filters=24, **_K232), "elu", None, 11, "2", 2),        # two channel blocks per tap
    ("nt3_relu_bn", (30, 30, 30, 16), dict(filters=33, **_K232), "relu_bn", None, 13, "2", 3),    # one real column in the last tile
    ("nt4_leaky", (30, 30, 30, 16), dict(filters=64, **_K232), "leaky", None, 12, "2", 4),
    ("nt6_tanh", (30, 30, 30, 16), dict(filters=80, **_K232), "tanh", None, 10, "2", 6),      # five tiles rounded up to six: a zero tile
    ("nt8_relu_bn", (30, 30, 30, 32), dict(filters=128, **_K232), "relu_bn", None, 11, "2", 8),
    ("pre_bn_relu_nt2", (30, 30, 30, 16), dict(filters=24, **_K232), "none", "relu", 10, "2", 2),     # PRE = true: padding voxels and
    ("pre_bn_elu_nt8", (30, 30, 30, 16), dict(filters=128, **_K232), "none", "elu", 13, "2", 8),      # rows past the end stay zero in
    ("pre_bn_nt3", (30, 30, 30, 16), dict(filters=48, **_K232), "none", "bn", 11, "2", 3),            # both tiles, not act(shift)
    # ProDCoNN's conv3d_2 on its own geometry, chosen by the default rule (TH_CONV_GL unset: the layer is strided)
    ("strided_default", (60, 60, 60, 16), dict(filters=48, kernel_size=3, strides=2, padding="same"), "elu", None, 10, None, 3),
]


@pytest.mark.parametrize("shape,kw,chain,pre,n,knob,nt", [c[1:] for c in MT2_CASES], ids=[c[0] for c in MT2_CASES])
def test_conv_gl_two_row_tiles(gpu, monkeypatch, shape, kw, chain, pre, n, knob, nt):
    """k_conv_gl<NT, PRE, 2> against k_conv_gl<NT, PRE, 1> bit for bit (a row's K order does not depend on the row tiles per wave, so
    no tolerance applies) and against the float64 oracle on the first, a middle and the last frame: the first wave, interior frame
    boundaries, the ragged end.  th_conv_gl_row_tiles is asked, not copied: a moved threshold fails here and does not turn this
    into a second one-tile test."""
    if knob is None:
        monkeypatch.delenv("TH_CONV_GL", raising=False)
    else:
        monkeypatch.setenv("TH_CONV_GL", knob)

    def build(b, x):
        if pre:
            x = b.batchnorm(x)
            if pre != "bn":
                x = b.activation(x, pre)
        return _build(kw, chain)(b, x)

    cfg, w = _net(shape, build, seed=100 * nt + n)
    Vo = int(np.prod([-(-s // kw["strides"]) for s in shape[:3]]))    # 'same': ceil(extent / stride) per axis
    assert Vo == 27000
    assert _row_tiles(n * Vo) == 2 and _row_tiles(2 * Vo) == 1 and _row_tiles(Vo) == 1
    x = np.random.default_rng(n).standard_normal((n, *shape)).astype(np.float32)
    got, labels = _run(cfg, w, x, chunk=n)                              # the whole batch in one launch
    gl = [l for l in labels if "k_conv_gl" in l]
    assert len(gl) == 1 and f"conv_gl<{nt} column tiles>" in gl[0], labels
    assert got.shape == (n, Vo * kw["filters"]) and np.isfinite(got).all()
    one, labels1 = _run(cfg, w, x, chunk=2)                             # 54 000 rows per launch (27 000 in the last of an odd n): one tile
    assert any("k_conv_gl" in l for l in labels1), labels1
    assert np.array_equal(got, one), (f"two row tiles differ from one in frames {np.flatnonzero((got != one).any(axis=1)).tolist()}, "
                                      f"max {float(np.abs(got - one).max()):.3e}")
    sel = [0, n // 2, n - 1]
    want = cnn_oracle.forward(cfg, w, x[sel], np.float64)
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got[sel] - want).max())
    assert want.shape == got[sel].shape and err <= 5e-6 * scale, (err, scale)
    if knob is None:                                                    # once: the kernel the layer had before (test_conv_gl_per_element's bounds)
        monkeypatch.setenv("TH_CONV_GL", "0")
        ref, rl = _run(cfg, w, x[sel])
        assert not any("k_conv_gl" in l for l in rl), rl
        assert float(np.abs(got[sel] - ref).max()) <= 3e-6 * scale
        assert err <= 1.5 * float(np.abs(ref - want).max()) + 2e-7 * scale


def test_default_rule_and_layers_it_leaves_alone(gpu):
    """by default: strided layers and those with at most 64 outputs per frame; a stride-1 'same' layer on 10^3 keeps its kernel, and
    so does one whose Cin is not a multiple of 16"""
    cfg, w = synth.prodconn_synth(20, seed=3)
    m = engine.HipFrameModel.from_keras(cfg, w)
    labels = [s["label"] for s in m.steps()]
    m.close()
    assert sum("k_conv_gl" in l for l in labels) == 2, labels           # conv3d_2 (stride 2) and conv3d_3 (27 outputs per frame)
    for shape, kw in (((10, 10, 10, 32), dict(filters=48, kernel_size=3, padding="same")),
                      ((6, 6, 6, 20), dict(filters=16, kernel_size=3, strides=2, padding="same"))):
        cfg, w = _net(shape, _build(kw, "none"), seed=1)
        x = np.random.default_rng(0).standard_normal((3, *shape)).astype(np.float32)
        got, labels = _run(cfg, w, x)
        assert not any("k_conv_gl" in l for l in labels), labels
        want = cnn_oracle.forward(cfg, w, x, np.float64)
        assert float(np.abs(got - want).max()) <= 2e-5 * max(1.0, float(np.abs(want).max()))


def test_conv_gl_random_geometries(gpu, monkeypatch):
    """thirty seeded draws of (extent, kernel, stride, dilation, padding, Cin in {16, 32, 48}, 1..128 filters, 1..9 frames): every one
    within 5e-6 x scale of the float64 oracle, on the kernel whenever the layer is eligible"""
    monkeypatch.setenv("TH_CONV_GL", "2")
    rng = np.random.default_rng(2024)
    ran = 0
    for case in range(30):
        shape = tuple(int(v) for v in rng.integers(3, 10, 3))
        k = tuple(int(v) for v in rng.integers(1, 5, 3))
        st = tuple(int(v) for v in rng.integers(1, 4, 3))
        dl = tuple(int(v) for v in rng.integers(1, 3, 3)) if case % 3 == 0 else (1, 1, 1)
        if any(d > 1 for d in dl):
            st = (1, 1, 1)                                              # Keras: strides and dilation do not combine
        padding = "same" if case % 2 else "valid"
        if padding == "valid" and any((kk - 1) * dd + 1 > n for kk, dd, n in zip(k, dl, shape)):
            padding = "same"
        cin, cout, n = int(rng.choice([16, 32, 48])), int(rng.integers(1, 129)), int(rng.integers(1, 10))
        kw = dict(filters=cout, kernel_size=k, strides=st, dilation_rate=dl, padding=padding)
        cfg, w = _net((*shape, cin), _build(kw, ("none", "elu", "relu_bn")[case % 3]), seed=case)
        x = rng.standard_normal((n, *shape, cin)).astype(np.float32)
        want = cnn_oracle.forward(cfg, w, x, np.float64)
        got, labels = _run(cfg, w, x)
        ran += any("k_conv_gl" in l for l in labels)
        assert got.shape == want.shape, (case, kw, shape)
        assert float(np.abs(got - want).max()) <= 5e-6 * max(1.0, float(np.abs(want).max())), (case, kw, shape, cin, n, labels)
    assert ran >= 20, ran
