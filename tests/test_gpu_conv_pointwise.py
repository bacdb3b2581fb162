"""Every instantiation of the pointwise (1x1x1) convolution kernels, k_conv_pw and k_conv_pw2 (csrc/conv_pointwise_k.h), against the
float64 oracle at shapes a few tiles long, from the case table of tests/pointwise_cases.py (tests/test_conv_pointwise_host.py shows
without a GPU that the table reaches all of them).

  * each row: [prologue] -> Conv3D 1x1x1 -> [epilogue] -> [2x2x2 pool] -> Flatten, 5 frames, every voxel and channel compared;
    volumes (3, 2, 3) (18 voxels: frames straddle the 32-row tiles) and (6, 3, 2) pooled to (3, 1, 1) (the 4-voxel pooled tiles
    straddle frames, the odd H is trimmed);
  * the GEMM core alone against the forward bound of a float32 dot product;
  * TH_PW_RESIDENT=1, one workgroup: each wave walks up to four tiles (k_conv_pw2's register ping-pong, the prefetch of tile
    t + stride, both loop exits), bit for bit against the default grid where every wave takes one tile;
  * chunk-blocked output in front of conv_wfused (every BLK kernel, and k_conv_pw's own blocked stores) bit for bit against the
    channels-last plan (TH_WF_NOBLK=1);
  * channel slices of a concat buffer at offsets and strides that are no multiple of 4 floats.
Every test asks th_conv_pw_pick which kernel its layer runs and finds that name in the step label."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_cases as pc  # noqa: E402
from oracle import cnn_oracle  # noqa: E402
from timed_hip import _lib, engine, synth  # noqa: E402

pytestmark = pytest.mark.gpu

VOL, VOL_POOLED, VOL_BLK = (3, 2, 3), (6, 3, 2), (10, 10, 10)


def _rows(*groups):
    return [pytest.param(c, id=pc.case_id(c)) for c in pc.CASES if c.group in groups]


def _pick(c):
    buf = C.create_string_buffer(64)
    assert _lib.load().th_conv_pw_pick(*pc.pick_args(c), buf, 64) == 0
    assert buf.value, c
    return buf.value.decode()


def _volume(c):
    return VOL_BLK if c.blocked else (VOL if c.pool == "none" else VOL_POOLED)


def _net(c):
    """the net of a row; 'gemm' rows come from pointwise_cases.gemm_operands, whose weights the bound needs"""
    if c.group == "gemm":
        return pc.gemm_operands(c)[:2]
    b = synth.KerasGraphBuilder((*_volume(c), c.cin), seed=1000 + c.cin * 131 + c.cout, bias_std=0.3)
    x = b.input_name
    x = {"none": lambda t: t, "bn_relu": lambda t: b.relu(b.batchnorm(t)), "relu": b.relu, "bn_elu": lambda t: b.elu(b.batchnorm(t)),
         "bn": b.batchnorm}[c.pre](x)
    x = b.conv3d(x, c.cout, 1, padding="same", use_bias=not (c.pre == c.epi == "bn_relu"))       # DenseNet's bottlenecks have no bias
    x = {"none": lambda t: t, "relu": b.relu, "elu_bn": lambda t: b.batchnorm(b.elu(t)), "bn_relu": lambda t: b.relu(b.batchnorm(t)),
         "leaky": lambda t: b.leaky_relu(t, 0.2), "elu": b.elu}[c.epi](x)
    if c.pool != "none":
        x = (b.maxpool if c.pool == "max" else b.avgpool)(x, 2)
    if c.blocked:
        x = b.conv3d(x, 16, 3, padding="same")
    return b.finish(b.flatten(x))


def _frames(n, volume, cin, seed, dense):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, *volume, cin))
    return (x if dense else x * (rng.random(x.shape) < 0.5)).astype(np.float32)


def _case_frames(c, n):
    if c.group == "gemm":
        return pc.gemm_operands(c, n)[2]
    return _frames(n, _volume(c), c.cin, c.cin * 7 + c.cout, c.dense)


def _load(cfg, weights, monkeypatch, **env):
    """a model loaded under the given TH_* knobs (they are read at load), which are unset again afterwards"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = engine.HipFrameModel.from_keras(cfg, weights)
    for k in env:
        monkeypatch.delenv(k)
    assert all(f"{k}={v}" in m.knobs() for k, v in env.items()), m.knobs()
    return m


def _label(m, layer="conv3d"):
    return next(s["label"] for s in m.steps() if s["label"].startswith(layer + ": "))


def _within(got, want):
    """the project's per-element bound (tests/test_gpu_conv_sweep.py), here against the float64 oracle"""
    err, scale = float(np.abs(got - want).max()), max(1.0, float(np.abs(want).max()))
    return got.shape == want.shape and err <= 2e-5 * scale, (err, scale)


@pytest.mark.parametrize("c", _rows("pw2", "epi2", "pw", "gemm"))
def test_every_instantiation_against_the_oracle(gpu, c):
    cfg, weights = _net(c)
    frames = _case_frames(c, 5)
    want = cnn_oracle.forward(cfg, weights, frames, np.float64)
    m = engine.HipFrameModel.from_keras(cfg, weights)
    label = _label(m)
    got = m.predict(frames)
    one = m.predict(frames[2:3])
    m.close()
    assert f"[{_pick(c)}]" in label, label
    ok, figures = _within(got, want)
    assert ok, (figures, label)
    assert np.array_equal(one[0], got[2]), label                     # a frame's result does not depend on its neighbours in the tiles


@pytest.mark.parametrize("c", _rows("gemm"))
def test_gemm_core_within_the_dot_product_bound(gpu, c):
    """No prologue, epilogue or pool: bias + sum over Cin on the fp32 matrix pipe, per element within
    2 (Cin + 2) 2^-24 (sum |x| |w| + |b|) of float64 (pointwise_cases.gemm_bound: any summation order meets it).  Worst
    |got - want64| / bound over the 21 rows: numpy float32 on the CPU 0.213 (3 -> 64), the kernels on the GPU 0.213 as well (3 -> 64; 0.142 at 8 -> 64)."""
    cfg, weights, frames, w, bias = pc.gemm_operands(c)
    want = cnn_oracle.forward(cfg, weights, frames, np.float64)
    m = engine.HipFrameModel.from_keras(cfg, weights)
    label = _label(m)
    got = m.predict(frames)
    m.close()
    assert f"[{_pick(c)}]" in label, label
    ratio = np.abs(got.astype(np.float64) - want).reshape(-1, c.cout) / pc.gemm_bound(c, frames, w, bias)
    print(f"{pc.case_id(c)}: {_pick(c)} / bound = {float(ratio.max()):.4f}")
    assert float(ratio.max()) <= 1.0, (float(ratio.max()), label)


def _multi_trip_rows():
    rows = [c for c in pc.CASES if c.group in ("pw2", "epi2") or (c.group == "gemm" and c.cin % 8 == 0 and c.cin <= 128)]
    for lo, hi in ((1, 32), (33, 64), (65, 128)):                    # k_conv_pw: one row per KMAX and pool
        for pool in pc.POOLS:
            rows.append(next(c for c in pc.CASES if c.group == "pw" and lo <= c.cin <= hi and c.pool == pool))
    return [pytest.param(c, id=pc.case_id(c)) for c in rows]


@pytest.mark.parametrize("c", _multi_trip_rows())
def test_waves_that_walk_several_tiles_compute_what_one_tile_per_wave_computes(gpu, monkeypatch, c):
    """TH_PW_RESIDENT=1: one workgroup, four waves.  Frame counts that give 2, 5, 11 and 14 tiles, the last one ragged, are
    1,1,0,0 / 2,1,1,1 / 3,3,3,2 / 4,4,3,3 trips per wave: the early return, k_conv_pw2's two loop exits and a second turn of its
    loop.  A row's arithmetic does not depend on the schedule: bit-identical to the default grid (one trip per wave)."""
    pooled = c.pool != "none"
    kernel = _pick(c)
    assert kernel.startswith("k_conv_pw<" if c.group == "pw" else "k_conv_pw2<"), kernel
    cfg, weights = _net(c)
    counts = (2, 6, 14, 18) if pooled else (3, 8, 19, 24)
    vol = _volume(c)
    rows = [n * (vol[0] // 2) * (vol[1] // 2) * (vol[2] // 2) * 8 if pooled else n * vol[0] * vol[1] * vol[2] for n in counts]
    assert [(r + 31) // 32 for r in rows] == [2, 5, 11, 14] and all(r % 32 for r in rows), rows
    frames = _case_frames(c, counts[-1])
    want = cnn_oracle.forward(cfg, weights, frames, np.float64)
    one = _load(cfg, weights, monkeypatch, TH_PW_RESIDENT="1")
    ref = engine.HipFrameModel.from_keras(cfg, weights)
    assert "TH_PW_RESIDENT" not in ref.knobs() and f"[{kernel}]" in _label(one) and _label(one) == _label(ref)
    for n in counts:
        got = one.predict(frames[:n])
        assert np.array_equal(got, ref.predict(frames[:n])), (n, kernel)
    one.close()
    ref.close()
    ok, figures = _within(got, want)
    assert ok, (figures, kernel)


@pytest.mark.parametrize("c", _rows("blk"))
def test_chunk_blocked_output_of_every_kernel_that_writes_it(gpu, monkeypatch, c):
    """[prologue] -> Conv 1x1x1 -> [epilogue] -> Conv 3x3x3 'same' on 10^3: the tensor between the two is stored [C/4][voxel][4].
    k_conv_pw2's BLK kernels transpose each 32 x 32 tile through LDS; k_conv_pw (96 -> 128: no k_conv_pw2<16,4>; 30 -> 20:
    Cin % 8 != 0) stores element by element.  3 frames = 3000 rows, 94 tiles, a ragged last one.  No arithmetic changes with the
    layout or with the grid: bit-identical to the channels-last plan and to one workgroup walking all 94 tiles."""
    cfg, weights = _net(c)
    frames = _case_frames(c, 3)
    want = cnn_oracle.forward(cfg, weights, frames, np.float64)
    m = engine.HipFrameModel.from_keras(cfg, weights)
    labels = [s["label"] for s in m.steps()]
    got = m.predict(frames)
    m.close()
    assert sum("output chunk-blocked" in l for l in labels) == 1 and sum("input chunk-blocked" in l for l in labels) == 1, labels
    assert any(f"[{_pick(c)}]" in l and "output chunk-blocked" in l and l.startswith("conv3d: ") for l in labels), labels
    ok, figures = _within(got, want)
    assert ok, (figures, labels)
    m = _load(cfg, weights, monkeypatch, TH_WF_NOBLK="1")
    assert not any("chunk-blocked" in s["label"] for s in m.steps())
    assert np.array_equal(m.predict(frames), got)
    m.close()
    m = _load(cfg, weights, monkeypatch, TH_PW_RESIDENT="1")         # 23 or 24 trips per wave
    assert f"[{_pick(c)}]" in _label(m)
    assert np.array_equal(m.predict(frames), got)
    m.close()


@pytest.mark.parametrize("pool", ["none", "max"])
def test_misaligned_and_offset_views_of_a_concat_buffer(gpu, pool):
    """Two pointwise layers write channels 0..17 and 18..33 of one 34-channel buffer (the second at an output offset that is no
    multiple of 4: k_conv_pw2's 4-byte stores).  One bottleneck reads the 16-channel slice at offset 18 (Cin % 8 == 0, but the
    view is not 16-byte aligned: k_conv_pw, scalar loads of full vectors, and the label says so), one reads all 34 channels
    (Cin % 4 != 0).  The layers are the 'view' rows of the case table."""
    vol = VOL if pool == "none" else VOL_POOLED
    b = synth.KerasGraphBuilder((*vol, 8), seed=34 + len(pool), bias_std=0.3)
    p = b.conv3d(b.input_name, 18, 1, padding="same")
    q = b.conv3d(b.input_name, 16, 1, padding="same")
    cat = b.concat([p, q])
    z = b.conv3d(b.relu(b.batchnorm(q)), 40, 1, padding="same")
    t = b.conv3d(b.relu(b.batchnorm(cat)), 24, 1, padding="same", use_bias=False)
    # a second reader of the buffer keeps it a tensor of its own (the front end pushes BN -> ReLU through a concat that only they read)
    if pool == "max":
        z, t, u = b.maxpool(z, 2), b.maxpool(t, 2), b.maxpool(cat, 2)
    else:
        u = b.elu(cat)
    cfg, weights = b.finish(b.flatten(b.concat([z, t, u])))
    frames = _frames(5, vol, 8, 18, pool == "max")
    want = cnn_oracle.forward(cfg, weights, frames, np.float64)
    m = engine.HipFrameModel.from_keras(cfg, weights)
    labels = [s["label"] for s in m.steps()]
    got = m.predict(frames)
    m.close()
    assert not any("concat(copy" in l for l in labels), labels                     # the slices live in the concat buffer
    view = [c for c in pc.CASES if c.group == "view"]
    rows = view[:4] if pool == "none" else view[4:]
    assert [(c.cin, c.cout, c.pool) for c in rows] == [(8, 18, "none"), (8, 16, "none"), (16, 40, pool), (34, 24, pool)]
    for layer, c in zip(("conv3d", "conv3d_1", "conv3d_2", "conv3d_3"), rows):
        label = next(l for l in labels if l.startswith(layer + ": "))
        assert f"[{_pick(c)}]" in label, (layer, _pick(c), label)
    assert "[k_conv_pw<4,2," in next(l for l in labels if l.startswith("conv3d_2: ")), labels      # not k_conv_pw2
    assert "[k_conv_pw2<4,1,0,0,0>]" in next(l for l in labels if l.startswith("conv3d_1: ")), labels
    ok, figures = _within(got, want)
    assert ok, (figures, labels)
