"""Every instantiation of the two brick kernels, k_conv_mfma and k_conv_n16, and every staging mode that only their plan arithmetic
selects, on the GPU: the rows of tests/brick_cases.py (tests/test_conv_brick_host.py shows without a GPU that they reach all 48
kernels, z-bricks with ragged, pooled and strided bricks, 16 frames per workgroup, ragged Cin chunks, geo_compact, ...).  Per row:
  * the step that ran carries the label th_conv_brick_pick gives the row: what was planned is what ran;
  * every voxel and channel against the float64 oracle, max|got - want| <= 2e-5 max(1, max|want|), the bound of
    tests/test_gpu_conv_sweep.py (fp32 MFMA is an fmaf chain: accumulation-order rounding only);
  * the same values with set_chunk(c), c < FB and no divisor of n (frames share workgroups differently), and for the first frame
    run alone.  Values, not bytes: the z-major tap skip drops fmaf(0, w, acc) terms depending on how frames share an m-tile, which
    can turn a -0 into +0 and nothing else;
  * within the same bound of the TH_LOAD_NO_MFMA plan (the direct kernel), which tells a wrong brick kernel from a wrong net."""
import os
import sys

import numpy as np
import pytest

from oracle import cnn_oracle
from timed_hip import _lib, engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brick_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu


def _ran(labels, layer):
    """the plan label of `layer`'s step, without the layer's name and without the remark on why no minimal-filtering form took a
    3x3x3 layer, which the planner puts in front of the last bracket"""
    label = next(l for l in labels if l.startswith(layer + ": "))[len(layer) + 2:]
    k = label.rfind(" [")
    head, note = label[:k], label[:k].find(" (direct form: ")
    return (head[:note] if note >= 0 else head) + label[k:]


@pytest.mark.parametrize("r", bc.ROWS, ids=bc.row_id)
def test_brick_row(gpu, lib, monkeypatch, r):
    for k, v in r.env.items():
        monkeypatch.setenv(k, v)
    i = bc.ROWS.index(r)
    cfg, weights, layer = bc.build(r, seed=500 + i)
    frames = bc.frames(r, seed=900 + i)
    want = cnn_oracle.forward(cfg, weights, frames, np.float64)
    scale = max(1.0, float(np.abs(want).max()))

    m = engine.HipFrameModel.from_keras(cfg, weights)
    labels = [s["label"] for s in m.steps()]
    picked = bc.pick(lib, r)
    assert picked and _ran(labels, layer) == picked, (picked, labels)
    got = m.predict(frames)
    alone = m.predict(frames[:1])
    c = bc.chunk_for(r.FB, r.n)
    m.set_chunk(c)
    chunked = m.predict(frames)
    m.close()
    err = float(np.abs(got - want).max())
    print(f"{r.id}: {picked}: max|got - want| {err:.3e} = {err / scale:.2e} of the scale {scale:.3f}; chunk {c} of n {r.n}")
    assert got.shape == want.shape and err <= 2e-5 * scale, (err, scale, picked)
    assert np.array_equal(chunked, got), (c, float(np.abs(chunked - got).max()))
    assert np.array_equal(alone[0], got[0]), float(np.abs(alone[0] - got[0]).max())

    m = engine.HipFrameModel.from_keras(cfg, weights, flags=_lib.TH_LOAD_NO_MFMA)
    direct = m.predict(frames)
    m.close()
    assert float(np.abs(direct - want).max()) <= 2e-5 * scale                       # the net and the oracle agree without the brick kernel
    assert float(np.abs(got - direct).max()) <= 2e-5 * scale
