"""The closed Keras op set on the GPU: every op and activation of timed_hip/keras_config.py, run and checked.

Groups 1 to 9 of tests/op_cases.py against tests/golden/op_set_golden.npz (torch, float64; tests/golden/make_op_set_golden.py), under
four plans: the default plan, TH_LOAD_NO_MFMA, TH_LOAD_NO_FUSE | TH_LOAD_NO_MFMA (the generic kernels of csrc/kernels_generic.hip
alone) and TH_LOAD_KEEP_ALL.  The output and every layer a case names are within TIGHT = 5e-6 x max(1, |want|max) of the float64
fixture (the bound tests/test_gpu_cnn.py asserts against float64; tests/test_op_cases_host.py shows plain float32 arithmetic
stays within 2e-6 of it on these cases).  Layer by layer: an error in one op is not washed out by a later softmax.
"""
import re

import numpy as np
import pytest

import op_cases
from oracle import cnn_oracle
from timed_hip import _lib, engine

pytestmark = pytest.mark.gpu
TIGHT = 5e-6
PLANS = {"default": 0, "no_mfma": _lib.TH_LOAD_NO_MFMA, "generic": _lib.TH_LOAD_NO_FUSE | _lib.TH_LOAD_NO_MFMA,
         "keep_all": _lib.TH_LOAD_KEEP_ALL}
FUSED_TAIL = r"k_gap_softmax|k_tail_dense"
GOLDEN = op_cases.GOLDEN
FIXTURE_CASES = op_cases.fixture_cases()
IDS = [c.name for c in FIXTURE_CASES]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _close(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert not np.isnan(got).any(), what
    err, scale = float(np.abs(got - want).max()), max(1.0, float(np.abs(want).max()))
    print(f"{what}: max|d| {err:.3e} scale {scale:.3g}")
    assert err <= TIGHT * scale, (what, err, scale)


def _in_order(labels, patterns):
    """every pattern matches a step label, each in a later step than the one before"""
    at = -1
    for pat in patterns:
        at = next((j for j in range(at + 1, len(labels)) if re.search(pat, labels[j])), None)
        assert at is not None, (pat, labels)


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("cs", FIXTURE_CASES, ids=IDS)
def test_case_matches_the_float64_fixture_layer_by_layer(gpu, golden, cs, plan):
    cfg, weights, probes = cs.model()
    frames = cs.frames()
    m = engine.HipFrameModel.from_keras(cfg, weights, device=gpu, flags=PLANS[plan])
    labels = [s["label"] for s in m.steps()]
    print(plan, labels)
    got = m.predict(frames)
    want = golden[f"{cs.name}__out"]
    _close(got, want, f"{cs.name} output")
    if cs.group == 5:
        # the rows with 1e4 and -1e30: where float64 gives exactly 0 or exactly 1, so does float32
        exact = (want == 0.0) | (want == 1.0)
        assert exact[0].all() or cs.shape[-1] == 1
        assert np.array_equal(got[exact], want[exact].astype(np.float32))
    for pn in probes:
        lw = golden[f"{cs.name}__layer__{pn}"]
        try:
            lg = m.fetch(pn, len(frames), lw.shape[1:])
        except _lib.TimedHipError as e:
            # a fused plan does not hold every tensor; the plan that keeps all of them does
            assert "fused away" in str(e) and plan != "keep_all", (pn, str(e))
            continue
        _close(lg, lw, f"{cs.name} {pn}")
    if plan == "default":
        for pat in cs.must:
            assert any(re.search(pat, l) for l in labels), (pat, labels)
        for pat in cs.must_not:
            assert not any(re.search(pat, l) for l in labels), (pat, labels)
        _in_order(labels, cs.order)
    m.close()


@pytest.mark.parametrize("cs", FIXTURE_CASES, ids=IDS)
def test_ragged_chunks_give_the_same_bits(gpu, cs):
    """3 to 11 frames in chunks of 2: a ragged last chunk, the same bits as in one pass"""
    cfg, weights, _ = cs.model()
    frames = cs.frames()
    m = engine.HipFrameModel.from_keras(cfg, weights, device=gpu)
    whole = m.predict(frames)
    m.set_chunk(2)
    assert np.array_equal(m.predict(frames), whole)
    m.close()


@pytest.mark.parametrize("cs", [c for c in FIXTURE_CASES if c.tail], ids=[c.name for c in FIXTURE_CASES if c.tail])
def test_fused_tails_equal_the_separate_kernels_bit_for_bit(gpu, monkeypatch, cs):
    """groups 4 to 6: where k_gap_softmax or k_tail_dense is taken, probabilities and logits equal the TH_NO_TAIL_FUSE=1 run bit for bit
    (what tests/test_gpu_cnn.py promises for the two benchmark tails)"""
    cfg, weights, _ = cs.model()
    frames = cs.frames()
    fused = engine.HipFrameModel.from_keras(cfg, weights, device=gpu)
    assert any(re.search(FUSED_TAIL, s["label"]) for s in fused.steps()), [s["label"] for s in fused.steps()]
    monkeypatch.setenv("TH_NO_TAIL_FUSE", "1")
    plain = engine.HipFrameModel.from_keras(cfg, weights, device=gpu)
    assert not any(re.search(FUSED_TAIL, s["label"]) for s in plain.steps()), [s["label"] for s in plain.steps()]
    for n in (1, len(frames)):
        assert np.array_equal(fused.predict(frames[:n]), plain.predict(frames[:n]))
        assert np.array_equal(fused.predict(frames[:n], logits=True), plain.predict(frames[:n], logits=True))
    fused.close(); plain.close()


@pytest.mark.parametrize("plan", ["default", "generic"])
@pytest.mark.parametrize("cs", [c for c in FIXTURE_CASES if c.group == 9], ids=[c.name for c in FIXTURE_CASES if c.group == 9])
def test_input_dtypes_into_a_first_node_that_is_no_convolution(gpu, cs, plan):
    """k_convert_frames: float64, uint8, bool and float16 frames of 0 / 1 voxels give the bytes of the float32 run"""
    cfg, weights, _ = cs.model()
    frames = cs.frames()
    m = engine.HipFrameModel.from_keras(cfg, weights, device=gpu, flags=PLANS[plan])
    base = m.predict(frames)
    for dt in op_cases.INPUT_DTYPES:
        assert np.array_equal(frames.astype(dt).astype(np.float32), frames), dt
        assert m.predict(frames.astype(dt)).tobytes() == base.tobytes(), dt
    m.close()


def _family_run(gpu, monkeypatch, cs, knobs):
    """the case under its own knobs plus `knobs`: (output, step labels)"""
    flags = 0
    for k, v in {**(cs.env or {}), **(knobs or {})}.items():
        if k == "flags":
            flags = v
        else:
            monkeypatch.setenv(k, v)
    cfg, weights, _ = cs.model()
    m = engine.HipFrameModel.from_keras(cfg, weights, device=gpu, flags=flags)
    labels = [s["label"] for s in m.steps()]
    got = m.predict(cs.frames())
    m.close()
    for k in {**(cs.env or {}), **(knobs or {})}:
        if k != "flags":
            monkeypatch.delenv(k)
    return got, labels


@pytest.mark.parametrize("cs", op_cases.family_cases(), ids=[c.name for c in op_cases.family_cases()])
def test_every_fused_family_runs_sigmoid_elu_and_a_prologue(gpu, monkeypatch, cs):
    """group 10: sigmoid and elu(alpha=0.7) as epilogues, BN -> sigmoid as a prologue and elu(alpha=-0.5) in front of a fused max pool, once
    per fused kernel family at the family's smallest selecting shape; the plan label names the kernel.  Against the oracle in float64 at
    the bound the family's own test file asserts (op_cases.FAMILIES names file and bound), and against the run with the family switched off
    at the bound that file uses between the two.  Where a family's file has no bound between two plans (k_conv_pw, k_conv_pw2; conv_wino for a
    layer's tensor) it is 2e-5 x scale, the bound of tests/test_gpu_conv_sweep.py."""
    cfg, weights, _ = cs.model()
    want = cnn_oracle.forward(cfg, weights, cs.frames(), np.float64)
    scale = max(1.0, float(np.abs(want).max()))
    got, labels = _family_run(gpu, monkeypatch, cs, None)
    print(labels)
    for pat in cs.must:
        assert any(re.search(pat, l) for l in labels), (pat, labels)
    for pat in cs.must_not:
        assert not any(re.search(pat, l) for l in labels), (pat, labels)
    err = float(np.abs(got - want).max())
    print(f"{cs.name}: max|d| {err:.3e} scale {scale:.3g}")
    assert got.shape == want.shape and err <= cs.bound * scale, (err, scale)
    if cs.off is not None:
        ref, rl = _family_run(gpu, monkeypatch, cs, cs.off)
        for pat in cs.must:
            assert not any(re.search(pat, l) for l in rl), (pat, rl)
        d = float(np.abs(got - ref).max())
        print(f"{cs.name}: against the run with {cs.off}: {d:.3e}")
        assert float(np.abs(ref - want).max()) <= cs.bound * scale
        assert d <= cs.between * scale, (d, scale)
    if cs.pool_first:
        ref, rl = _family_run(gpu, monkeypatch, cs, {"TH_NO_POOL_FIRST": "1"})
        if cs.pool_first_bound == 0.0:
            assert np.array_equal(got, ref)          # the rewrite must not have been applied
        else:                                        # the knob takes the kernel itself away: two kernels, the bound between them
            assert not any(re.search(pat, l) for pat in cs.must for l in rl), rl
            assert float(np.abs(got - ref).max()) <= cs.pool_first_bound * scale
