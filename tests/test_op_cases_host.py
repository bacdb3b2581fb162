"""The case table of tests/op_cases.py on the host: the NumPy oracle's branch for every op and activation of the closed set
against an arbiter that is not the oracle (tests/golden/op_set_golden.npz: torch, float64, its own padding and pooling
arithmetic), in float64 and in float32, and the closure of the table over timed_hip/keras_config.py's op and activation codes.

The float32 comparison is the condition that makes the GPU bound of tests/test_gpu_op_set.py meaningful: an engine that computes
in float32 can be held to 5e-6 of the float64 result only where plain float32 arithmetic stays within 2e-6 of it."""
import os
import re

import numpy as np
import pytest

import op_cases
from oracle import cnn_oracle
from timed_hip import keras_config as kc

GOLDEN = op_cases.GOLDEN
FIXTURE_CASES = op_cases.fixture_cases()
IDS = [c.name for c in FIXTURE_CASES]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _tensors(golden, cs, cfg, probes):
    """(layer name, float64 fixture tensor) of the output and of every layer the case names"""
    out = cfg["config"]["output_layers"][0][0]
    return [(out, golden[f"{cs.name}__out"])] + [(p, golden[f"{cs.name}__layer__{p}"]) for p in probes]


@pytest.mark.parametrize("cs", FIXTURE_CASES, ids=IDS)
def test_oracle_float64_matches_torch_float64(golden, cs):
    """1e-12 x max(1, |want|max): tests/test_oracle_cnn.py asserts bounds of this order (1e-14 / 1e-13)"""
    cfg, weights, probes = cs.model()
    vals = cnn_oracle.forward(cfg, weights, cs.frames(), np.float64, return_all=True)
    for name, want in _tensors(golden, cs, cfg, probes):
        got = vals[name]
        assert got.shape == want.shape and got.dtype == np.float64, name
        assert not np.isnan(got).any(), name
        assert float(np.abs(got - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max())), name


@pytest.mark.parametrize("cs", FIXTURE_CASES, ids=IDS)
def test_oracle_float32_stays_within_2e6_of_torch_float64(golden, cs):
    """2e-6 x max(1, |want|max), the bound of test_oracle_cnn.py::test_oracle_matches_torch"""
    cfg, weights, probes = cs.model()
    vals = cnn_oracle.forward(cfg, weights, cs.frames(), np.float32, return_all=True)
    for name, want in _tensors(golden, cs, cfg, probes):
        got = vals[name]
        assert got.shape == want.shape and got.dtype == np.float32, name
        assert float(np.abs(got - want).max()) <= 2e-6 * max(1.0, float(np.abs(want).max())), name


def test_fixture_holds_every_case_and_nothing_else(golden):
    want = set()
    for cs in FIXTURE_CASES:
        cfg, _, probes = cs.model()
        want.add(f"{cs.name}__out")
        want.update(f"{cs.name}__layer__{p}" for p in probes)
    assert set(golden.files) == want
    assert all(golden[k].dtype == np.float64 for k in golden.files)
    assert os.path.getsize(GOLDEN) < 1000000


def test_case_sizes_stay_small():
    """volumes of 2 to 9 voxels per side (one voxel where the row is about the channel count alone), 3 to 11 frames"""
    for cs in FIXTURE_CASES:
        frames = cs.frames()
        assert 3 <= len(frames) <= 11 and frames.shape[1:] == cs.shape, cs.name
        assert max(cs.shape[:3]) <= 9, cs.name
        if cs.group not in (4, 5, 6):
            assert cs.shape[3] <= 24 and min(cs.shape[:3]) >= 2, cs.name
        if cs.make_frames is None:
            assert 0.35 < float((frames == 0).mean()) < 0.65, cs.name


def test_cases_close_over_the_op_and_activation_tables():
    """every op of keras_config.OP_NAMES but the identity, every activation code, and both states of every integer option of
    the pools and of BatchNormalization occur in some case: an op added to the table later without a case fails here"""
    ops, acts, pool_same, bn_gamma, bn_beta, pool_iso, pool_stride_is_size = set(), set(), set(), set(), set(), set(), set()
    bn_rank, eps = set(), set()
    for cs in op_cases.CASES:
        cfg, weights, _ = cs.model()
        for l in kc.parse_keras_model(cfg, weights):
            ops.add(l.op)
            if "act" in l.ip:
                acts.add(l.ip["act"])
            if l.op in (kc.OP_MAXPOOL, kc.OP_AVGPOOL):
                pool_same.add((l.op, l.ip["same"]))
                pool_iso.add((l.op, l.ip["pd"] == l.ip["ph"] == l.ip["pw"]))
                pool_stride_is_size.add((l.op, (l.ip["sd"], l.ip["sh"], l.ip["sw"]) == (l.ip["pd"], l.ip["ph"], l.ip["pw"])))
            if l.op == kc.OP_BN:
                bn_gamma.add("gamma" in l.weights)
                bn_beta.add("beta" in l.weights)
                bn_rank.add(len(l.out_shape))
                eps.add(l.fp["eps"])
    assert ops == set(kc.OP_NAMES) - {kc.OP_IDENTITY}, sorted(set(kc.OP_NAMES) - {kc.OP_IDENTITY} - ops)
    assert acts == set(kc._ACT_BY_NAME.values()), sorted(set(kc._ACT_BY_NAME.values()) - acts)
    both = {(op, v) for op in (kc.OP_MAXPOOL, kc.OP_AVGPOOL) for v in (0, 1)}
    assert pool_same == both and pool_iso == both and pool_stride_is_size == both
    assert bn_gamma == {True, False} and bn_beta == {True, False} and bn_rank == {1, 4} and eps == {1e-3, 1e-5}


def test_every_label_pattern_compiles_and_names_are_unique():
    names = [c.name for c in op_cases.CASES]
    assert len(set(names)) == len(names)
    for cs in op_cases.CASES:
        for pat in (*cs.must, *cs.must_not, *cs.order):
            re.compile(pat)


def test_no_skip_or_expected_failure_in_the_op_set_modules():
    """no name or attribute of either module is one of pytest's ways of not running a test"""
    import ast
    banned = {"skip", "skipif", "xfail", "importorskip"}
    here = os.path.dirname(os.path.abspath(__file__))
    for mod in ("test_op_cases_host.py", "test_gpu_op_set.py"):
        tree = ast.parse(open(os.path.join(here, mod)).read())
        used = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)} | {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)}
        assert not used & banned, (mod, sorted(used & banned))
