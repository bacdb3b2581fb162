"""One case table for the closed Keras op set (timed_hip/keras_config.py: thirteen ops, seven activations), usable on the host.

Every row is a small Keras graph over ``synth.KerasGraphBuilder`` with seeded frames, the names of the layers whose tensors
are compared one by one (an error in one op must not be washed out by a later softmax), and the plan labels that must or must
not appear in the engine's default plan (regular expressions, searched in each step label).

Groups 1 to 9 are evaluated in float64 by tests/golden/make_op_set_golden.py (torch; it shares no padding or pooling
arithmetic with oracle/cnn_oracle.py) into tests/golden/op_set_golden.npz; tests/test_op_cases_host.py holds the oracle to that
fixture and tests/test_gpu_op_set.py the engine.  Group 10 (one sigmoid, one elu(0.7) and one prologue row per fused kernel
family) is compared with the oracle in float64.

Sizes: volumes of 2 to 9 voxels per side, 1 to 24 channels unless a row is about a channel count, 3 to 11 frames (a ragged last
frame group occurs), random inputs with about half their entries zero (tests/test_gpu_conv_sweep.py ``_frames``), inputs to
activations of both signs with |x| up to about 8.
"""
from __future__ import annotations

import itertools
import os
import sys
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "timed-design_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from timed_hip import synth  # noqa: E402


class Builder(synth.KerasGraphBuilder):
    """KerasGraphBuilder plus what the op set allows and the benchmark topologies never needed: anisotropic pools, a ReLU with
    a negative slope, and a list of the layers a case wants compared (``keep``)."""

    def __init__(self, input_shape, seed, bias_std=0.3):
        super().__init__(input_shape, seed=seed, bias_std=bias_std, name="op_case")
        self.probes: List[str] = []

    def keep(self, x: str) -> str:
        if x not in self.probes:
            self.probes.append(x)
        return x

    def pool(self, kind, x, size, strides=None, padding="valid"):
        d, h, w, c = self.shapes[x]
        p = (size,) * 3 if isinstance(size, int) else tuple(size)
        s = p if strides is None else (strides,) * 3 if isinstance(strides, int) else tuple(strides)
        same = padding == "same"
        shape = tuple(self._out(n, pk, sk, same) for n, pk, sk in zip((d, h, w), p, s)) + (c,)
        cls, base = {"max": ("MaxPooling3D", "max_pooling3d"), "avg": ("AveragePooling3D", "average_pooling3d")}[kind]
        return self._emit(cls, base, dict(pool_size=list(p), strides=list(s), padding=padding, data_format="channels_last"), [x], shape)

    def relu_slope(self, x, negative_slope):
        return self._emit("ReLU", "re_lu", dict(max_value=None, negative_slope=negative_slope, threshold=0.0), [x], self.shapes[x])

    def negate_gamma(self, bn: str, every: int = 3):
        """negative gammas on some channels of a BatchNormalization built with scale=True"""
        g = self.weights[bn][0].copy()
        g[::every] *= -1.0
        self.weights[bn] = [g] + list(self.weights[bn][1:])


def half_zero_frames(n, shape, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, *shape)) * scale * (rng.random((n, *shape)) < 0.5)).astype(np.float32)


def binary_frames(n, shape, seed):
    """0 / 1 voxels: exact in float32, float64, uint8, bool and float16"""
    return (np.random.default_rng(seed).random((n, *shape)) < 0.4).astype(np.float32)


@dataclass
class Case:
    name: str
    group: int
    shape: Tuple[int, int, int, int]
    build: Callable[[Builder], str]
    n: int = 5
    seed: int = 0
    scale: float = 1.0
    make_frames: Optional[Callable[["Case"], np.ndarray]] = None
    must: Tuple[str, ...] = ()            # each pattern is found in some step label of the default plan
    must_not: Tuple[str, ...] = ()        # no step label of the default plan matches
    order: Tuple[str, ...] = ()           # patterns found in this order, in different steps
    tail: bool = False                    # a fused tail is taken: bit-identical to the TH_NO_TAIL_FUSE=1 run
    # group 10 only
    env: Optional[dict] = None            # knobs the family's own test file sets to select it
    bound: float = 0.0                    # x max(1, |want|max), against the float64 oracle: what the family's own test file asserts
    off: Optional[dict] = None            # knobs that switch the family off ({"flags": ...}: load flags instead)
    between: float = 0.0                  # bound between the two runs (0: bit-identical)
    pool_first: bool = False              # a max-pooled row whose epilogue is not monotone: equal to the TH_NO_POOL_FIRST=1 run
    pool_first_bound: float = 0.0         # ... bit for bit (0), or within this where the knob itself takes the kernel away

    def model(self):
        """(model_config, weights, names of the layers to compare)"""
        b = Builder(self.shape, seed=1000 + self.seed)
        out = self.build(b)
        cfg, weights = b.finish(out)
        return cfg, weights, list(b.probes)

    def frames(self) -> np.ndarray:
        if self.make_frames is not None:
            return self.make_frames(self)
        return half_zero_frames(self.n, self.shape, 77 + self.seed, self.scale)


CASES: List[Case] = []
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_set_golden.npz")
_seed = itertools.count(1)


def case(name, group, shape, build, **kw):
    assert name not in {c.name for c in CASES}, name
    CASES.append(Case(name=name, group=group, shape=tuple(shape), build=build, seed=next(_seed), **kw))


# ---- group 1: activations as layer arguments (fused into the convolution) and as stand-alone layers with two consumers --------
# (label, what Conv3D's `activation` argument takes or None, the layer form)
ACTIVATIONS = [
    ("sigmoid", "sigmoid", lambda b, x: b.activation(x, "sigmoid")),
    ("tanh", "tanh", lambda b, x: b.activation(x, "tanh")),
    ("elu_1", "elu", lambda b, x: b.elu(x, 1.0)),
    ("elu_07", None, lambda b, x: b.elu(x, 0.7)),
    ("elu_neg05", None, lambda b, x: b.elu(x, -0.5)),
    ("leaky_str", "leaky_relu", lambda b, x: b.activation(x, "leaky_relu")),
    ("leaky_layer", None, lambda b, x: b.leaky_relu(x, 0.3)),
    ("relu_slope", None, lambda b, x: b.relu_slope(x, 0.1)),
    ("relu", "relu", lambda b, x: b.relu(x)),
    ("linear", "linear", lambda b, x: b.activation(x, "linear")),
    ("softmax", "softmax", lambda b, x: b.softmax(x)),
]


def _activation_case(arg, layer):
    def build(b):
        x = b.input_name
        # behind a Conv3D that the planner fuses: as the layer's own argument where Keras has a name for it, else as the next layer
        p = b.conv3d(x, 5, 3, padding="same", activation=arg) if arg is not None else layer(b, b.conv3d(x, 5, 3, padding="same"))
        # stand-alone: its input has two consumers (nothing absorbs it as an epilogue) and so has its output (nor as a prologue)
        c = b.conv3d(x, 4, 1, padding="same")
        s = b.keep(layer(b, c))
        t = b.conv3d(s, 3, 1, padding="same")
        return b.flatten(b.concat([p, c, s, t]))         # the output holds every tensor of the case, element by element
    return build


for _label, _arg, _layer in ACTIVATIONS:
    case(f"act_{_label}", 1, (3, 3, 2, 3), _activation_case(_arg, _layer), n=5, scale=3.0,
         must=(r": softmax$",) if _label == "softmax" else (r": activation$",))


# ---- group 2: BatchNormalization ----------------------------------------------------------------------------------------------
def _bn_rank4(center, scale):
    def build(b):
        x = b.input_name
        a = b.conv3d(x, 6, 3, padding="same")
        bn1 = b.batchnorm(a, epsilon=1e-3, center=center, scale=scale)       # the convolution's epilogue
        r = b.keep(b.relu(bn1))
        bn2 = b.keep(b.batchnorm(x, epsilon=1e-5, center=center, scale=scale))   # on the model input, two consumers: a step of its own
        if scale:
            b.negate_gamma(bn1)
            b.negate_gamma(bn2, 2)
        c = b.conv3d(bn2, 4, 3, padding="same")
        return b.flatten(b.concat([r, c, bn2]))
    return build


def _bn_rank1(center, scale, eps):
    def build(b):
        x = b.flatten(b.input_name)
        d = b.dense(x, 12)
        bn = b.keep(b.batchnorm(d, epsilon=eps, center=center, scale=scale))
        if scale:
            b.negate_gamma(bn)
        return b.dense(b.relu(bn), 5)
    return build


for _c, _s in ((True, True), (True, False), (False, True), (False, False)):
    _tag = f"center{int(_c)}_scale{int(_s)}"
    case(f"bn_rank4_{_tag}", 2, (3, 4, 2, 3), _bn_rank4(_c, _s), n=5, must=(r": batchnorm$",))
    case(f"bn_rank1_{_tag}", 2, (2, 3, 2, 3), _bn_rank1(_c, _s, 1e-5 if _c == _s else 1e-3), n=7)       # (the Dense layer's epilogue)


# ---- group 3: pooling off 2^3 / 'valid' ---------------------------------------------------------------------------------------
POOLS = [(2, 2, "valid"), (3, 2, "same"), (3, 1, "same"), (2, 1, "valid"), ((1, 2, 3), (1, 2, 3), "valid"),
         ((3, 2, 1), (2, 1, 1), "same"), (2, 3, "same"), (4, 4, "same")]
POOL_EXTENTS = [(5, 6, 7), (8, 4, 3)]


def _pool_case(arena):
    def build(b):
        x = b.input_name
        if arena:
            # the pools read the second input of a Concatenate: a channel offset of 3 and a channel stride of 5
            first = b.conv3d(x, 3, 1, padding="same", activation="tanh")
            y = b.keep(b.conv3d(x, 2, 3, padding="same"))
            cat = b.concat([first, y])
        else:
            y = b.keep(b.conv3d(x, 2, 3, padding="same"))
        heads = []
        for kind in ("max", "avg"):
            vs = [b.gmp(b.keep(b.pool(kind, y, p, s, pad))) for p, s, pad in POOLS]
            heads.append(b.concat(vs))
        if arena:
            heads.append(b.gap(cat))
        return b.concat(heads)
    return build


for _ext in POOL_EXTENTS:
    for _arena in (False, True):
        case(f"pool_{'x'.join(map(str, _ext))}_{'arena' if _arena else 'plain'}", 3, (*_ext, 2), _pool_case(_arena), n=3,
             must=(r": maxpool3d$", r": avgpool3d$"))


def _pool_same_not_fused(b):
    x = b.elu(b.conv3d(b.input_name, 6, 3, padding="same"))
    return b.flatten(b.keep(b.pool("max", x, 2, 2, "same")))


case("pool_conv_elu_maxpool_same_odd", 3, (5, 7, 5, 3), _pool_same_not_fused, n=5, must=(r": maxpool3d$",), must_not=(r"pool1",))


# ---- group 4: global pools ----------------------------------------------------------------------------------------------------
def _global_case(kind, C, tail, arena=False):
    def build(b):
        x = b.input_name
        if arena:
            a = b.conv3d(x, C - 7, 3, padding="same")
            y = b.conv3d(x, 7, 1, padding="same")
            x = b.concat([a, y])
        else:
            x = b.conv3d(x, C, 3, padding="same")
        g = b.keep(b.gmp(x) if kind == "gmp" else b.gap(x))
        if tail == "softmax":
            return b.softmax(g)
        if tail == "dense_softmax":
            return b.softmax(b.keep(b.dense(g, 9)))
        return b.dense(b.keep(b.dense(g, 11, activation="relu")), 6, activation="softmax")
    return build


for _kind in ("gmp", "gap"):
    for _C in (1, 20, 65):
        for _tail in ("softmax", "dense_softmax", "dense_relu_dense_softmax"):
            _fused = _kind == "gap" and _tail != "dense_relu_dense_softmax"
            _must = {("gap", "softmax"): (r"k_gap_softmax",), ("gap", "dense_softmax"): (r"k_tail_dense",)}.get((_kind, _tail), ())
            if _kind == "gmp":
                _must = (r": global_max_pool$",)
            case(f"{_kind}_c{_C}_{_tail}", 4, (3, 2, 4, 3), _global_case(_kind, _C, _tail), n=7, must=_must, tail=_fused,
                 must_not=(r"k_gap_softmax", r"k_tail_dense") if _kind == "gmp" else ())
    case(f"{_kind}_arena_softmax", 4, (3, 2, 4, 3), _global_case(_kind, 20, "softmax", arena=True), n=7, tail=_kind == "gap",
         must=(r"k_gap_softmax",) if _kind == "gap" else (r": global_max_pool$",))


# ---- group 5: softmax numerics ------------------------------------------------------------------------------------------------
SOFTMAX_C = [1, 63, 64, 65, 338, 513]


def softmax_rows(C, seed):
    """the hand-written logit rows, then two random ones: +1e4 next to 0, -1e4 next to 0, all entries equal, two exact ties at the
    maximum, -1e30 next to small values"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((7, C), dtype=np.float32)
    rows[0, C // 2] = 1e4
    rows[1, :] = 0.0
    rows[1, (C // 3)] = -1e4
    rows[2, :] = 2.5
    rows[3] = rng.standard_normal(C).astype(np.float32)
    rows[3, [0, C - 1]] = 6.0
    rows[4] = rng.standard_normal(C).astype(np.float32)
    rows[4, ::2] = -1e30
    rows[5] = rng.standard_normal(C).astype(np.float32) * 4
    rows[6] = rng.standard_normal(C).astype(np.float32) * (rng.random(C) < 0.5)
    return rows


def _flatten_softmax(b):
    return b.softmax(b.flatten(b.input_name))


def _identity_conv_gap_softmax(b):
    C = b.shapes[b.input_name][-1]
    c = b.conv3d(b.input_name, C, 1, padding="same")
    b.weights[c] = [np.eye(C, dtype=np.float32).reshape(1, 1, 1, C, C), np.zeros(C, dtype=np.float32)]
    return b.softmax(b.gap(c))


for _C in SOFTMAX_C:
    case(f"softmax_flatten_c{_C}", 5, (1, 1, 1, _C), _flatten_softmax, n=7,
         make_frames=lambda cs: softmax_rows(cs.shape[-1], cs.seed).reshape(7, 1, 1, 1, -1))
    # two voxels that hold the same row: their mean is the row, exactly
    case(f"softmax_conv_gap_c{_C}", 5, (2, 1, 1, _C), _identity_conv_gap_softmax, n=7, tail=_C <= 512,
         make_frames=lambda cs: np.repeat(softmax_rows(cs.shape[-1], cs.seed).reshape(7, 1, 1, 1, -1), 2, axis=1))


# ---- group 6: the limits of the fused tails (k_gap_softmax: C <= 512; k_tail_dense: F <= 2048, O <= 512) ----------------------
def _gap_softmax(b):
    return b.softmax(b.keep(b.gap(b.input_name)))


def _tail_dense(units):
    def build(b):
        x = b.relu(b.batchnorm(b.input_name))
        return b.softmax(b.keep(b.dense(b.gap(x), units)))
    return build


case("limit_gap_softmax_c512", 6, (2, 1, 1, 512), _gap_softmax, n=3, must=(r"k_gap_softmax",), tail=True)
case("limit_gap_softmax_c513", 6, (2, 1, 1, 513), _gap_softmax, n=3, must_not=(r"k_gap_softmax",),
     order=(r": global_avg_pool$", r": softmax$"))
case("limit_tail_dense_f2048_o20", 6, (2, 1, 1, 2048), _tail_dense(20), n=3, must=(r"k_tail_dense",), tail=True)
case("limit_tail_dense_f24_o512", 6, (2, 2, 2, 24), _tail_dense(512), n=3, must=(r"k_tail_dense",), tail=True)
case("limit_tail_dense_f2049_o20", 6, (2, 1, 1, 2049), _tail_dense(20), n=3, must_not=(r"k_tail_dense",),
     order=(r": global_avg_pool$", r": dense", r": softmax$"))
case("limit_tail_dense_f24_o513", 6, (2, 2, 2, 24), _tail_dense(513), n=3, must_not=(r"k_tail_dense",),
     order=(r": global_avg_pool$", r": dense", r": softmax$"))


# ---- group 7: Add and Concatenate ---------------------------------------------------------------------------------------------
def _add_case(branches):
    def build(b):
        x = b.conv3d(b.input_name, 6, 3, padding="same", activation="relu")      # the block input is one of the summands
        ys = [x] + [b.conv3d(x, 6, k, padding="same", activation=a) for k, a in (((3, 1, 3), "elu"), (1, "tanh"), (3, "linear"))][:branches - 1]
        return b.flatten(b.add(ys))
    return build


def _add_twice(b):
    x = b.conv3d(b.input_name, 5, 3, padding="same")
    return b.flatten(b.add([x, x]))


def _concat_copy_input(b):
    x = b.input_name
    return b.flatten(b.concat([x, b.conv3d(x, 5, 3, padding="same", activation="relu")]))


def _concat_copy_flatten(b):
    x = b.input_name
    f1 = b.flatten(b.conv3d(x, 3, 3, padding="same"))
    f2 = b.flatten(b.pool("avg", x, 2, 1, "valid"))
    return b.dense(b.keep(b.concat([f1, f2])), 7)


def _concat_of_concats(b):
    x = b.input_name
    a = b.conv3d(x, 3, 3, padding="same", activation="relu")
    c = b.conv3d(x, 5, 1, padding="same")
    inner = b.keep(b.concat([a, c]))
    d = b.conv3d(inner, 4, 3, padding="same", activation="elu")
    e = b.conv3d(x, 2, (1, 3, 1), padding="same")
    outer = b.keep(b.concat([inner, d, e]))
    return b.flatten(b.conv3d(outer, 6, 1, padding="same"))


def _flatten_of_arena_slice(b):
    x = b.input_name
    a = b.conv3d(x, 3, 1, padding="same")
    y = b.conv3d(x, 4, 3, padding="same", activation="relu")
    cat = b.concat([a, y])
    f = b.keep(b.flatten(y))                             # y lives in the arena at channel offset 3, stride 7
    g = b.gap(cat)
    return b.dense(b.concat([f, g]), 6)


for _k in (2, 3, 4):
    case(f"add_{_k}_branches", 7, (4, 3, 3, 3), _add_case(_k), n=5, must=(r": add$",))
case("add_x_x", 7, (3, 3, 2, 4), _add_twice, n=3, must=(r": add$",))
case("concat_copy_input", 7, (3, 4, 3, 3), _concat_copy_input, n=5, must=(r"concat\(copy",))
case("concat_copy_flatten", 7, (3, 4, 3, 2), _concat_copy_flatten, n=5, must=(r"concat\(copy",))
case("concat_of_concats", 7, (3, 4, 3, 3), _concat_of_concats, n=5, must_not=(r"concat\(copy",))
case("flatten_of_arena_slice", 7, (3, 2, 3, 3), _flatten_of_arena_slice, n=5, must=(r"flatten\(copy\)",))


# ---- group 8: softmax as a layer activation, followed by more layers ----------------------------------------------------------
_LAYER_SOFTMAX = r"softmax \(layer activation\)"


def _dense_softmax_bn(b):
    d = b.keep(b.dense(b.flatten(b.input_name), 8, activation="softmax"))
    bn = b.keep(b.batchnorm(d))
    return b.softmax(b.dense(bn, 5))


def _conv_softmax_elu_pool(b):
    c = b.conv3d(b.input_name, 6, 1, activation="softmax")
    return b.flatten(b.keep(b.maxpool(b.keep(b.elu(c)), 2)))


def _conv_softmax_bn_gap(b):
    c = b.conv3d(b.input_name, 20, 3, padding="same", activation="softmax")
    return b.gap(b.keep(b.batchnorm(c)))


def _conv_softmax_avgpool(b):
    c = b.conv3d(b.input_name, 4, 3, padding="valid", activation="softmax")
    return b.flatten(b.keep(b.avgpool(c, 2)))


case("layer_softmax_dense_bn", 8, (2, 3, 2, 3), _dense_softmax_bn, n=7, order=(_LAYER_SOFTMAX, r": batchnorm$"))
case("layer_softmax_conv_elu_maxpool", 8, (4, 4, 2, 5), _conv_softmax_elu_pool, n=5, scale=2.0,
     order=(_LAYER_SOFTMAX, r": activation$", r": maxpool3d$"))
case("layer_softmax_conv_bn_gap", 8, (3, 2, 3, 6), _conv_softmax_bn_gap, n=5, scale=2.0,
     order=(_LAYER_SOFTMAX, r": batchnorm$", r": global_avg_pool$"))
case("layer_softmax_conv_avgpool", 8, (6, 4, 5, 5), _conv_softmax_avgpool, n=5, scale=2.0, order=(_LAYER_SOFTMAX, r": avgpool3d$"))


# ---- group 9: input dtypes into a first node that is not a convolution (k_convert_frames) -------------------------------------
INPUT_DTYPES = [np.float32, np.float64, np.uint8, np.bool_, np.float16]


def _input_avgpool(b):
    return b.flatten(b.keep(b.avgpool(b.input_name, 2)))


def _input_concat(b):
    x = b.input_name
    return b.flatten(b.keep(b.concat([x, b.conv3d(x, 4, 3, padding="same")])))


def _input_conv_only(b):
    return b.flatten(b.conv3d(b.input_name, 4, 3, padding="same"))       # 3 channels stored with a channel stride of 4


_binary = lambda cs: binary_frames(cs.n, cs.shape, cs.seed)                # noqa: E731
case("dtype_input_avgpool", 9, (4, 5, 6, 3), _input_avgpool, n=5, make_frames=_binary, must=(r": avgpool3d$",))
case("dtype_input_concat", 9, (4, 3, 5, 3), _input_concat, n=5, make_frames=_binary, must=(r"concat\(copy input\)",))
case("dtype_input_conv", 9, (4, 3, 5, 3), _input_conv_only, n=5, make_frames=_binary)


# ---- group 10: one sigmoid row and one elu(alpha=0.7) row per fused kernel family, one BN -> sigmoid -> Conv prologue row for the
# families that take a PreOp, one elu(alpha=-0.5) row for the max-pooled ones.  Each family's smallest selecting shape, the knobs and
# the bounds are those of its own test file (named per family); compared with the oracle in float64 ---------------------------------
def _family_conv(cout, k, strides, pool, act, pre):
    def build(b):
        x = b.input_name
        if pre:
            x = b.activation(b.batchnorm(x), "sigmoid")
        x = b.conv3d(x, cout, k, strides=strides, padding="same")
        x = b.activation(x, "sigmoid") if act == "sigmoid" else b.elu(x, {"elu07": 0.7, "eluneg": -0.5}[act])
        if pool:
            x = b.maxpool(x, 2)
        return b.flatten(x)
    return build


def _family_dense(act):
    def build(b):
        x = b.dense(b.flatten(b.input_name), 128)
        return b.activation(x, "sigmoid") if act == "sigmoid" else b.elu(x, 0.7)
    return build


def _family_tail(act):
    def build(b):
        x = b.batchnorm(b.input_name)
        x = b.activation(x, "sigmoid") if act == "sigmoid" else b.elu(x, 0.7)
        return b.softmax(b.dense(b.gap(x), 20))
    return build


_NO_MFMA = {"flags": 2}       # TH_LOAD_NO_MFMA: the families without a knob of their own
# family: (input shape, Cout, kernel, stride, max pool, frames, label pattern, env, bound, off, between, takes a PreOp)
FAMILIES = {
    # test_gpu_conv_sweep.py::test_first_layer_on_the_bf16_pipe_with_split_operands: 2e-5; 4e-6 to TH_FIRST_SPLIT=0
    "k_conv_first_b3": ((21, 21, 21, 6), 32, 3, 1, True, 2, r"k_conv_first_b3", None, 2e-5, {"TH_FIRST_SPLIT": "0"}, 4e-6, False),
    # test_gpu_conv_sweep.py::test_first_layer_winograd_along_x: 2e-5; 4e-6 to TH_FIRST_WINO=0
    "k_conv_first_w": ((7, 6, 6, 4), 33, 3, 1, True, 3, r"k_conv_first_w", None, 2e-5, {"TH_FIRST_WINO": "0"}, 4e-6, False),
    # test_gpu_conv_first5.py: 2e-5; 4e-6 to TH_FIRST_SPLIT=0
    "k_conv_first5": ((21, 21, 21, 5), 9, 5, 1, True, 2, r"k_conv_first5", None, 2e-5, {"TH_FIRST_SPLIT": "0"}, 4e-6, False),
    # test_gpu_conv_sweep.py / test_gpu_conv_brick.py: 2e-5 to the oracle, 2e-5 between the kernel and the direct plan
    "k_conv_mfma": ((5, 5, 5, 64), 128, 3, 1, False, 5, r"k_conv_mfma<", {"TH_WINOGRAD": "0"}, 2e-5, _NO_MFMA, 2e-5, True),
    "k_conv_n16": ((6, 6, 6, 48), 16, 3, 1, False, 5, r"k_conv_n16<", None, 2e-5, _NO_MFMA, 2e-5, True),
    # test_gpu_conv_pointwise.py: 2e-5 to the oracle; the file has no bound between two plans: the sweep's 2e-5
    "k_conv_pw": ((8, 8, 8, 20), 64, 1, 1, False, 3, r"k_conv_pw<", None, 2e-5, _NO_MFMA, 2e-5, False),
    "k_conv_pw2": ((8, 8, 8, 32), 64, 1, 1, False, 3, r"k_conv_pw2<", None, 2e-5, _NO_MFMA, 2e-5, True),
    # test_gpu_conv_gl.py: 5e-6 to the float64 oracle; 3e-6 to TH_CONV_GL=0
    "conv_gl": ((9, 9, 9, 16), 20, 3, 2, False, 5, r"k_conv_gl", None, 5e-6, {"TH_CONV_GL": "0"}, 3e-6, False),
    # test_gpu_conv_wfused.py: 2e-5; 4e-5 to TH_WFUSED=0
    "conv_wfused": ((10, 10, 10, 32), 64, 3, 1, False, 3, r"k_conv_wf<", {"TH_WF_SPLIT": "0"}, 2e-5, {"TH_WFUSED": "0"}, 4e-5, True),
    # test_gpu_conv_wfsplit.py: 2e-5; 4e-6 to TH_WF_SPLIT=0
    # (conv_wfs_plan declines a layer with an input prologue: its slices go from HBM to LDS without passing through registers)
    "conv_wfsplit": ((10, 10, 10, 32), 64, 3, 1, False, 3, r"k_conv_wfs<", None, 2e-5, {"TH_WF_SPLIT": "0"}, 4e-6, False),
    # test_gpu_wino.py: LAYER = 1e-5 on a layer's tensor; the file bounds no layer tensor between two plans: the sweep's 2e-5
    "conv_wino": ((5, 5, 5, 64), 128, 3, 1, False, 5, r"conv_wino", None, 1e-5, {"TH_WINOGRAD": "0"}, 2e-5, False),
}

for _fam, (_shape, _cout, _k, _st, _pool, _n, _pat, _env, _bound, _off, _btw, _preop) in FAMILIES.items():
    for _act in ("sigmoid", "elu07"):
        case(f"family_{_fam}_{_act}", 10, _shape, _family_conv(_cout, _k, _st, _pool, _act, False), n=_n, must=(_pat,), env=_env,
             bound=_bound, off=_off, between=_btw)
    if _preop:
        case(f"family_{_fam}_prologue", 10, _shape, _family_conv(_cout, _k, _st, _pool, "elu07", True), n=_n, must=(_pat,), env=_env,
             bound=_bound, off=_off, between=_btw)
    if _pool:
        # not monotone: the kernel must not pool the raw sums first (conv_first_b3 declines such a chain, the fp32-input kernel runs)
        # k_conv_first5 is not planned under TH_NO_POOL_FIRST=1 (conv_first5_ok): that run is the fp32-input kernel, another summation
        # order; the two are held to the 4e-6 test_gpu_conv_first5.py asserts between them, and the plan must name another kernel
        case(f"family_{_fam}_elu_negative", 10, _shape, _family_conv(_cout, _k, _st, True, "eluneg", False), n=_n, bound=_bound, pool_first=True,
             must=(_pat,) if _fam == "k_conv_first5" else (), pool_first_bound=_btw if _fam == "k_conv_first5" else 0.0)
# the two brick families with a fused max pool (test_gpu_conv_sweep.py: (4, 4, 4) 24 -> 20 and (10, 10, 10) 32 -> 64, both pooled)
case("family_k_conv_mfma_elu_negative", 10, (4, 4, 4, 24), _family_conv(20, 3, 1, True, "eluneg", False), n=3, must=(r"pool1.*k_conv_mfma<",),
     bound=2e-5, pool_first=True)
case("family_conv_wf_elu_negative", 10, (10, 10, 10, 32), _family_conv(64, 3, 1, True, "eluneg", False), n=3, must=(r"k_conv_wf",),
     bound=2e-5, pool_first=True)
# the same prologue row under the default knobs: the split kernel declines it and conv_wfused runs
case("family_conv_wfsplit_prologue", 10, (10, 10, 10, 32), _family_conv(64, 3, 1, False, "elu07", True), n=3, must=(r"k_conv_wf<",),
     must_not=(r"k_conv_wfs<",), bound=2e-5, off={"TH_WFUSED": "0"}, between=4e-5)
for _act in ("sigmoid", "elu07"):
    # test_gpu_dense_gemm.py: 5e-6 to the float64 oracle; 2e-6 to TH_DENSE_GEMM=0
    case(f"family_k_dense_gemm_{_act}", 10, (4, 4, 4, 8), _family_dense(_act), n=5, must=(r"k_dense_gemm",), bound=5e-6,
         off={"TH_DENSE_GEMM": "0"}, between=2e-6)
    # test_gpu_cnn.py: 5e-6 to the float64 oracle; bit-identical to TH_NO_TAIL_FUSE=1
    case(f"family_k_tail_dense_{_act}", 10, (2, 2, 2, 24), _family_tail(_act), n=5, must=(r"k_tail_dense",), bound=5e-6,
         off={"TH_NO_TAIL_FUSE": "1"}, between=0.0)


def family_cases() -> List[Case]:
    return [c for c in CASES if c.group == 10]


def fixture_cases() -> List[Case]:
    """groups 1 to 9: the rows tests/golden/op_set_golden.npz holds"""
    return [c for c in CASES if c.group <= 9]
