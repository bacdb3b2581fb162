"""The case table of the two brick convolution kernels, k_conv_mfma (csrc/conv_mfma.hip) and k_conv_n16 (csrc/conv_n16.hip), shared by
tests/test_conv_brick_host.py (no GPU: every compiled instantiation is the expected kernel of a row, every staging mode of the plan
arithmetic occurs) and tests/test_gpu_conv_brick.py (every row against the float64 oracle).

A row is one convolution and the net around it.  Which instantiation and which brick (FB frames per workgroup, ZB of Dc computed
planes per z-brick) the planner gives it is asked of th_conv_brick_pick; the `kernel`, `FB`, `ZB`, `nzb` columns say what the row is
in the table FOR, and the host test holds the pick to them, so a changed plan rule shows up as a row that no longer reaches its kernel.

    front   input: the convolution reads the model input (Cin > 8, or behind a prologue: a bare Cin <= 8 stem goes to conv_first)
            pw:    a 1x1x1 convolution from FRONT_CH channels in front, a dense tensor of its own
            slice: two 1x1x1 convolutions write channels 0..17 and 18.. of a concat arena; the row reads the second slice (channel
                   offset 18: no multiple of 4, scalar staging loads) and writes its output behind ELU(arena) into a second arena
    pre     none | bn_relu | relu | bn_elu          the prologue folded into the staging
    epi     none | relu | elu | elu_bn | bn_relu | leaky | tanh | bn_neg (BatchNorm with every third gamma negative: not monotone,
            so a max-pool cannot move in front of it)
    env     knobs a shape needs to stay off another kernel family (5^3: conv_wino, 10^3: conv_wfused), or TH_N16_RESIDENT
    kernel  the instantiation(s) the row runs: two for a layer whose last Cout block runs on a narrower kernel (conv_mfma_plan_tail)
"""
import ctypes as C
import re
from collections import namedtuple

import numpy as np

Row = namedtuple("Row", "id vol cin cout k stride padding pool epi pre front bias env n kernel FB ZB nzb")

FRONT_CH = 5          # channels of the model input in front of a `pw` / `slice` row
SLICE_OFF = 18        # channels of the first slice of the arena a `slice` row reads
POOLS = ("none", "max", "avg")
W0, WF0 = {"TH_WINOGRAD": "0"}, {"TH_WFUSED": "0"}


def _m(*a):
    return "k_conv_mfma<%d,%d,%d,%d,%d,%d,%d,%d>" % a


def _n(*a):
    return "k_conv_n16<%d,%d,%d,%d,%d>" % a


def _rows():
    R = []

    def add(id, vol, cin, cout, kernel, FB, ZB, nzb, n, k=3, stride=1, padding="same", pool="none", epi="none", pre="none", front=None,
            bias=True, env=None):
        front = front or ("input" if cin > 8 or pre != "none" else "pw")
        R.append(Row(id, vol, cin, cout, k, stride, padding, pool, epi, pre, front, bias, dict(env or {}), n,
                     kernel if isinstance(kernel, tuple) else (kernel,), FB, ZB, nzb))

    # ---- k_conv_mfma, 8-channel chunks (Cin <= 8, Cout <= 64): weights resident in LDS (kC8Res32 / 64) or streamed (kC8Str32 / 64) ----
    add("res32-k5-zbrick", (9, 8, 7), 6, 20, _m(8, 1, 1, 1, 8, 1, 0, 0), 1, 3, 3, 3, k=5, epi="elu_bn")
    add("res32-max-fb4", (9, 8, 7), 6, 20, _m(8, 1, 1, 1, 8, 1, 1, 0), 4, 8, 1, 7, pool="max", epi="bn_neg", pre="bn_relu")
    add("res32-avg-fb4", (9, 8, 7), 6, 20, _m(8, 1, 1, 1, 8, 1, 2, 0), 4, 8, 1, 5, pool="avg", epi="relu")
    add("res32-valid-fb6", (9, 8, 7), 8, 30, _m(8, 1, 1, 1, 8, 1, 0, 0), 6, 7, 1, 8, padding="valid", epi="bn_relu")
    add("res32-fb16", (3, 3, 3), 6, 32, _m(8, 1, 1, 1, 8, 1, 0, 0), 16, 3, 1, 19, epi="leaky", bias=False)
    add("res64", (12, 11, 10), 7, 64, _m(8, 2, 2, 2, 8, 1, 0, 0), 1, 12, 1, 3, epi="elu")
    add("res64-max", (12, 11, 10), 7, 64, _m(8, 2, 2, 2, 8, 1, 1, 0), 1, 12, 1, 3, pool="max", epi="elu_bn")
    add("res64-avg", (13, 10, 11), 8, 40, _m(8, 2, 2, 2, 8, 1, 2, 0), 1, 12, 1, 3, pool="avg", epi="bn_relu", pre="relu")
    add("res64-avg-zbrick21", (21, 21, 21), 8, 64, _m(8, 2, 2, 2, 8, 1, 2, 0), 1, 2, 10, 3, pool="avg", epi="elu_bn")
    add("str64-k5", (9, 8, 8), 8, 64, _m(8, 2, 2, 2, 8, 2, 0, 0), 2, 9, 1, 5, k=5, epi="tanh")
    add("str64-k5-max", (9, 8, 8), 8, 64, _m(8, 2, 2, 2, 8, 2, 1, 0), 2, 8, 1, 5, k=5, pool="max", epi="bn_neg")
    add("str64-k5-avg", (10, 9, 8), 5, 48, _m(8, 2, 2, 2, 8, 2, 2, 0), 2, 10, 1, 5, k=5, pool="avg", epi="elu_bn", pre="bn_relu")
    add("str32-k755", (8, 8, 8), 5, 24, _m(8, 2, 1, 1, 8, 2, 0, 0), 2, 8, 1, 5, k=(7, 5, 5), epi="bn_relu")
    add("str32-k5-max", (8, 12, 12), 6, 24, _m(8, 2, 1, 1, 8, 2, 1, 0), 1, 8, 1, 3, k=5, pool="max", epi="elu_bn")
    add("str32-k755-avg", (8, 8, 8), 5, 24, _m(8, 2, 1, 1, 8, 2, 2, 0), 2, 8, 1, 5, k=(7, 5, 5), pool="avg", epi="leaky", bias=False)
    # ---- 16-channel chunks, whole frames in half the LDS: two 4-wave workgroups per CU (kS4N32 / 64 / 128); three ragged chunks ------
    for pool, couts, zb in (("avg", (32, 64, 128), 6), ("max", (30, 50, 100), 6), ("none", (32, 64, 128), 7)):
        for cout, (tm, tn, nt), epi, pre in zip(couts, ((2, 1, 1), (4, 2, 2), (4, 2, 4)), ("elu_bn", "bn_neg", "relu"), ("bn_relu", "none", "none")):
            add(f"s4n{32 * nt}-{pool}", (7, 6, 6), 40, cout, _m(4, tm, tn, nt, 16, 2, POOLS.index(pool), 0), 1, zb, 1, 3, pool=pool, epi=epi, pre=pre)
    # ---- 16-channel chunks, z-bricks on one 8-wave workgroup (kS8N32 / 64 / 128) --------------------------------------------------
    for cout, (tm, tn, nt), epi in zip((32, 64, 128), ((2, 1, 1), (4, 2, 2), (4, 2, 4)), ("elu_bn", "tanh", "bn_relu")):
        add(f"s8n{32 * nt}-avg-zbrick", (13, 12, 10), 40, cout, _m(8, tm, tn, nt, 16, 2, 2, 0), 1, 6, 2, 3, pool="avg", epi=epi,
            pre="bn_relu" if nt == 2 else "none")
    for cout, (tm, tn, nt), epi in zip((28, 50, 130), ((2, 1, 1), (4, 2, 2), (4, 2, 4)), ("bn_neg", "elu_bn", "elu_bn")):
        add(f"s8n{32 * nt}-max-zbrick-odd", (13, 12, 10), 24, cout, _m(8, tm, tn, nt, 16, 2, 1, 0), 1, 6, 2, 3, pool="max", epi=epi)
    for cout, (tm, tn, nt), epi in zip((30, 60, 100), ((2, 1, 1), (4, 2, 2), (4, 2, 4)), ("relu", "elu_bn", "leaky")):
        add(f"s8n{32 * nt}-zbrick-ragged", (17, 14, 13), 24, cout, _m(8, tm, tn, nt, 16, 2, 0, 0), 1, 5, 4, 3, epi=epi,
            pre="bn_relu" if nt == 4 else "none", bias=nt != 2)
    add("s8n64-stride2-zbrick", (15, 13, 12), 20, 40, _m(8, 4, 2, 2, 16, 2, 0, 0), 1, 4, 2, 3, stride=2, epi="elu_bn")
    add("s8n64-stride3", (11, 10, 9), 24, 40, _m(8, 4, 2, 2, 16, 2, 0, 0), 1, 4, 1, 3, stride=3, epi="relu")
    add("s8n64-k4", (9, 9, 9), 24, 40, _m(8, 4, 2, 2, 16, 2, 0, 0), 1, 9, 1, 3, k=4, epi="elu")
    add("s8n64-k313", (9, 9, 8), 24, 40, _m(8, 4, 2, 2, 16, 2, 0, 0), 1, 9, 1, 3, k=(3, 1, 3), epi="bn_relu", pre="bn_elu")
    add("s8n64-slice", (9, 8, 7), 24, 40, _m(8, 4, 2, 2, 16, 2, 0, 0), 1, 9, 1, 3, epi="elu_bn", front="slice")
    # ---- compile-time geometry (kMfmaGeo) and the heterogeneous Cout blocks that reach kS4N96 ------------------------------------------
    add("geo7-s4n128-compact", (5, 5, 5), 32, 128, _m(4, 4, 2, 4, 16, 2, 0, 7), 2, 5, 1, 5, epi="elu_bn", pre="bn_relu", env=W0)
    add("geo7-s4n128-cin40", (5, 5, 5), 40, 128, _m(4, 4, 2, 4, 16, 2, 0, 7), 2, 5, 1, 5, epi="elu_bn", pre="bn_relu", env=W0)
    add("geo7-s4n64", (5, 5, 5), 32, 64, _m(4, 4, 2, 2, 16, 2, 0, 7), 2, 5, 1, 5, epi="relu", env=W0)
    add("geo7-tail96", (5, 5, 5), 32, 208, (_m(4, 4, 2, 4, 16, 2, 0, 7), _m(4, 2, 3, 3, 16, 2, 0, 7)), 2, 5, 1, 5, epi="bn_relu", env=W0)
    add("tail96-max", (4, 4, 4), 32, 210, (_m(4, 4, 2, 4, 16, 2, 1, 0), _m(4, 2, 3, 3, 16, 2, 1, 0)), 4, 4, 1, 7, pool="max", epi="elu_bn")
    add("tail96-avg", (4, 4, 4), 32, 210, (_m(4, 4, 2, 4, 16, 2, 2, 0), _m(4, 2, 3, 3, 16, 2, 2, 0)), 4, 4, 1, 5, pool="avg", epi="bn_neg")
    add("tail96", (6, 5, 4), 32, 210, (_m(4, 4, 2, 4, 16, 2, 0, 0), _m(4, 2, 3, 3, 16, 2, 0, 0)), 2, 6, 1, 5, epi="leaky")
    add("geo12-s8n64-max", (10, 10, 10), 32, 64, _m(8, 4, 2, 2, 16, 2, 1, 12), 1, 10, 1, 3, pool="max", epi="elu_bn", pre="bn_relu", env=WF0)
    # ---- k_conv_n16 ---------------------------------------------------------------------------------------------------------------
    add("n16-w8-max", (10, 10, 10), 48, 16, _n(8, 8, 1, 0, 0), 1, 10, 1, 3, pool="max", epi="elu_bn", pre="bn_relu", env=WF0)
    add("n16-w8-avg", (11, 10, 10), 48, 12, _n(8, 8, 2, 0, 0), 1, 10, 1, 3, pool="avg", epi="bn_neg")
    add("n16-w4-avg", (7, 6, 4), 20, 16, _n(4, 4, 2, 0, 0), 1, 6, 1, 3, pool="avg", epi="relu", pre="bn_relu")
    add("n16-w4-max-cout9", (7, 6, 4), 20, 9, _n(4, 4, 1, 0, 0), 1, 6, 1, 3, pool="max", epi="bn_neg")
    add("n16-w4-cout9", (7, 6, 4), 20, 9, _n(4, 4, 0, 0, 0), 1, 7, 1, 3, epi="elu_bn", bias=False)
    add("n16-w8-trips", (8, 7, 6), 24, 16, _n(8, 8, 0, 0, 0), 2, 8, 1, 7, epi="elu", pre="bn_relu", env={"TH_N16_RESIDENT": "3"})
    add("n16-w8-cout1", (8, 7, 6), 24, 1, _n(8, 8, 0, 0, 0), 2, 8, 1, 5, epi="bn_relu")
    add("n16-xc4-cout17", (6, 5, 4), 24, 17, _n(4, 4, 0, 4, 0), 2, 6, 1, 5, epi="elu_bn")
    add("n16-xc4-cout20", (6, 5, 4), 24, 20, _n(4, 4, 0, 4, 0), 2, 6, 1, 5, epi="tanh", pre="bn_relu")
    add("n16-geo12", (10, 10, 10), 48, 16, _n(8, 8, 0, 0, 12), 1, 10, 1, 3, epi="relu", env=WF0)
    add("n16-geo7", (5, 5, 5), 48, 16, _n(4, 4, 0, 0, 7), 2, 5, 1, 5, epi="elu_bn", pre="bn_relu")
    add("n16-geo7-xc4", (5, 5, 5), 48, 20, _n(4, 4, 0, 4, 7), 2, 5, 1, 5, epi="elu_bn")
    add("n16-geo4-fb16", (2, 2, 2), 32, 16, _n(4, 4, 0, 0, 4), 16, 2, 1, 19, epi="bn_relu", pre="relu")
    return R


ROWS = _rows()
# instantiations no layer the planner accepts can reach, with the rule that blocks them (file:line): none today
UNREACHABLE = {}


def row_id(r):
    return r.id


def _triple(v):
    return (v,) * 3 if isinstance(v, int) else tuple(v)


def in_view(r):
    """(in_cs, in_coff) of the view the row's convolution reads, in floats"""
    if r.front == "slice":
        return SLICE_OFF + r.cin, SLICE_OFF
    if r.front == "input" and r.pre == "none":
        return (r.cin + 3) // 4 * 4, 0          # a model input read by convolutions only has 16-byte voxel rows
    return r.cin, 0


def pick(lib, r):
    """th_conv_brick_pick's label for the row"""
    buf = C.create_string_buffer(512)
    cs, coff = in_view(r)
    rc = lib.th_conv_brick_pick(*r.vol, r.cin, r.cout, *_triple(r.k), (C.c_int * 3)(*_triple(r.stride)), (C.c_int * 3)(1, 1, 1),
                                int(r.padding == "same"), POOLS.index(r.pool), cs, coff, buf, 512)
    assert rc == 0, lib.th_last_error()
    return buf.value.decode()


def kernels(lib):
    buf = C.create_string_buffer(1 << 14)
    assert lib.th_conv_brick_kernels(buf, 1 << 14) == 0
    return buf.value.decode().split()


Plan = namedtuple("Plan", "kernels FB ZB Dc nzb rows nnb nchunks")


def parse(label, r):
    """what a plan label says, and what follows from it for the row: kernels named (main first), FB, ZB, Dc, the number of z-bricks, GEMM
    rows per frame-brick, Cout blocks of the main launch and Cin chunks"""
    names = re.findall(r"\[(k_conv_(?:mfma|n16)<[^\]]*>)\]", label)
    fb, zb, dc, rows = (int(v) for v in re.search(r" FB(\d+) ZB(\d+)/(\d+) rows(\d+) ", label).groups())
    a = [int(v) for v in names[0][names[0].index("<") + 1:-1].split(",")]
    if names[0].startswith("k_conv_mfma"):
        bn, ci = 32 * a[3], a[4]
        nnb = -(-r.cout // bn)
    else:
        ci, nnb = 16, 1
    return Plan(tuple(names), fb, zb, dc, -(-dc // zb), rows, nnb, -(-r.cin // ci))


def build(r, seed):
    """the row's net, Flatten-ed so that every voxel and channel is compared: (cfg, weights, name of the convolution under test)"""
    from timed_hip import synth
    b = synth.KerasGraphBuilder((*r.vol, r.cin if r.front == "input" else FRONT_CH), seed=seed, bias_std=0.3)
    x, cat = b.input_name, None
    if r.front == "pw":
        x = b.conv3d(x, r.cin, 1, padding="same")
    elif r.front == "slice":
        p = b.conv3d(x, SLICE_OFF, 1, padding="same")
        x = b.conv3d(x, r.cin, 1, padding="same")
        cat = b.concat([p, x])
    if r.pre == "bn_relu":
        x = b.relu(b.batchnorm(x))
    elif r.pre == "bn_elu":
        x = b.elu(b.batchnorm(x))
    elif r.pre == "relu":
        x = b.relu(x)
    conv = x = b.conv3d(x, r.cout, r.k, strides=r.stride, padding=r.padding, use_bias=r.bias)
    neg = None
    if r.epi == "elu_bn":
        x = b.batchnorm(b.elu(x))
    elif r.epi == "bn_relu":
        x = b.relu(b.batchnorm(x))
    elif r.epi == "bn_neg":
        neg = x = b.batchnorm(x)
    elif r.epi == "relu":
        x = b.relu(x)
    elif r.epi == "elu":
        x = b.elu(x, 0.7)
    elif r.epi == "leaky":
        x = b.leaky_relu(x, 0.2)
    elif r.epi == "tanh":
        x = b.activation(x, "tanh")
    if r.pool == "max":
        x = b.maxpool(x, 2)
    elif r.pool == "avg":
        x = b.avgpool(x, 2)
    if cat is not None:
        x = b.concat([b.elu(cat), x])          # the row's output lands at channel offset SLICE_OFF + Cin of this arena
    cfg, weights = b.finish(b.flatten(x))
    if neg is not None:
        g = weights[neg][0].copy()
        g[::3] *= -1.0
        weights[neg] = [g] + list(weights[neg][1:])
    return cfg, weights, conv


def frames(r, seed):
    """n frames, half of the values exact zeros"""
    rng = np.random.default_rng(seed)
    shape = (r.n, *r.vol, r.cin if r.front == "input" else FRONT_CH)
    return (rng.standard_normal(shape) * (rng.random(shape) < 0.5)).astype(np.float32)


def chunk_for(fb, n):
    """a chunk size c < FB that does not divide n, the largest there is: the batch then runs in ragged groups of other sizes than the
    default run's.  FB <= 2 leaves no such c (1 divides everything): then the smallest c that neither divides n nor is a multiple of
    FB (FB = 2, n = 5, c = 3: frames 2, 3, 4 change their partners), which still ends the batch on a short chunk"""
    for c in range(fb - 1, 1, -1):
        if n % c:
            return c
    return next(c for c in range(2, n) if n % c and (c % fb or fb == 1))
