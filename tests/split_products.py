"""CPU references for the split-operand ("bf16x3", csrc/bf16x3.h) convolution kernels.  Test infrastructure, not collected by pytest.

Every wide convolution multiplies on the bf16 matrix pipe with both operands cut exactly into three bf16 pieces x = h + m + l,
u = H + M + L, and keeps six of the nine piece products (KEEP6).  The three small kept ones (m*M, h*L, l*H) are each about 2^-18
of |x u|: on dense random frames a kernel that loses one of them moves its result by 1e-6 of the tensor's scale, below every
gate of the suite.  On frames with ONE nonzero voxel an output is a single product (a few dozen in a minimal-filtering form), and
measured in its natural unit

    u = 2^-24 * sum |a| |U| |v|        over every product that feeds the output in the kernel's own algorithm, in float64
                                       (the algorithm on absolute values: |v| = |B| |x|, |U| = |G| |w| |G|^T, |a| the entries of A)

the full scheme stays within a few u of float64 while a lost small product shows as ~100 u.  (A cruder unit, |x| max |w|, leaves
a Winograd form a separation of about 3: the unit has to follow the points.)  This module holds

    split_conv      one emulator of a 'same' convolution in the split scheme for the four algorithms of csrc/:
                      conv_wino      segments (None, [3, 2], [3, 2])   F(3,3)+F(2,3) in-plane, z taps direct
                      conv_wfsplit   segments (None, [2] * 5, [2] * 5) F(2,3)^2 in-plane, z taps direct
                      conv_first_b3  segments (None, None, [2] * 10)   F(2,3) along x, tap (2, 2, .) as plain fp32 products
                      conv_first5    segments (None, None, None)       direct 5^3
    natural_unit    the same algorithm on absolute values in float64, times 2^-24
    impulse_frames  frames with one nonzero full-mantissa fp32 voxel, and `expected`, their float64 result in closed form
    separation      E6 (all six products) and E5 (the best of the emulations that lose one small product) in units of u
    plain_conv      the same transforms with UNSPLIT operands: U rounded once to float32, one fp32 product per multiply-add, fp32
                    accumulation — what conv_wino.hip's fp32-input GEMM (k_wino_gemm, TH_WINO_SPLIT=0) computes; Eplain in separation

All of it is emulation on the CPU: it says what the scheme of bf16x3.h computes, not what a kernel computes.  The GPU tests
(tests/test_gpu_split_products.py) hold the kernels to the geometric mean of E6 and E5 — and the fp32-input GEMM, the plan the
load-time guard retreats to when the split kernels are off, to the geometric mean of Eplain and E5: the same side of the same line."""
from __future__ import annotations

import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_wino_tables import composite  # noqa: E402

# data piece (lower case) times weight piece (upper case), small products first: the order of conv_wino.hip's kWinoPA / kWinoPB
KEEP6 = ("lH", "hL", "mM", "mH", "hM", "hH")
ALL9 = KEEP6 + ("mL", "lM", "lL")
SMALL = ("lH", "mM", "hL")                     # the kept products a cheaper, wrong scheme would lose first
_PIECE = {"h": 0, "m": 1, "l": 2, "H": 0, "M": 1, "L": 2}

WINO = (None, [3, 2], [3, 2])
WFS = (None, [2] * 5, [2] * 5)
FIRST_B3 = (None, None, [2] * 10)
FIRST5 = (None, None, None)
B3_PLAIN_TAPS = ((2, 2),)                      # conv_first_b3: tap 8 = (dz, dy) = (2, 2) runs on the fp32 matrix pipe, unsplit


def _bf16(x):
    """round to nearest even to bfloat16, returned as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _split3(x):
    h = _bf16(x)
    m = _bf16(x - h)
    return h, m, _bf16(x - h - m)


def _split3_from64(x, exact_tail=False):
    """the host packers' split (bf16x3::split3): residuals in float64.  exact_tail: the third piece is the whole remainder
    (float64), so that the nine piece products add up to the product itself"""
    x = np.asarray(x, np.float64)
    h = _bf16(x.astype(np.float32)).astype(np.float64)
    m = _bf16((x - h).astype(np.float32)).astype(np.float64)
    r = x - h - m
    return h, m, (r if exact_tail else _bf16(r.astype(np.float32)).astype(np.float64))


def _axes(x_shape, k_shape, segments):
    """per spatial axis: None for a direct axis, (B [P, n_in], G [P, 3], A [n_out, P]) for a transformed one"""
    out = []
    for ax in range(3):
        seg, n_in, k = segments[ax], x_shape[1 + ax], k_shape[ax]
        if seg is None:
            out.append(None)
            continue
        n = sum(seg)
        assert k == 3 and n <= n_in <= n + 1, (ax, k, n, n_in)     # the padded input of n outputs is n + 2 wide
        BTc, Gc, ATc = composite(n, seg)
        out.append((BTc[:, 1:1 + n_in], Gc, ATc))
    return out


def _along(M, a, axis):
    """M [R, C] applied to axis `axis` (extent C) of a, in a's dtype"""
    return np.moveaxis(np.tensordot(M.astype(a.dtype), a, axes=([1], [axis])), 0, axis)


def _run(x, kernel, segments, mode, keep=KEEP6, dtype=np.float32, plain_taps=()):
    """mode "split": the piece products of `keep`, accumulated in `dtype`; mode "plain": unsplit operands, the weights rounded once
    to `dtype` after their float64 transform, one product per multiply-add, accumulated in `dtype`; mode "abs": every product of the
    same algorithm on absolute values, float64.  x [N, D, H, W, Cin], kernel [kd, kh, kw, Cin, Cout] -> [N, D', H', W', Cout]: a transformed axis has
    sum(segments) outputs, a direct one as many as inputs."""
    absolute = mode == "abs"
    dt = np.dtype(np.float64 if absolute else dtype)
    ax = _axes(x.shape, kernel.shape, segments)
    tr = [i for i in range(3) if ax[i] is not None]
    di = [i for i in range(3) if ax[i] is None]
    f = np.abs if absolute else (lambda a: a)
    # weights: transformed in float64 (the host packers), U [z: taps or points][y][x][ci][co]
    U = f(kernel.astype(np.float64))
    for i in tr:
        U = _along(f(ax[i][1]), U, i)
    # data: transformed in the working precision, y before x as the kernels do
    v = f(x.astype(dt))
    for i in tr:
        v = _along(f(ax[i][0]), v, 1 + i)
    if absolute:
        vp, Up = [v], [np.abs(U)]
        pairs = [(0, 0)]
    elif mode == "plain":
        vp, Up = [v], [U.astype(dt)]
        pairs = [(0, 0)]
    else:
        if dt == np.float32:
            vp = list(_split3(v))
            Up = [p.astype(np.float32) for p in _split3_from64(U)]
        else:                                   # float64: h and m as bf16, the tail exact — nine products are the product
            vp = list(_split3_from64(v, exact_tail=True))
            Up = list(_split3_from64(U, exact_tail=True))
        pairs = [(_PIECE[k[0]], _PIECE[k[1]]) for k in keep]
    # layout for the products: transformed axes lead (one weight matrix per point), rows are frames x the direct axes' voxels
    n_out = [x.shape[1 + i] for i in di]
    pads = [(kernel.shape[i] - 1) // 2 for i in di]
    perm = [1 + i for i in tr] + [0] + [1 + i for i in di] + [4]
    padw = [(0, 0)] * (len(tr) + 1) + [(p, p) for p in pads] + [(0, 0)]
    vp = [np.pad(np.transpose(p, perm), padw) for p in vp]
    if not absolute:
        vfull = np.pad(np.transpose(v, perm), padw)
    lead = vp[0].shape[:len(tr)]
    rows = x.shape[0] * int(np.prod(n_out, dtype=np.int64))
    uperm = tr + di + [3, 4]
    Up = [np.transpose(p, uperm) for p in Up]
    Ufull = np.transpose(U, uperm)
    acc = np.zeros(lead + (rows, kernel.shape[4]), dt)
    for tap in itertools.product(*[range(kernel.shape[i]) for i in di]):
        sl = (slice(None),) * (len(tr) + 1) + tuple(slice(t, t + n) for t, n in zip(tap, n_out))
        usl = (slice(None),) * len(tr) + tap

        def rows_of(a):
            return np.ascontiguousarray(a[sl]).reshape(lead + (rows, -1))
        if not absolute and tap[:2] in plain_taps and len(tap) >= 2:
            acc = acc + np.matmul(rows_of(vfull), Ufull[usl].astype(dt)).astype(dt)
            continue
        for a, b in pairs:
            acc = acc + np.matmul(rows_of(vp[a]), Up[b][usl].astype(dt)).astype(dt)
    y = acc.reshape(lead + (x.shape[0],) + tuple(n_out) + (kernel.shape[4],))
    y = np.transpose(y, np.argsort(perm))
    for i in tr:
        y = _along(f(ax[i][2]), y, 1 + i)
    return y.astype(dt)


def split_conv(x, kernel, segments, keep=KEEP6, dtype=np.float32, plain_taps=()):
    """A 'same' stride-1 convolution in the split scheme.  `segments` per axis (z, y, x): None = the axis's taps are summed
    directly, a list = Cook-Toom F(m, 3) segments (tools/gen_wino_tables.composite).  `keep`: the piece products, in order.
    Weights are transformed and split in float64, data in `dtype`, accumulation in `dtype`.  With dtype float64 the third piece of
    both operands is the exact remainder, so ALL9 gives the convolution itself.  plain_taps: (dz, dy) taps multiplied unsplit."""
    return _run(x, kernel, segments, "split", keep, dtype, plain_taps)


def plain_conv(x, kernel, segments, dtype=np.float32):
    """The same convolution with unsplit operands: the weights' transform in float64 and ONE rounding to `dtype` (as
    conv_wino_pack_weights stores U for the fp32-input GEMM), the data's transform, every product and the accumulation in `dtype`."""
    return _run(x, kernel, segments, "plain", dtype=dtype)


def natural_unit(x, kernel, segments):
    """u per output: the algorithm of split_conv on absolute values (|B| |x|, |G| |w| |G|^T, |A|) in float64, times 2^-24"""
    return _run(x, kernel, segments, "abs") * 2.0 ** -24


def impulse_frames(shape, cin, n, rng, positions=None):
    """n frames [n, *shape, cin] float32 with one nonzero voxel each, and the list of (position, channel, value) per frame.
    Values are full-mantissa: standard normal times 10^U(-3, 3), both signs.  positions: a list of voxels, cycled (default: every
    voxel of the volume in a random order); channels cycle through a random order, so n >= cin visits them all."""
    shape = tuple(shape)
    if positions is None:
        positions = [tuple(int(k) for k in np.unravel_index(i, shape)) for i in rng.permutation(int(np.prod(shape)))]
    chans = rng.permutation(cin)
    frames = np.zeros((n, *shape, cin), np.float32)
    imp = []
    for i in range(n):
        pos, c = tuple(positions[i % len(positions)]), int(chans[i % cin])
        val = np.float32(rng.standard_normal() * 10.0 ** rng.uniform(-3, 3))
        frames[(i, *pos, c)] = val
        imp.append((pos, c, float(val)))
    return frames, imp


def cancelling_frames(shape, cin, n, rng, positions=None):
    """two impulses of opposite sign at the same voxel in the channels (2 k, 2 k + 1): x and -x (1 + 2^-12).  With weights whose
    rows 2 k and 2 k + 1 are equal (`pair_rows`) the high pieces cancel and the small products carry the output.  Returns the
    frames and, per frame, the LIST of its impulses."""
    frames, imp = impulse_frames(shape, cin // 2, n, rng, positions)
    out = np.zeros((n, *shape, cin), np.float32)
    lists = []
    for i, (pos, k, val) in enumerate(imp):
        other = np.float32(-np.float32(val) * np.float32(1.0 + 2.0 ** -12))
        out[(i, *pos, 2 * k)] = val
        out[(i, *pos, 2 * k + 1)] = other
        lists.append([(pos, 2 * k, val), (pos, 2 * k + 1, float(other))])
    return out, lists


def pair_rows(kernel):
    """a copy of kernel [.., Cin, Cout] whose input-channel rows 2 k + 1 equal rows 2 k"""
    k = kernel.copy()
    n = kernel.shape[3] // 2
    k[:, :, :, 1:2 * n:2] = k[:, :, :, 0:2 * n:2]
    return k


def expected(impulses, kernel, shape):
    """float64 result of the 'same' convolution of impulse frames in closed form: x * w[tap, c, :] at the voxels the impulse
    reaches, 0 elsewhere.  impulses: per frame one (position, channel, value) or a list of them."""
    kd = kernel.shape[:3]
    w = kernel.astype(np.float64)
    out = np.zeros((len(impulses), *shape, kernel.shape[4]), np.float64)
    for i, fr in enumerate(impulses):
        for pos, c, val in ([fr] if isinstance(fr, tuple) else fr):
            for tap in itertools.product(*[range(k) for k in kd]):
                o = tuple(p - t + (k - 1) // 2 for p, t, k in zip(pos, tap, kd))
                if all(0 <= oo < s for oo, s in zip(o, shape)):
                    out[(i, *o)] += np.float64(val) * w[(*tap, c)]
    return out


def in_units(got, exact, unit):
    """(max, rms) of |got - exact| / unit over the outputs with unit > 0, and the largest |got - exact| where unit == 0 (an output
    no product feeds: it has to be exact)"""
    err = np.abs(np.asarray(got, np.float64) - exact)
    live = unit > 0
    e = err[live] / unit[live]
    stray = float(err[~live].max()) if (~live).any() else 0.0
    return (float(e.max()), float(np.sqrt(np.mean(e * e)))), stray


def _around_the_impulses(x, kernel, segments, fn):
    """fn(frames) of sparse frames at the cost of a crop: along every DIRECT axis each frame is cut to a window that holds its
    nonzero voxels and the kernel's reach around them (all frames the same width), fn runs on the windows and its output is put
    back into a volume of zeros.  Exact, not an approximation: what lies outside a window is zero, so the zero padding at the
    window's edge is the data itself, and no product reaches an output outside it."""
    di = [i for i in range(3) if segments[i] is None]
    n = x.shape[0]
    lo = np.zeros((n, 3), np.int64)
    width = [x.shape[1 + i] for i in range(3)]
    nz = [np.nonzero(x[f]) for f in range(n)]
    for i in di:
        r = (kernel.shape[i] - 1) // 2
        ext = [(int(z[i].min()), int(z[i].max())) if len(z[i]) else (0, 0) for z in nz]
        width[i] = min(x.shape[1 + i], max(b - a for a, b in ext) + 1 + 2 * r)
        lo[:, i] = [min(max(a - r, 0), x.shape[1 + i] - width[i]) for a, _ in ext]
    if width == list(x.shape[1:4]):
        return fn(x)
    win = np.stack([x[f, lo[f, 0]:lo[f, 0] + width[0], lo[f, 1]:lo[f, 1] + width[1], lo[f, 2]:lo[f, 2] + width[2]] for f in range(n)])
    yw = fn(win)
    full = [x.shape[1 + i] if i in di else yw.shape[1 + i] for i in range(3)]
    y = np.zeros((n, *full, yw.shape[4]), yw.dtype)
    for f in range(n):
        a = [lo[f, i] if i in di else 0 for i in range(3)]
        y[f, a[0]:a[0] + yw.shape[1], a[1]:a[1] + yw.shape[2], a[2]:a[2] + yw.shape[3]] = yw[f]
    return y


def separation(x, kernel, segments, exact, post=None, unit_post=None, plain_taps=(), drops=SMALL, plain=False):
    """E6: (max, rms) in units of u of the six-piece emulation of the frames x against `exact`; E5: the smallest max and the
    smallest rms over the emulations that lose one product of `drops`; with `plain` also Eplain, the unsplit fp32 form (plain_conv).  post / unit_post: the epilogue applied to the emulator's
    output and to the unit (e.g. a crop and a max-pool: max-pooling is 1-Lipschitz, the pooled unit is the window's largest).
    The emulations run on a crop around each frame's nonzero voxels (_around_the_impulses)."""
    post = post or (lambda y: y)

    def emulate(keep):
        y = _around_the_impulses(x, kernel, segments, lambda w: split_conv(w, kernel, segments, keep, np.float32, plain_taps))
        return post(y.astype(np.float64))
    unit = (unit_post or post)(_around_the_impulses(x, kernel, segments, lambda w: natural_unit(w, kernel, segments)))
    res = {"unit": unit}
    e6, stray = in_units(emulate(KEEP6), exact, unit)
    assert stray == 0.0, stray
    res["E6"] = e6
    if plain:
        y = _around_the_impulses(x, kernel, segments, lambda w: plain_conv(w, kernel, segments))
        res["Eplain"], stray = in_units(post(y.astype(np.float64)), exact, unit)
        assert stray == 0.0, stray
    per = {}
    for d in drops:
        per[d], _ = in_units(emulate(tuple(k for k in KEEP6 if k != d)), exact, unit)
    res["drop"] = per
    res["E5"] = (min(v[0] for v in per.values()), min(v[1] for v in per.values()))
    return res


def bound(sep, correct="E6"):
    """the GPU tests' bound: the geometric mean of "correct" and "one product missing", for max and for rms.  correct: "E6" for the
    split kernels, "Eplain" for the fp32-input GEMM"""
    return (float(np.sqrt(sep[correct][0] * sep["E5"][0])), float(np.sqrt(sep[correct][1] * sep["E5"][1])))


def maxpool2(y):
    """2^3 max-pool, 'valid': [N, D, H, W, C] -> [N, D // 2, H // 2, W // 2, C]"""
    n, d, h, w, c = y.shape
    y = y[:, :d // 2 * 2, :h // 2 * 2, :w // 2 * 2]
    return y.reshape(n, d // 2, 2, h // 2, 2, w // 2, 2, c).max(axis=(2, 4, 6))


# ---- the cases of tests/test_split_products_host.py and tests/test_gpu_split_products.py ---------------------------------------
# One-layer models whose epilogue is the identity where the planner allows it, and otherwise the smallest 1-Lipschitz epilogue
# that makes the planner pick the kernel ("form"):
#   identity   Conv3D (no bias, linear) -> Flatten
#   relu_pool  Conv3D (no bias) -> ReLU -> MaxPool 2^3 -> Flatten: conv_first_b3 serves only a layer whose max-pool stands in
#              front of a monotone chain, and an empty chain does not count as one.  ReLU is exact in fp32
#   pool       Conv3D 5^3 (no bias) -> MaxPool 2^3 -> Flatten: conv_first5 serves only a pooled layer
# The same epilogue is applied in float64 to the exact products; the unit is pooled with max (ReLU and max-pool are 1-Lipschitz).
def _wfs_positions():
    c = [(z, y, x) for z in (0, 9) for y in (0, 9) for x in (0, 9)]                                   # corners: all four (y, x) parities
    e = [(0, 0, 4), (0, 5, 9), (9, 3, 0), (4, 9, 9), (5, 0, 0), (0, 9, 6)]                            # edges
    f = [(0, 4, 5), (9, 5, 4), (3, 0, 6), (6, 9, 3), (2, 7, 0), (7, 2, 9)]                            # faces
    i = [(4, 4, 4), (5, 4, 5), (3, 5, 4), (6, 5, 5)]                                                  # interior, the four parities
    return c + e + f + i


def _b3_positions(xs=(0, 1, 10, 19, 20)):
    # x at the pair boundaries and in the ragged last pair of the odd extent, times corner / face / interior in (z, y)
    zy = [(0, 0), (20, 20), (0, 11), (10, 20), (10, 9)]
    return [(z, y, x) for (z, y) in zy for x in xs][:24]


def _f5_positions():
    # every axis visits both border layers on each side (a 5^3 kernel reaches two voxels), and the interior
    return [(0, 0, 0), (1, 1, 1), (20, 20, 20), (19, 19, 19), (0, 19, 1), (1, 20, 10), (10, 0, 19), (20, 1, 0), (19, 10, 20),
            (10, 10, 10), (2, 18, 1), (18, 1, 2)]


CASES = {
    # name: algorithm, volume, Cin, Cout, frames, frames per predict call, positions (None: a random order of all voxels)
    "wino_32_64": dict(alg="wino", side=5, cin=32, cout=64, n=140, batch=70, positions=None),
    "wino_40_72": dict(alg="wino", side=5, cin=40, cout=72, n=140, batch=70, positions=None),
    # (the narrow GEMM takes layers with Cin >= 128 only: conv_wino_plan)
    "n32_128_20": dict(alg="wino", side=5, cin=128, cout=20, n=40, batch=40, positions=None),
    "n32_160_7": dict(alg="wino", side=5, cin=160, cout=7, n=40, batch=40, positions=None),
    "wfs_16_33": dict(alg="wfs", side=10, cin=16, cout=33, n=24, batch=24, positions=_wfs_positions()),
    "wfs_48_64": dict(alg="wfs", side=10, cin=48, cout=64, n=24, batch=24, positions=_wfs_positions()),
    "b3_6_32": dict(alg="b3", side=21, cin=6, cout=32, n=24, batch=24, positions=_b3_positions()),
    "b3_5_24": dict(alg="b3", side=21, cin=5, cout=24, n=24, batch=24, positions=_b3_positions()),
    "f5_6_16": dict(alg="f5", side=21, cin=6, cout=16, n=12, batch=12, positions=_f5_positions()),
    "f5_3_1": dict(alg="f5", side=21, cin=3, cout=1, n=12, batch=12, positions=_f5_positions()),
}
ALGS = {
    "wino": dict(segments=WINO, k=3, form="identity", plain_taps=()),
    "wfs": dict(segments=WFS, k=3, form="identity", plain_taps=()),
    "b3": dict(segments=FIRST_B3, k=3, form="relu_pool", plain_taps=B3_PLAIN_TAPS),
    "f5": dict(segments=FIRST5, k=5, form="pool", plain_taps=()),
}


def case_model(name, paired=False):
    """(model_config, weights, kernel) of a case; paired: the kernel's input-channel rows 2 k + 1 equal rows 2 k"""
    from timed_hip import synth
    c = CASES[name]
    a = ALGS[c["alg"]]
    b = synth.KerasGraphBuilder((c["side"],) * 3 + (c["cin"],), seed=1000 + 7 * c["cin"] + c["cout"])
    x = b.conv3d(b.input_name, c["cout"], a["k"], padding="same", use_bias=False)
    conv = x
    if a["form"] == "relu_pool":
        x = b.relu(x)
    if a["form"] in ("relu_pool", "pool"):
        x = b.maxpool(x, 2)
    cfg, w = b.finish(b.flatten(x))
    if paired:
        w[conv][0] = pair_rows(w[conv][0])
    return cfg, w, w[conv][0]


def case_post(name):
    """(post, unit_post) of a case's form, on [N, D, H, W, C] arrays"""
    form = ALGS[CASES[name]["alg"]]["form"]
    if form == "identity":
        return (lambda y: y), (lambda u: u)
    if form == "pool":
        return maxpool2, maxpool2
    return (lambda y: np.maximum(maxpool2(y), 0.0)), maxpool2


def case_frames(name, kind="impulse"):
    """(frames, impulses) of a case.  kind: "impulse" one nonzero voxel per frame; "cancel" two of opposite sign in paired
    channels; "u8" (conv_first_b3) uint8 frames with 255 and 254 in two x-adjacent voxels of one channel"""
    c = CASES[name]
    shape = (c["side"],) * 3
    rng = np.random.default_rng(1000 * c["cin"] + 10 * c["cout"] + {"impulse": 0, "cancel": 1, "u8": 2}[kind])
    if kind == "impulse":
        return impulse_frames(shape, c["cin"], c["n"], rng, c["positions"])
    if kind == "cancel":
        return cancelling_frames(shape, c["cin"], c["n"], rng, c["positions"])
    assert kind == "u8" and c["alg"] == "b3"
    pos = _b3_positions(xs=(0, 1, 10, 18, 19))
    frames = np.zeros((c["n"], *shape, c["cin"]), np.uint8)
    imp = []
    for i in range(c["n"]):
        z, y, x = pos[i % len(pos)]
        ch = int(rng.integers(c["cin"])) if i >= c["cin"] else i
        frames[i, z, y, x, ch], frames[i, z, y, x + 1, ch] = 255, 254
        imp.append([((z, y, x), ch, 255.0), ((z, y, x + 1), ch, 254.0)])
    return frames, imp


def case_reference(name, kind="impulse"):
    """everything the CPU knows about a case: frames, model, the float64 expectation behind the case's epilogue, the unit, E6, E5
    and the bound; for the conv_wino cases also Eplain and bound_plain, the fp32-input GEMM's.  E5 is taken over the small products that exist in the frames: all three on impulse frames; on cancelling
    frames m*M and l*H (the two impulses have the same h up to sign — the factor 1 + 2^-12 changes bits below the first piece — so
    h*H, h*M and h*L cancel, and the m and l pieces of the data carry the output); on uint8 frames m*M and h*L (a voxel is one
    bf16 piece, the F(2,3) sum point 255 + 254 two: l = 0 everywhere)."""
    c = CASES[name]
    a = ALGS[c["alg"]]
    cfg, w, kernel = case_model(name, paired=(kind == "cancel"))
    frames, imp = case_frames(name, kind)
    post, unit_post = case_post(name)
    exact = post(expected(imp, kernel, (c["side"],) * 3))
    sep = separation(frames.astype(np.float32), kernel, a["segments"], exact, post, unit_post, a["plain_taps"],
                     drops={"impulse": SMALL, "cancel": ("lH", "mM"), "u8": ("mM", "hL")}[kind], plain=c["alg"] == "wino")
    return dict(cfg=cfg, weights=w, kernel=kernel, frames=frames, impulses=imp, exact=exact, unit=sep["unit"], sep=sep,
                bound=bound(sep), bound_plain=bound(sep, "Eplain") if "Eplain" in sep else None, batch=c["batch"])
