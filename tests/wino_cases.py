"""The case table of the Winograd GEMM kernels of the 5^3 layers (csrc/conv_wino.hip), shared by tests/test_wino_cases_host.py (no GPU:
every GEMM x scheme cell has its rows, every edge of the tile arithmetic occurs for every kernel it applies to) and
tests/test_gpu_wino_cases.py (every row, under its environment, against the float64 oracle).  Test infrastructure, not collected.

A row is one 3x3x3 'same' convolution Cin -> Cout at 5^3 with bias, n frames, and the net around it:

    gemm    f32    k_wino_gemm          TH_WINO_SPLIT=0     fp32-input MFMA, the first plan the load-time guard retreats to
            b3_16  k_wino_gemm_b3_16    the default         split operands, 16x16x32 MFMA
            b3_32  k_wino_gemm_b3_32    TH_WINO_B3VAR=0     split operands, 32x32x16 MFMA
            n32    k_wino_gemm_n32      the default         the narrow split GEMM: Cout <= 32 and Cin >= 128
    scheme  9 (TH_WINOGRAD=1: F(3,3)+F(2,3), 81 positions per plane) | 7 (TH_WINOGRAD=2: F(5,3), 49 positions)
    pre     none | bn_relu                                  the BN -> ReLU prologue of k_wino_in<true, P>
    tail    keep   Conv -> ELU -> BN -> GAP -> Softmax with TH_NO_TAIL_FUSE=1: the layer's tensor exists and is fetched
            gap    the same net with the tail fused: the pooling output transform, "wino_out + global_avg_pool"
            mid    Conv -> ELU -> BN -> Conv (Cout -> MID_COUT[gemm]) -> ELU -> BN -> GAP -> Softmax: a second Winograd layer
                   behind the row's, reached through k_wino_mid
    arena   none | write: the row reads the model input and writes its tensor behind it into a concat arena (voxel stride
            Cin + Cout, first channel Cin) | read: two 1x1x1 convolutions write channels 0..31 and 32.. of an arena, the row reads the
            second slice (voxel stride 32 + Cin, first channel 32) and writes into a second arena — strided views on both sides of the
            transform kernels, as in tests/test_gpu_wino.py::test_winograd_layers_on_concat_arenas.  Arena rows keep their tensor.

Which block, chunk and ragged edge a shape reaches follows from the three tile sizes; they are asked of th_conv_wino_tiles and held
to TILES, so a changed tile fails the host test instead of silently hollowing the table."""
import ctypes as C
from collections import namedtuple

import numpy as np

Row = namedtuple("Row", "id cin cout n gemm scheme pre tail arena")

TILES = (64, 128, 32)                 # kNF frames per row block, kCB columns per column block, kKC channels per chunk
GEMMS = ("f32", "b3_16", "b3_32", "n32")
SCHEMES = (9, 7)
KERNEL = {"f32": "[k_wino_gemm]", "b3_16": "[k_wino_gemm_b3]", "b3_32": "[k_wino_gemm_b3]", "n32": "[k_wino_gemm_n32]"}
FRONT_CH = 5                          # channels of the model input in front of an `arena == "read"` row
SLICE_OFF = 32                        # channels of the first slice of the arena such a row reads
MID_COUT = {"f32": 64, "b3_16": 130, "b3_32": 64, "n32": 64}      # width of the second layer of a `mid` row
# the cells whose kernels no test compared with a reference before this table (and the narrow GEMM): they get every edge
FULL = [(g, s) for g in ("f32", "n32") for s in SCHEMES] + [("b3_32", 7)]
# combinations conv_wino_plan refuses, with the rule (file:line): a narrow layer needs split operands, so under TH_WINO_SPLIT=0 a
# Cout <= 32 layer is no Winograd layer at all and k_wino_gemm_n32 never runs fp32 products
UNREACHABLE = {("n32", "TH_WINO_SPLIT=0"): "csrc/conv_wino.hip:919: const bool narrow = split && Cout <= 32 && Cin >= 128"}

# the edges, one reason each
WIDE_CIN = (32, 40, 96)               # one chunk (the last k-slot's prefetch re-reads its own slot) | padded to 64 | three chunks
WIDE_COUT = (64, 72, 128, 130, 338)   # waves 2, 3 idle | ragged | full block | a second block of one wave, two columns | the head: 3 blocks
NARROW_CIN = (128, 160, 136)          # 4 and 5 chunks against the three-chunk loop body | 136 padded to 160
NARROW_COUT = (1, 20, 32)
FRAMES = (1, 63, 64, 65, 130)         # around the 64-frame row block; three row blocks (narrow: Ns = 192, a ragged last workgroup)


def _rows():
    R = []

    def add(gemm, scheme, cin, cout, n, pre="none", tail="keep", arena="none"):
        rid = f"{gemm}-s{scheme}-{cin}to{cout}-n{n}" + ("" if pre == "none" else "-" + pre) + ("" if tail == "keep" else "-" + tail) + \
              ("" if arena == "none" else "-" + arena)
        R.append(Row(rid, cin, cout, n, gemm, scheme, pre, tail, arena))

    def wide_full(gemm, scheme):       # every row carries an edge no other row of its cell has
        add(gemm, scheme, 32, 64, 1)
        add(gemm, scheme, 40, 72, 63, pre="bn_relu")
        add(gemm, scheme, 96, 128, 64)
        add(gemm, scheme, 64, 130, 65)
        add(gemm, scheme, 32, 338, 130)
        add(gemm, scheme, 40, 72, 5, tail="gap")
        add(gemm, scheme, 32, 72, 65, tail="mid")             # 72 -> 96 channels of the next layer's V: k_wino_mid writes the padding
        add(gemm, scheme, 32, 64, 9, arena="write")
        add(gemm, scheme, 40, 72, 9, arena="read")

    def narrow_full(scheme):
        add("n32", scheme, 128, 20, 1)
        add("n32", scheme, 160, 1, 63)
        add("n32", scheme, 136, 32, 64, pre="bn_relu")
        add("n32", scheme, 128, 32, 65)
        add("n32", scheme, 160, 20, 130)
        add("n32", scheme, 136, 20, 5, tail="gap")
        add("n32", scheme, 128, 32, 9, tail="mid")            # 32 -> 64 behind it: the narrow GEMM's M through k_wino_mid
        add("n32", scheme, 128, 20, 9, arena="write")
        add("n32", scheme, 128, 7, 9, arena="read")

    for scheme in SCHEMES:
        wide_full("f32", scheme)
    # k_wino_gemm_b3_16, covered elsewhere: two rows per scheme, chosen so that the kernel still sees every chunk count, column-block
    # and row-block count here; scheme 7 takes the two transform instantiations nothing ran: k_wino_in<true, 7> and k_wino_mid<7>
    # across padded channel counts (40 -> 72 -> 130: V rows 64 and 96 wide)
    add("b3_16", 9, 32, 338, 130)
    add("b3_16", 9, 40, 130, 65, tail="gap")
    add("b3_16", 7, 96, 72, 5, pre="bn_relu")
    add("b3_16", 7, 40, 72, 66, tail="mid")
    add("b3_32", 9, 96, 130, 65)
    add("b3_32", 9, 40, 72, 5, pre="bn_relu")
    wide_full("b3_32", 7)
    for scheme in SCHEMES:
        narrow_full(scheme)
    return R


ROWS = _rows()


def row_id(r):
    return r.id


def cell(r):
    return (r.gemm, r.scheme)


def tiles(lib):
    """(kNF, kCB, kKC) as the library reports them"""
    t = (C.c_int32 * 3)()
    assert lib.th_conv_wino_tiles(t) == 0, lib.th_last_error()
    return tuple(t)


Geometry = namedtuple("Geometry", "Cinp nchunks Coutp ncb Ns nfb npos total per_xcd idle idle_waves nfb32 groups")


def geometry(r, t=TILES):
    """what launch_wino_gemm makes of a row: padded widths, blocks, workgroups, the workgroups of the rounded-up grid that get no tile
    (wino_tile_index) and the waves whose 32 columns are all padding (WinoTile::active); for the narrow GEMM the 32-frame blocks and
    the workgroups per position"""
    nf, cb, kc = t
    narrow = r.gemm == "n32"
    cinp = -(-r.cin // kc) * kc
    coutp = 32 if narrow else -(-r.cout // cb) * cb
    ncb = 1 if narrow else coutp // cb
    ns = -(-r.n // nf) * nf
    nfb, npos = ns // nf, r.scheme * r.scheme
    total = npos * nfb * ncb
    per_xcd = -(-total // 8)
    idle_waves = 0 if narrow else sum(1 for b in range(ncb) for w in range(cb // 32) if b * cb + w * 32 >= r.cout)
    nfb32 = ns // 32
    return Geometry(cinp, cinp // kc, coutp, ncb, ns, nfb, npos, total, per_xcd, per_xcd * 8 - total, idle_waves, nfb32, -(-nfb32 // 4))


def env_of(r):
    """the TH_WINOGRAD, TH_WINO_SPLIT and TH_WINO_B3VAR settings of the row (all three, defaults included: a row does not inherit them)"""
    return {"TH_WINOGRAD": "1" if r.scheme == 9 else "2", "TH_WINO_SPLIT": "0" if r.gemm == "f32" else "1",
            "TH_WINO_B3VAR": "0" if r.gemm == "b3_32" else "2"}


def tail_env(r):
    """a row whose tensor is fetched keeps its tail unfused"""
    return {"TH_NO_TAIL_FUSE": "1"} if r.tail == "keep" else {}


Markers = namedtuple("Markers", "kernel label no_label knobs no_knobs")


def markers(r):
    """what the plan label of the row's GEMM step and model.knobs() must show: the bracketed kernel name, strings the label carries
    and must not carry, knob settings the handle lists (only a setting that differs from the default is listed) and knob names it
    must not list"""
    label, no_label = [], []
    (label if r.scheme == 7 else no_label).append("F(5,3)")
    (no_label if r.scheme == 7 else label).append("F(3,3)+F(2,3)")
    (no_label if r.gemm == "f32" else label).append("bf16x3")
    label.append("gemm 32f x 32c" if r.gemm == "n32" else f"gemm {TILES[0]}f x {TILES[1]}c")
    g = geometry(r)
    label.append(f"K{g.Cinp}" + (f" ({r.cin} real)" if g.Cinp != r.cin else ""))
    knobs, no_knobs = [], []
    (knobs if r.scheme == 7 else no_knobs).append("TH_WINOGRAD=2" if r.scheme == 7 else "TH_WINOGRAD")
    (knobs if r.gemm == "f32" else no_knobs).append("TH_WINO_SPLIT=0" if r.gemm == "f32" else "TH_WINO_SPLIT")
    (knobs if r.gemm == "b3_32" else no_knobs).append("TH_WINO_B3VAR=0" if r.gemm == "b3_32" else "TH_WINO_B3VAR")
    return Markers(KERNEL[r.gemm], tuple(label), tuple(no_label), tuple(knobs), tuple(no_knobs))


Net = namedtuple("Net", "cfg weights conv layer next_conv")


def build(r, seed=None):
    """the row's net: (cfg, weights, name of the convolution under test, name of the tensor behind its Conv -> ELU -> BN block, name
    of the second convolution of a `mid` row or None)"""
    from timed_hip import synth
    seed = 700 + ROWS.index(r) if seed is None else seed
    b = synth.KerasGraphBuilder((5, 5, 5, FRONT_CH if r.arena == "read" else r.cin), seed=seed, bias_std=0.2)
    x = src = b.input_name
    cat = None
    if r.arena == "read":
        p = b.conv3d(x, SLICE_OFF, 1, padding="same")
        x = b.conv3d(x, r.cin, 1, padding="same")
        cat = b.concat([p, x])
    if r.pre == "bn_relu":
        x = b.relu(b.batchnorm(x))
    conv = b.conv3d(x, r.cout, 3, padding="same")
    layer = x = b.batchnorm(b.elu(conv))
    nxt = None
    if r.tail == "mid":
        nxt = b.conv3d(x, MID_COUT[r.gemm], 3, padding="same")
        x = b.batchnorm(b.elu(nxt))
    if r.arena == "write":
        x = b.conv3d(b.concat([src, x]), 20, 1, padding="same")
    elif r.arena == "read":
        x = b.conv3d(b.concat([x, b.conv3d(cat, 8, 1, padding="same")]), 20, 1, padding="same")
    cfg, weights = b.finish(b.softmax(b.gap(x)))
    return Net(cfg, weights, conv, layer, nxt)


def frames(r, seed=None):
    """n frames, half of the values exact zeros"""
    rng = np.random.default_rng(1700 + ROWS.index(r) if seed is None else seed)
    shape = (r.n, 5, 5, 5, FRONT_CH if r.arena == "read" else r.cin)
    return (rng.standard_normal(shape) * (rng.random(shape) < 0.5)).astype(np.float32)


def chunk_for(n):
    """a chunk size c < n that does not divide n, or None (n <= 2): the largest of a few that cut the batch inside a 64-frame row
    block and leave a ragged last launch"""
    return next((c for c in (64, 63, 32, 7, 3, 2) if c < n and n % c), None)


# per-element (relative to max(1, max|y|)), rms and probability bounds of tests/test_gpu_wino.py: LAYER / 3e-6 / TIGHT for the default
# scheme, 1e-4 / 1.5e-5 / FAST for F(5,3), whose transforms carry entries up to 16
BOUNDS = {9: (1e-5, 3e-6, 5e-6), 7: (1e-4, 1.5e-5, 2e-5)}
