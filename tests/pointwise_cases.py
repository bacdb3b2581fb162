"""The case table of the pointwise (1x1x1) convolution kernels, shared by tests/test_conv_pointwise_host.py (no GPU: every compiled
instantiation is picked by a row) and tests/test_gpu_conv_pointwise.py (every row against the float64 oracle).

conv_pointwise.hip dispatches on
  * K8 = ceil(Cin / 8): KMAX 4 (Cin <= 32), 8 (<= 64), 16 (more; several K passes above 128), and the 12-slot k_conv_pw2 for
    Cin 72..96 with Cout <= 64;
  * NT = 1 / 2 / 4 tiles of 32 output channels (Cout <= 32 / <= 64 / <= 128);
  * the fused 2x2x2 pool (none, max, avg);
  * k_conv_pw2 (software pipeline, buffer addressing) when Cin % 8 == 0, one K pass, a 16-byte aligned view and an instantiation
    exists (none for KMAX 16 x NT 4), else k_conv_pw;
  * chunk-blocked output (BLK, in front of conv_wfused) and the straight-line "BN -> ReLU" epilogue (EPI = 2: unpooled,
    Cout <= 64, Cin <= 96), both k_conv_pw2 only.
A row says what the net around the convolution looks like; which kernel that selects is asked of th_conv_pw_pick, never restated."""
from collections import namedtuple

import numpy as np

# group: which part of the table the row belongs to (and which GPU tests take it)
#   pw2 / epi2 / pw : one row per instantiation, prologues and epilogues rotating
#   gemm            : no prologue, epilogue or pool, dense frames: the GEMM core alone (also held to the dot-product bound)
#   blk             : chunk-blocked output, 10^3 volume, a 3x3x3 'same' convolution (conv_wfused) behind the layer
#   view            : the layers of the concat-buffer net of test_gpu_conv_pointwise.py: in_cs / coff are the input view's voxel stride and channel offset
# pre: none | bn_relu | relu | bn_elu | bn          epi: none | relu | elu_bn | bn_relu | leaky | elu
# dense: frames are dense normals (else half the values are exact zeros)
Case = namedtuple("Case", "group cin cout pool pre epi blocked coff in_cs dense")

POOLS = ("none", "max", "avg")
PRES = ("none", "bn_relu", "relu", "bn_elu", "bn")          # the last two both take the generic copy of the MFMA loop
PW2_PRES = ("none", "bn_relu", "relu", "bn_elu", "none", "bn_relu", "relu", "bn")
EPIS = ("none", "relu", "elu_bn", "bn_relu", "leaky")
COUTS = ((7, 32), (33, 64), (65, 128))                      # NT 1, 2, 4: both ends of each class


def _has_relu_epilogue_kernel(cin, cout):
    return cin % 8 == 0 and cin <= 96 and cout <= 64


def _table():
    rows = []
    state = {"epi": 0}

    def add(group, cin, cout, pool="none", pre="none", epi="none", blocked=False, coff=0, in_cs=0):
        rows.append(Case(group, cin, cout, pool, pre, epi, blocked, coff, in_cs, len(rows) % 2 == 0))

    def next_epi(plain_pw2, cin, cout, pool):
        # the rows of the plain k_conv_pw2 kernels must not carry the chain that selects the EPI = 2 kernel instead
        while True:
            e = EPIS[state["epi"] % len(EPIS)]
            state["epi"] += 1
            if not (plain_pw2 and e == "bn_relu" and pool == "none" and _has_relu_epilogue_kernel(cin, cout)):
                return e

    # ---- k_conv_pw2, plain: 30 kernels.  The two Cin and the two Cout of a class alternate across the pools --------------------
    for cins, ntis in (((8, 32), (0, 1, 2)), ((40, 64), (0, 1, 2)), ((72, 96), (0, 1)), ((104, 128), (0, 1))):
        k = 0                                                # the prologue rotates per KMAX class: each sees all four copies of its loop
        for nti in ntis:
            for p, pool in enumerate(POOLS):
                cin, cout = cins[(p + nti) % 2], COUTS[nti][p % 2]
                add("pw2", cin, cout, pool, PW2_PRES[k % 8], next_epi(True, cin, cout, pool))
                k += 1
    # ---- k_conv_pw2 with the "BN -> ReLU" epilogue (EPI = 2), channels-last: 6 kernels ------------------------------------------
    for i, (cin, cout) in enumerate(((8, 7), (32, 64), (40, 32), (64, 33), (72, 32), (96, 64))):
        add("epi2", cin, cout, "none", PRES[i % 4], "bn_relu")
    # ---- k_conv_pw: 27 kernels.  Cin = 3: every vector short of 4 channels; Cin % 8 != 0 throughout ----------------------------
    for cins in ((3, 30), (36, 61), (68, 100)):
        k = 0
        for nti in (0, 1, 2):
            for p, pool in enumerate(POOLS):
                cin, cout = cins[(p + nti) % 2], COUTS[nti][p % 2]
                add("pw", cin, cout, pool, PRES[k % 5], next_epi(False, cin, cout, pool))
                k += 1
    # the hole of k_conv_pw2's table (KMAX 16 x NT 4), two K passes (NT <= 2 fits in LDS), three K passes with one slot in the last (NT 1)
    for p, pool in enumerate(POOLS):
        add("pw", 96, 128, pool, PRES[p + 1], next_epi(False, 96, 128, pool))
        add("pw", 136, (20, 64, 48)[p], pool, PRES[p], next_epi(False, 136, 64, pool))
        add("pw", 260, (20, 32, 7)[p], pool, PRES[(p + 2) % 4], next_epi(False, 260, 32, pool))
    # ---- the GEMM core alone: one row per (kernel, KMAX, NT), and the multi-pass shapes: 21 rows --------------------------------
    for cin, cout in ((32, 32), (8, 64), (32, 128), (64, 7), (40, 33), (64, 65), (96, 32), (72, 64), (128, 32), (104, 64),          # k_conv_pw2
                      (30, 32), (3, 64), (30, 128), (61, 7), (36, 33), (61, 65), (100, 32), (68, 64), (100, 128), (136, 64), (260, 32)):
        rows.append(Case("gemm", cin, cout, "none", "none", "none", False, 0, 0, True))
    # ---- chunk-blocked output: the 10 generic-chain BLK kernels, the 6 EPI = 2 BLK kernels, k_conv_pw's own out_blk branch --------
    i = 0
    for cin in (8, 40, 72, 104):
        for cout in (20, 48, 100):
            if cin >= 72 and cout == 100:
                continue                                     # no k_conv_pw2 for 12 or 16 slots x 4 tiles: k_conv_pw, covered below
            add("blk", cin, cout, "none", PRES[i % 4], ("elu", "none")[i % 2], blocked=True)
            i += 1
    for i, (cin, cout) in enumerate(((8, 20), (8, 48), (40, 20), (40, 48), (72, 20), (72, 48))):
        add("blk", cin, cout, "none", "bn_relu", "bn_relu", blocked=True)
    add("blk", 96, 128, "none", "bn_relu", "elu", blocked=True)      # k_conv_pw<16,4,0>, 49 920 bytes of weights in LDS: the widest blocked layer
    add("blk", 30, 20, "none", "none", "none", blocked=True)         # Cin % 8 != 0: k_conv_pw<4,1,0>
    # ---- the concat-buffer net, unpooled and max-pooled readers -------------------------------------------------
    for pool in ("none", "max"):
        add("view", 8, 18, "none", in_cs=8)                          # writes channels 0..17 of the 34-channel buffer
        add("view", 8, 16, "none", in_cs=8)                          # writes channels 18..33: out_coff % 4 != 0 on k_conv_pw2's b32 stores
        add("view", 16, 40, pool, "bn_relu", "none", coff=18, in_cs=34)   # reads the 16-channel slice at offset 18: Cin % 8 == 0, scalar loads
        add("view", 34, 24, pool, "bn_relu", "none", coff=0, in_cs=34)    # reads the whole buffer: Cin % 4 != 0
    return rows


CASES = _table()


def pick_args(c):
    """the arguments of th_conv_pw_pick for a row: Cin, Cout, pool, in_cs, in_coff, out_blk, relu_chain"""
    return (c.cin, c.cout, POOLS.index(c.pool), c.in_cs, c.coff, int(c.blocked), int(c.epi == "bn_relu"))


def case_id(c):
    return f"{c.group}-{c.cin}to{c.cout}-{c.pool}-{c.pre}-{c.epi}" + ("-blk" if c.blocked else "") + (f"-off{c.coff}" if c.coff else "")


def gemm_operands(c, n=5, volume=(3, 2, 3)):
    """frames, weights [Cin, Cout] and bias of a 'gemm' row as the GPU test builds them (the same builder seed gives the same net)"""
    from timed_hip import synth
    b = synth.KerasGraphBuilder((*volume, c.cin), seed=1000 + c.cin * 131 + c.cout, bias_std=0.3)
    cfg, weights = b.finish(b.flatten(b.conv3d(b.input_name, c.cout, 1, padding="same")))
    frames = np.random.default_rng(c.cin * 7 + c.cout).standard_normal((n, *volume, c.cin)).astype(np.float32)
    w, bias = weights["conv3d"]
    return cfg, weights, frames, w.reshape(c.cin, c.cout), bias


def gemm_bound(c, frames, w, bias):
    """2 (Cin + 2) 2^-24 (sum_i |x_i| |w_io| + |b_o|) per output element: the forward bound of a length-Cin float32 dot product plus
    bias in ANY summation order (gamma_n <= n u (1 + o(1)), one more rounding for the bias, one for the store), times 2 for not
    knowing whether the matrix pipe fuses its multiply-adds"""
    x = np.abs(frames.reshape(-1, c.cin).astype(np.float64))
    return 2.0 * (c.cin + 2) * 2.0 ** -24 * (x @ np.abs(w.astype(np.float64)) + np.abs(bias.astype(np.float64)))
