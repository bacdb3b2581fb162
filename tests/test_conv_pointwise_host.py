"""The pointwise (1x1x1) convolution's dispatch rule, asked through th_conv_pw_pick / th_conv_pw_kernels (host code of
csrc/conv_pointwise.hip, no GPU): the case table of tests/pointwise_cases.py picks every compiled instantiation at least once and
nothing outside the dispatch tables, the boundaries of the rule sit where the kernel tables put them, and the float32 reference of the GEMM
rows stays inside the dot-product bound that tests/test_gpu_conv_pointwise.py holds the kernels to."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_cases as pc  # noqa: E402


def _pick(lib, cin, cout, pool=0, in_cs=0, in_coff=0, out_blk=0, relu_chain=0):
    buf = C.create_string_buffer(64)
    assert lib.th_conv_pw_pick(cin, cout, pool, in_cs, in_coff, out_blk, relu_chain, buf, 64) == 0
    return buf.value.decode()


def _kernels(lib):
    buf = C.create_string_buffer(1 << 14)
    assert lib.th_conv_pw_kernels(buf, 1 << 14) == 0
    return buf.value.decode().split()


def test_case_table_picks_every_compiled_instantiation(lib):
    """79 kernels today: 27 k_conv_pw, 30 plain k_conv_pw2, 10 chunk-blocked, 12 with the "BN -> ReLU" epilogue (6 of them
    chunk-blocked).  A new instantiation without a row in the table fails here, and so does a row that picks nothing."""
    names = _kernels(lib)
    assert len(names) == len(set(names)) == 79, names
    assert sum(n.startswith("k_conv_pw<") for n in names) == 27 and sum(n.startswith("k_conv_pw2<") for n in names) == 52
    assert sum(n.endswith(",1,0>") and n.startswith("k_conv_pw2<") for n in names) == 10
    assert sum(n.endswith(",2>") and n.startswith("k_conv_pw2<") for n in names) == 12
    picked = {}
    for c in pc.CASES:
        picked.setdefault(_pick(lib, *pc.pick_args(c)), []).append(pc.case_id(c))
    assert "" not in picked, picked.get("")
    missing, foreign = sorted(set(names) - set(picked)), sorted(set(picked) - set(names))
    print(f"{len(set(picked) & set(names))} of {len(names)} instantiations covered by {len(pc.CASES)} rows; missing {missing}; outside the tables {foreign}")
    assert not missing and not foreign


def test_case_table_groups_hold_what_the_gpu_tests_expect(lib):
    """the rows of each group select the family the group is named after; every chunk-blocked k_conv_pw2 kernel has a blocked row"""
    for c in pc.CASES:
        k = _pick(lib, *pc.pick_args(c))
        if c.group in ("pw2", "epi2"):
            assert k.startswith("k_conv_pw2<") and k.endswith(",0,2>" if c.group == "epi2" else ",0,0>"), (c, k)
        if c.group == "pw":
            assert k.startswith("k_conv_pw<"), (c, k)
        if c.group == "gemm":
            assert c.pre == c.epi == c.pool == "none" and c.dense and not c.blocked
    gemm = {_pick(lib, *pc.pick_args(c)) for c in pc.CASES if c.group == "gemm"}
    assert len(gemm) == 19 and sum(c.group == "gemm" for c in pc.CASES) == 21      # 10 + 9 (kernel, KMAX, NT), and the 2- and 3-pass shapes
    blk = {_pick(lib, *pc.pick_args(c)) for c in pc.CASES if c.blocked}
    assert {n for n in _kernels(lib) if n.startswith("k_conv_pw2<") and n[:-3].endswith(",1")} <= blk
    assert {"k_conv_pw<16,4,0>", "k_conv_pw<4,1,0>"} <= blk
    # every KMAX class of k_conv_pw2 meets all four prologue copies of its MFMA loop (none, BN -> ReLU, ReLU, generic)
    kinds = {"none": 0, "bn_relu": 1, "relu": 2, "bn_elu": 3, "bn": 3}
    seen = {}
    for c in pc.CASES:
        k = _pick(lib, *pc.pick_args(c))
        if k.startswith("k_conv_pw2<"):
            seen.setdefault(k[len("k_conv_pw2<"):].split(",")[0], set()).add(kinds[c.pre])
    assert seen == {"4": {0, 1, 2, 3}, "8": {0, 1, 2, 3}, "12": {0, 1, 2, 3}, "16": {0, 1, 2, 3}}, seen


def test_boundaries_of_the_dispatch_rule(lib):
    p = lambda *a, **k: _pick(lib, *a, **k)     # noqa: E731
    # K8 = ceil(Cin / 8) slots: 4 up to 32 channels, 8 up to 64, 16 above; Cin % 8 != 0 leaves the pipelined kernel
    assert p(32, 32) == "k_conv_pw2<4,1,0,0,0>" and p(33, 32) == "k_conv_pw<8,1,0>" and p(40, 32) == "k_conv_pw2<8,1,0,0,0>"
    assert p(64, 32) == "k_conv_pw2<8,1,0,0,0>" and p(65, 32) == "k_conv_pw<16,1,0>"
    # 12 slots: 72..96 channels into at most 64
    assert p(72, 64) == "k_conv_pw2<12,2,0,0,0>" and p(96, 64, 2) == "k_conv_pw2<12,2,2,0,0>" and p(96, 32, 1) == "k_conv_pw2<12,1,1,0,0>"
    assert p(96, 65) == "k_conv_pw<16,4,0>" and p(96, 128, 2) == "k_conv_pw<16,4,2>"        # no k_conv_pw2<16,4> and no <12,4>
    assert p(104, 64) == "k_conv_pw2<16,2,0,0,0>" and p(104, 32) == "k_conv_pw2<16,1,0,0,0>"
    assert p(128, 64) == "k_conv_pw2<16,2,0,0,0>" and p(136, 64) == "k_conv_pw<16,2,0>"     # 136: two K passes
    assert p(260, 32) == "k_conv_pw<16,1,0>"                                                # three K passes, one slot in the last
    # the NT steps
    assert [p(32, c) for c in (32, 33, 64, 65)] == ["k_conv_pw2<4,1,0,0,0>", "k_conv_pw2<4,2,0,0,0>", "k_conv_pw2<4,2,0,0,0>", "k_conv_pw2<4,4,0,0,0>"]
    assert [p(30, c, 1) for c in (32, 33, 64, 65, 128)] == ["k_conv_pw<4,1,1>", "k_conv_pw<4,2,1>", "k_conv_pw<4,2,1>", "k_conv_pw<4,4,1>", "k_conv_pw<4,4,1>"]
    assert p(64, 128) == "k_conv_pw2<8,4,0,0,0>" and p(64, 129) == "" and p(3, 129) == ""  # wider layers go to the brick kernel
    assert p(128, 128) == "" and p(136, 65) == "" and p(260, 33) == ""                     # weights past 64 KiB of LDS: refused
    # the input view: a channel slice at an offset, or a voxel stride, that is no multiple of 4 floats runs k_conv_pw (scalar loads)
    assert p(16, 32, in_cs=34, in_coff=18) == "k_conv_pw<4,1,0>" and p(16, 32, in_cs=36, in_coff=20) == "k_conv_pw2<4,1,0,0,0>"
    assert p(16, 32, in_cs=34, in_coff=0) == "k_conv_pw<4,1,0>" and p(16, 32, in_cs=36, in_coff=18) == "k_conv_pw<4,1,0>"
    # chunk-blocked output and the "BN -> ReLU" epilogue: k_conv_pw2 instantiations of their own, where they exist
    assert p(24, 64, out_blk=1, relu_chain=1) == "k_conv_pw2<4,2,0,1,2>" and p(24, 64, out_blk=1) == "k_conv_pw2<4,2,0,1,0>"
    assert p(96, 64, relu_chain=1) == "k_conv_pw2<12,2,0,0,2>" and p(96, 64, 1, relu_chain=1) == "k_conv_pw2<12,2,1,0,0>"   # pooled: generic chain
    assert p(104, 64, relu_chain=1) == "k_conv_pw2<16,2,0,0,0>" and p(32, 100, relu_chain=1) == "k_conv_pw2<4,4,0,0,0>"
    assert p(96, 128, out_blk=1) == "k_conv_pw<16,4,0>" and p(30, 20, out_blk=1, relu_chain=1) == "k_conv_pw<4,1,0>"


def test_float32_gemm_of_the_gemm_rows_stays_inside_the_dot_product_bound():
    """Before the GPU is held to the bound: numpy's float32 GEMM of the same operands is inside it on every row, with room.  Worst
    |got - want64| / bound over the 21 rows: 0.213 (Cin = 3 -> 64: few terms, little slack; 0.007 at Cin = 260)."""
    worst = 0.0
    for c in (c for c in pc.CASES if c.group == "gemm"):
        _, _, frames, w, bias = pc.gemm_operands(c)
        want = frames.reshape(-1, c.cin).astype(np.float64) @ w.astype(np.float64) + bias.astype(np.float64)
        got = (frames.reshape(-1, c.cin) @ w + bias).astype(np.float32)
        ratio = float((np.abs(got - want) / pc.gemm_bound(c, frames, w, bias)).max())
        print(f"{pc.case_id(c)}: float32 numpy / bound = {ratio:.4f}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (c, ratio)
    print(f"worst ratio {worst:.4f}")
    assert worst > 1e-3          # the bound is of the size of the error it bounds, not orders of magnitude above it
