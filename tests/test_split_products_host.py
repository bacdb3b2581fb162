"""The CPU references of the split-operand tests (tests/split_products.py) checked against the oracle and against each other, and
the condition that gives tests/test_gpu_split_products.py its meaning: on the very frames and weights the GPU tests run, the
emulation that loses one small piece product (E5) is at least 8 times as far from float64 as the six-product scheme of
csrc/bf16x3.h (E6), in the worst output and in the rms, both in units of u = 2^-24 sum |a| |U| |v| — and, for the conv_wino cases that
also run on the fp32-input GEMM (TH_WINO_SPLIT=0), at least 8 times as far as the unsplit fp32 form (Eplain).  Established on references
alone: no kernel runs here.  Serves reference predict.py:142; uses the CPU oracle (test infrastructure)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_products as sp  # noqa: E402
from oracle import cnn_oracle  # noqa: E402

# the four algorithms at a small volume: (segments, frames shape, kernel extent)
SMALL = {
    "wino": (sp.WINO, (2, 5, 5, 5, 3), 3),
    "wfs": (sp.WFS, (1, 10, 10, 10, 2), 3),
    "b3": (sp.FIRST_B3, (1, 4, 5, 21, 3), 3),
    "f5": (sp.FIRST5, (1, 6, 7, 8, 2), 5),
}
PLAIN = ("wino_32_64", "wino_40_72")          # the cases tests/test_gpu_split_products.py runs under TH_WINO_SPLIT=0
KINDS = [(name, kind) for name in sp.CASES for kind in ("impulse", "cancel")] + [("b3_6_32", "u8")]


@pytest.mark.parametrize("alg", list(SMALL))
def test_nine_products_in_float64_are_the_convolution(alg):
    """transforms, tap geometry and the bookkeeping of the pieces: with all nine products and the third piece exact the emulator
    IS cnn_oracle.conv3d (a transformed axis computes its segments' outputs: 20 of 21 along x for conv_first_b3)"""
    seg, shape, k = SMALL[alg]
    rng = np.random.default_rng(3)
    x, w = rng.standard_normal(shape), rng.standard_normal((k, k, k, shape[-1], 4))
    want = cnn_oracle.conv3d(x, w, None, 1, 1, "same", np.float64)
    got = sp.split_conv(x, w, seg, sp.ALL9, np.float64, plain_taps=sp.ALGS[alg]["plain_taps"])
    want = want[:, :got.shape[1], :got.shape[2], :got.shape[3]]
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-9
    # six products in float64 miss it by the three dropped ones: ~3 x 2^-24 of the products' sum, not less
    six = sp.split_conv(x, w, seg, sp.KEEP6, np.float64, plain_taps=sp.ALGS[alg]["plain_taps"])
    unit = sp.natural_unit(x, w, seg)
    (mx, _), _ = sp.in_units(six, want, unit)
    assert 1e-3 < mx < 3.0, mx


@pytest.mark.parametrize("alg", list(SMALL))
def test_natural_unit_is_positive_where_a_product_arrives(alg):
    seg, shape, k = SMALL[alg]
    rng = np.random.default_rng(4)
    frames, imp = sp.impulse_frames(shape[1:4], shape[4], 6, rng)
    w = rng.standard_normal((k, k, k, shape[-1], 4)).astype(np.float32)
    unit = sp.natural_unit(frames, w, seg)
    exact = sp.expected(imp, w, shape[1:4])[:, :unit.shape[1], :unit.shape[2], :unit.shape[3]]
    assert (unit >= 0).all() and (unit[exact != 0] > 0).all() and (unit == 0).any()
    # the closed form is the oracle's convolution of the same frames
    want = cnn_oracle.conv3d(frames.astype(np.float64), w.astype(np.float64), None, 1, 1, "same", np.float64)
    assert np.abs(want[:, :unit.shape[1], :unit.shape[2], :unit.shape[3]] - exact).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("seg,side", [(sp.WINO, 5), (sp.WFS, 10)])
def test_in_plane_emulation_agrees_with_the_one_the_logit_gates_use(seg, side):
    """tests/test_winograd_numerics.py::_inplane_split is the same scheme written with other NumPy calls (another fp32 summation
    order): on impulse frames each is within E6 of float64, so they are within 2 E6 of each other — far from the ~100 u of a
    lost product — and with one product removed from this emulator only, they are not"""
    from test_winograd_numerics import _inplane_split
    rng = np.random.default_rng(5)
    frames, imp = sp.impulse_frames((side,) * 3, 8, 16, rng)
    w = (rng.standard_normal((3, 3, 3, 8, 6)) * 0.1).astype(np.float32)
    exact = sp.expected(imp, w, (side,) * 3)
    unit = sp.natural_unit(frames, w, seg)
    other = _inplane_split(frames, w, None, seg[1]).astype(np.float64)
    mine = sp.split_conv(frames, w, seg).astype(np.float64)
    (e_mine, _), _ = sp.in_units(mine, exact, unit)
    (e_other, _), _ = sp.in_units(other, exact, unit)
    (d, _), _ = sp.in_units(mine, other, unit)
    print(f"{side}^3: E6 {e_mine:.2f} u, _inplane_split {e_other:.2f} u, between them {d:.2f} u")
    assert d <= e_mine + e_other
    five = sp.split_conv(frames, w, seg, tuple(k for k in sp.KEEP6 if k != "mM")).astype(np.float64)
    (d5, _), _ = sp.in_units(five, other, unit)
    assert d5 >= 8 * (e_mine + e_other), d5


def test_plain_products_in_float64_are_the_convolution():
    """the unsplit emulation shares transforms and tap geometry with the split one: in float64 it IS cnn_oracle.conv3d, and in
    float32 it is within a few u of it on dense frames (one rounding of U, one per product and per addition)"""
    seg, shape, k = SMALL["wino"]
    rng = np.random.default_rng(6)
    x, w = rng.standard_normal(shape), rng.standard_normal((k, k, k, shape[-1], 4))
    want = cnn_oracle.conv3d(x, w, None, 1, 1, "same", np.float64)
    assert np.abs(sp.plain_conv(x, w, seg, np.float64) - want).max() < 1e-9
    x32, w32 = x.astype(np.float32), w.astype(np.float32)
    want = cnn_oracle.conv3d(x32.astype(np.float64), w32.astype(np.float64), None, 1, 1, "same", np.float64)
    got = sp.plain_conv(x32, w32, seg)
    assert got.dtype == np.float32
    (mx, _), _ = sp.in_units(got, want, sp.natural_unit(x32, w32, seg))
    assert 1e-3 < mx < 4.0, mx


@pytest.mark.parametrize("name,kind", KINDS)
def test_a_lost_product_is_eight_times_the_scheme_s_own_error(name, kind):
    r = sp.case_reference(name, kind)
    e6, e5 = r["sep"]["E6"], r["sep"]["E5"]
    print(f"{name} {kind}: E6 max {e6[0]:.2f} rms {e6[1]:.3f} u   E5 max {e5[0]:.1f} rms {e5[1]:.2f} u   "
          + "  ".join(f"-{k} {v[0]:.1f}/{v[1]:.2f}" for k, v in r["sep"]["drop"].items())
          + f"   bound max {r['bound'][0]:.2f} rms {r['bound'][1]:.3f}")
    assert e5[0] >= 8 * e6[0] and e5[1] >= 8 * e6[1], (e6, e5)
    if name in PLAIN:              # the fp32-input GEMM runs these frames too: its own form is as far from a lost product
        ep, bp = r["sep"]["Eplain"], r["bound_plain"]
        print(f"{name} {kind}: Eplain max {ep[0]:.2f} rms {ep[1]:.3f} u   bound max {bp[0]:.2f} rms {bp[1]:.3f}")
        assert e5[0] >= 8 * ep[0] and e5[1] >= 8 * ep[1], (ep, e5)
        assert bp == (float(np.sqrt(ep[0] * e5[0])), float(np.sqrt(ep[1] * e5[1])))
    # every channel is visited, and the frames are what they claim to be
    frames, imp = r["frames"], r["impulses"]
    per = 1 if kind == "impulse" else 2
    assert all(np.count_nonzero(f) == per for f in frames)
    c = sp.CASES[name]
    if kind == "impulse" and c["n"] >= c["cin"]:
        assert {ch for _, ch, _ in imp} == set(range(c["cin"]))
    if kind == "impulse" and c["n"] >= c["side"] ** 3:
        assert len({pos for pos, _, _ in imp}) == c["side"] ** 3
    assert (r["unit"] >= 0).all() and (r["unit"][r["exact"] != 0] > 0).all()
