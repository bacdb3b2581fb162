"""Six piece products, not five: the split-operand kernels (the scheme of csrc/bf16x3.h in conv_wino.hip, conv_wfsplit.hip,
conv_first_b3.hip and conv_first5.hip) on frames with ONE nonzero voxel, each output measured in its natural unit
u = 2^-24 sum |a| |U| |v| against the float64 result in closed form (tests/split_products.py).

On the dense frames of the other suites a kernel that loses one of its six products moves its result by 1e-6 of the tensor's
scale: the gates there see that by a small factor when the product is missing everywhere, and not at all when the damage is
confined to one K lane (profiles/split_products.txt).  Here the CPU emulation of the scheme stays within E6 = 1..2 u of float64
on the impulse frames and an emulation that loses one small product is E5 = 70..240 u away
(tests/test_split_products_host.py asserts E5 >= 8 E6 on these very frames); a kernel must stay below sqrt(E6 E5), in its worst
output and in the rms — the geometric midpoint between "correct" and "one product missing", taken from the references, never
from the kernel's own output.  An output that no product reaches, and every output of the all-zero frame, must be exactly 0.

The fp32-input GEMM of conv_wino.hip (k_wino_gemm, TH_WINO_SPLIT=0) runs the same frames: it is the plan the load-time guard retreats
to when the split kernels are off, so it is held to the same side of the same line — below sqrt(Eplain E5), Eplain the CPU emulation
of the unsplit form (U rounded once to float32, one fp32 product per multiply-add, fp32 accumulation: split_products.plain_conv).
Exact zeros there catch stale LDS and stale padding rows of V leaking into real rows.

Every model is one convolution without bias.  Its epilogue ("form", split_products.ALGS):
    k_wino_gemm_b3_16 / _b3_32 / _n32, k_conv_wfs     identity: Conv3D -> Flatten
    k_conv_first_b3                                   Conv3D -> ReLU -> MaxPool 2^3 -> Flatten (the planner gives the kernel only to a
                                                      layer whose max-pool stands in front of a monotone chain; ReLU is exact)
    k_conv_first5                                     Conv3D 5^3 -> MaxPool 2^3 -> Flatten (the kernel serves pooled layers only)
and the same epilogue is applied in float64 to the exact products; ReLU and max-pool are 1-Lipschitz, the unit is pooled with max.

Each case runs its impulse frames (every input channel, and for the 5^3 layers all 125 voxels: 140 frames in two calls of 70, past
the 64-row GEMM block with a ragged last block) and a second set with two impulses of opposite sign, x and -x (1 + 2^-12), at one
voxel in two channels whose weight rows are equal: the high pieces cancel and the small products carry the output.
Serves reference predict.py:142."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_products as sp  # noqa: E402
from timed_hip import engine  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(name, kind):
    """the CPU side of a case, computed once and shared by the tests that need it (left unchanged)"""
    if (name, kind) not in _REF:
        _REF[name, kind] = sp.case_reference(name, kind)
    return _REF[name, kind]


def _worst(got, r, k=4):
    """the outputs furthest off, with the impulse of their frame: which channel, tap and column fail says which piece or lane"""
    err = np.abs(got - r["exact"])
    e = np.where(r["unit"] > 0, err / np.where(r["unit"] > 0, r["unit"], 1.0), np.where(err > 0, np.inf, 0.0))
    out = []
    for flat in np.argsort(e, axis=None)[::-1][:k]:
        idx = tuple(int(i) for i in np.unravel_index(flat, e.shape))
        out.append(f"frame {idx[0]} impulse {r['impulses'][idx[0]]} output (z, y, x, co) {idx[1:]}: {e[idx]:.1f} u "
                   f"(got {got[idx]!r}, exact {r['exact'][idx]!r})")
    return "\n".join(out)


def _check(gpu, monkeypatch, name, kernel, env=(), kinds=("impulse", "cancel"), plain=False):
    """plain: the case runs on unsplit fp32 operands — no "bf16x3" in the label, Eplain in the place of E6"""
    for k, v in env:
        monkeypatch.setenv(k, v)
    for kind in kinds:
        r = _reference(name, kind)
        model = engine.HipFrameModel.from_keras(r["cfg"], r["weights"], device=gpu)
        labels = [s["label"] for s in model.steps()]
        # the layer's steps carry its name; a Winograd layer has its two transform steps besides the GEMM
        conv = [l for l in labels if l.startswith("conv3d: ") and "[k_wino_in]" not in l and "[k_wino_out]" not in l]
        assert len(conv) == 1 and kernel in conv[0] and ("bf16x3" in conv[0]) == (not plain), labels
        knobs, guard = model.knobs(), model.guard()
        assert guard["state"] != 2 and "guard:" not in knobs, (guard, knobs)       # the load-time guard dropped nothing
        for k, v in env:
            assert f"{k}={v}" in knobs, knobs
        if not any(k == "TH_WINO_B3VAR" for k, _ in env):
            assert "TH_WINO_B3VAR" not in knobs, knobs                             # the default: k_wino_gemm_b3_16
        frames, b = r["frames"], r["batch"]
        got = np.concatenate([model.predict(frames[i:i + b]) for i in range(0, len(frames), b)])
        zero = model.predict(np.zeros_like(frames[:1]))
        model.close()
        got = got.reshape(r["exact"].shape).astype(np.float64)
        (mx, rms), stray = sp.in_units(got, r["exact"], r["unit"])
        e6, e5, bound = r["sep"]["Eplain" if plain else "E6"], r["sep"]["E5"], r["bound_plain" if plain else "bound"]
        print(f"\n{name} {kind} {kernel} {dict(env)}: {'Eplain' if plain else 'E6'} max {e6[0]:.2f} rms {e6[1]:.3f}   E5 max {e5[0]:.1f} rms {e5[1]:.2f}   "
              f"bound max {bound[0]:.2f} rms {bound[1]:.3f}   GPU max {mx:.2f} rms {rms:.3f} u   off the impulse's reach {stray:g}")
        assert np.isfinite(got).all()
        assert not zero.any(), "the all-zero frame"
        assert stray == 0.0, _worst(got, r)
        assert mx <= bound[0] and rms <= bound[1], f"max {mx:.2f} > {bound[0]:.2f} or rms {rms:.3f} > {bound[1]:.3f} u\n" + _worst(got, r)


@pytest.mark.parametrize("name", ["wino_32_64", "wino_40_72"])
@pytest.mark.parametrize("var", ["16", "32"])
def test_wino_gemm_b3(gpu, monkeypatch, name, var):
    """k_wino_gemm_b3_16 (the default) and k_wino_gemm_b3_32 (TH_WINO_B3VAR=0): one K chunk (32 -> 64), and Cin 40 padded to 64 with
    a ragged column block (72 of 128) — the padding lanes must contribute nothing.  Form: identity"""
    _check(gpu, monkeypatch, name, "[k_wino_gemm_b3]", env=(("TH_WINO_B3VAR", "0"),) if var == "32" else ())


@pytest.mark.parametrize("name", ["wino_32_64", "wino_40_72"])
def test_wino_gemm_fp32(gpu, monkeypatch, name):
    """k_wino_gemm, the fp32-input GEMM (TH_WINO_SPLIT=0), on the frames of the split kernels: one K chunk, whose last k-slot's weight
    prefetch re-reads its own slot, and Cin 40 padded to 64 with a ragged column block; 140 frames in two calls of 70, so a row block
    of 6 real frames above 58 rows of V that hold whatever the call before left.  Form: identity"""
    _check(gpu, monkeypatch, name, "[k_wino_gemm]", env=(("TH_WINO_SPLIT", "0"),), plain=True)


@pytest.mark.parametrize("name", ["n32_128_20", "n32_160_7"])
def test_wino_gemm_n32(gpu, monkeypatch, name):
    """k_wino_gemm_n32, the narrow GEMM: the planner gives it layers with Cout <= 32 and Cin >= 128 — 128 -> 20 and 160 -> 7,
    40 frames.  Form: identity"""
    _check(gpu, monkeypatch, name, "[k_wino_gemm_n32]")


@pytest.mark.parametrize("name,resident", [("wfs_16_33", None), ("wfs_48_64", None), ("wfs_48_64", "2")])
def test_conv_wfs(gpu, monkeypatch, name, resident):
    """k_conv_wfs at 10^3: one phase with a second column tile of ONE real channel (16 -> 33) and three phases (48 -> 64); positions in
    all four in-tile parities of y and x, on faces, edges and corners; once with two resident workgroups that walk 12 frames each.
    Form: identity"""
    _check(gpu, monkeypatch, name, "k_conv_wfs<", env=(("TH_WF_RESIDENT", resident),) if resident else ())


@pytest.mark.parametrize("name", ["b3_6_32", "b3_5_24"])
def test_conv_first_b3(gpu, monkeypatch, name):
    """k_conv_first_b3 at 21^3 (the only volume it serves), two resident workgroups: x at the pair boundaries and in the ragged last
    pair of the odd extent, every channel, every tap — tap 8 included, which runs on the fp32 matrix pipe.  Form: ReLU + max-pool"""
    _check(gpu, monkeypatch, name, "[k_conv_first_b3]", env=(("TH_WF_RESIDENT", "2"),))


def test_conv_first_b3_uint8_sum_point(gpu, monkeypatch):
    """uint8 frames run the one-piece form of k_conv_first_b3; with 255 and 254 in two x-adjacent voxels the F(2,3) sum point
    d1 + d2 = 509 needs its second piece.  Form: ReLU + max-pool"""
    _check(gpu, monkeypatch, "b3_6_32", "[k_conv_first_b3]", env=(("TH_WF_RESIDENT", "2"),), kinds=("u8",))


@pytest.mark.parametrize("name", ["f5_6_16", "f5_3_1"])
def test_conv_first5(gpu, monkeypatch, name):
    """k_conv_first5: 6 -> 16 and 3 -> 1, positions in the two border layers of every side (a 5^3 kernel reaches two voxels).
    Form: max-pool"""
    _check(gpu, monkeypatch, name, "[k_conv_first5]")
