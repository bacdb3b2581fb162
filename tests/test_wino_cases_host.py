"""The case table of the Winograd GEMM kernels (tests/wino_cases.py) without a GPU: the tile sizes it computes with are the library's
(th_conv_wino_tiles), every GEMM x scheme cell has its rows, the cells nothing compared with a reference before carry every edge of
the table's lists (WIDE_CIN, WIDE_COUT, NARROW_CIN, NARROW_COUT, FRAMES, prologue, tails, arenas: one row each, so that a deleted row is missed), every condition of the tile arithmetic occurs for every GEMM kernel
it applies to, env_of and markers say the same thing, and UNREACHABLE cites the rule of conv_wino_plan that it claims.
tests/test_gpu_wino_cases.py runs the same rows."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino_cases as wc  # noqa: E402
from timed_hip import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _of(gemm=None, scheme=None):
    return [r for r in wc.ROWS if gemm in (None, r.gemm) and scheme in (None, r.scheme)]


def test_tile_sizes_are_the_library_s(lib):
    assert wc.tiles(lib) == wc.TILES == (64, 128, 32)
    assert lib.th_conv_wino_tiles(None) == _lib.TH_EINVAL and b"th_conv_wino_tiles" in lib.th_last_error()
    header = open(os.path.join(ROOT, "include", "timed_hip.h")).read()
    assert re.search(r"^int th_conv_wino_tiles\(int32_t\* tiles_out\);", header, re.M)
    res, args = _lib.PROTOTYPES["th_conv_wino_tiles"]
    assert res.__name__ == "c_int" and [a.__name__ for a in args] == ["c_void_p"]


def test_every_cell_has_its_rows_within_the_size_limits():
    assert len({r.id for r in wc.ROWS}) == len(wc.ROWS)
    for g in wc.GEMMS:
        for s in wc.SCHEMES:
            rows = _of(g, s)
            assert len(rows) >= 2, (g, s)
            assert any(r.tail == "keep" for r in rows), (g, s)             # a layer tensor against float64 in every cell
    for r in wc.ROWS:
        assert r.gemm in wc.GEMMS and r.scheme in wc.SCHEMES and r.pre in ("none", "bn_relu"), r.id
        assert r.tail in ("keep", "gap", "mid") and r.arena in ("none", "read", "write"), r.id
        assert r.arena == "none" or (r.tail == "keep" and r.pre == "none"), r.id
        assert 1 <= r.n <= 130, r.id
        if r.gemm == "n32":                                                # conv_wino_plan: narrow = split && Cout <= 32 && Cin >= 128
            assert r.cout <= 32 and 128 <= r.cin <= 160, r.id
        else:
            assert r.cin >= 32 and r.cout >= 64 and (r.cin * r.cout <= 136 * 130 or r.cout == 338), r.id
        if r.tail == "mid":                                                # the layer behind it is a Winograd layer of the same plan
            assert r.cout >= 32 and wc.MID_COUT[r.gemm] >= 64 and r.cout * wc.MID_COUT[r.gemm] <= 136 * 130, r.id


@pytest.mark.parametrize("gemm,scheme", wc.FULL)
def test_uncovered_cells_carry_every_edge(gemm, scheme):
    """the cells the suite produced no number from, and the narrow GEMM: every edge of the list, each in a row of its own kind"""
    rows = _of(gemm, scheme)
    narrow = gemm == "n32"
    plain = [r for r in rows if r.arena == "none"]
    for cin in (wc.NARROW_CIN if narrow else wc.WIDE_CIN):
        assert any(r.cin == cin and r.tail == "keep" for r in plain), ("Cin", cin)
    for cout in (wc.NARROW_COUT if narrow else wc.WIDE_COUT):
        assert any(r.cout == cout and r.tail == "keep" for r in plain), ("Cout", cout)
    for n in wc.FRAMES:
        assert any(r.n == n and r.tail == "keep" for r in plain), ("n", n)
    assert any(r.pre == "bn_relu" and r.tail == "keep" for r in plain)
    for tail in ("gap", "mid"):
        assert any(r.tail == tail for r in plain), tail
    for arena in ("read", "write"):
        assert any(r.arena == arena for r in rows), arena
    # one edge that no other row of the cell has, per row: deleting any row of the cell is noticed
    def edges(r):
        return {("cin", r.cin), ("cout", r.cout), ("n", r.n), ("pre", r.pre), ("tail", r.tail), ("arena", r.arena)}
    wanted = {("cin", c) for c in (wc.NARROW_CIN if narrow else wc.WIDE_CIN)} | {("cout", c) for c in (wc.NARROW_COUT if narrow else wc.WIDE_COUT)} | \
             {("n", n) for n in wc.FRAMES} | {("pre", "bn_relu"), ("tail", "gap"), ("tail", "mid"), ("arena", "read"), ("arena", "write")}
    for r in rows:
        others = set().union(*(edges(o) for o in rows if o is not r))
        assert (edges(r) & wanted) - others, f"{r.id} carries no edge of its own"


def test_every_condition_of_the_tile_arithmetic_occurs_for_every_kernel():
    def some(rows, cond, what):
        hit = [r.id for r in rows if cond(r, wc.geometry(r))]
        print(f"{what}: {hit}")
        assert hit, what

    for gemm in wc.GEMMS:
        rows = _of(gemm)
        some(rows, lambda r, g: g.Cinp != r.cin, f"{gemm}: Cinp != Cin")
        for k in (1, 2, 3):
            some(rows, lambda r, g: g.nfb == k, f"{gemm}: {k} row blocks")
        some(rows, lambda r, g: r.n % wc.TILES[0] != 0 and g.nfb > 1, f"{gemm}: a ragged last row block")
        if gemm == "n32":
            for k in (1, 2):
                some(rows, lambda r, g: g.nchunks % 3 == k, f"n32: nchunks % 3 == {k} (the three-chunk loop body)")
            some(rows, lambda r, g: g.nfb32 % 4 == 2 and g.groups > 1, "n32: a last workgroup of two waves")
            some(rows, lambda r, g: g.groups == 1 and g.nfb32 == 2, "n32: a single workgroup of two waves")
            continue
        some(rows, lambda r, g: g.nchunks == 1, f"{gemm}: one chunk")
        some(rows, lambda r, g: g.nchunks == 2, f"{gemm}: two chunks")
        some(rows, lambda r, g: g.nchunks >= 3, f"{gemm}: three chunks or more")
        some(rows, lambda r, g: g.idle_waves > 0, f"{gemm}: a column block with an inactive wave")
        some(rows, lambda r, g: g.ncb == 2 and r.cout - wc.TILES[1] <= 32, f"{gemm}: a second column block with one active wave")
        for k in (1, 2, 3):
            some(rows, lambda r, g: g.ncb == k, f"{gemm}: {k} column blocks")
        # 81 and 49 are odd: the grid is rounded up to 8 workgroups per XCD slot and the last ones get no tile (wino_tile_index)
        some(rows, lambda r, g: g.total % 8 != 0 and g.idle > 0, f"{gemm}: idle workgroups in the XCD deal")
    wide = [r for r in wc.ROWS if r.gemm != "n32"]
    assert sum(wc.geometry(r).total % 8 != 0 for r in wide) >= len(wide) - 2       # nearly every row
    for scheme in wc.SCHEMES:
        some(_of(scheme=scheme), lambda r, g: r.pre == "bn_relu", f"k_wino_in<true, {scheme}>")
        some(_of(scheme=scheme), lambda r, g: r.tail == "mid" and r.cout % wc.TILES[2] != 0, f"k_wino_mid<{scheme}> across padded channel counts")
        some(_of(scheme=scheme), lambda r, g: r.tail == "gap", f"k_wino_out<{scheme}, true>")


def test_env_and_markers_agree():
    for r in wc.ROWS:
        env, m = wc.env_of(r), wc.markers(r)
        assert set(env) == {"TH_WINOGRAD", "TH_WINO_SPLIT", "TH_WINO_B3VAR"}, r.id
        assert env["TH_WINOGRAD"] == {9: "1", 7: "2"}[r.scheme], r.id
        assert m.kernel == {"f32": "[k_wino_gemm]", "b3_16": "[k_wino_gemm_b3]", "b3_32": "[k_wino_gemm_b3]", "n32": "[k_wino_gemm_n32]"}[r.gemm]
        # the handle lists exactly the settings that differ from the defaults (TH_WINOGRAD=1, TH_WINO_SPLIT=1, TH_WINO_B3VAR=2)
        default = {"TH_WINOGRAD": "1", "TH_WINO_SPLIT": "1", "TH_WINO_B3VAR": "2"}
        assert set(m.knobs) == {f"{k}={v}" for k, v in env.items() if v != default[k]}, r.id
        assert set(m.no_knobs) == {k for k, v in env.items() if v == default[k]}, r.id
        assert ("F(5,3)" in m.label) == (r.scheme == 7) and ("F(5,3)" in m.no_label) == (r.scheme == 9), r.id
        assert ("bf16x3" in m.no_label) == (env["TH_WINO_SPLIT"] == "0") == (m.kernel == "[k_wino_gemm]"), r.id
        assert not set(m.label) & set(m.no_label), r.id
        assert (wc.tail_env(r) == {"TH_NO_TAIL_FUSE": "1"}) == (r.tail == "keep"), r.id


def test_unreachable_names_what_conv_wino_plan_refuses():
    """the narrow GEMM under TH_WINO_SPLIT=0: the cited line is the rule, and the line that refuses a layer below 64 columns hangs on
    it (tests/test_gpu_wino_cases.py loads such a layer and finds it on a direct kernel)"""
    assert set(wc.UNREACHABLE) == {("n32", "TH_WINO_SPLIT=0")}
    src = open(os.path.join(ROOT, "timed-design_amd", "csrc", "conv_wino.hip")).read().split("\n")
    for why in wc.UNREACHABLE.values():
        m = re.match(r"csrc/conv_wino\.hip:(\d+): (.*)$", why)
        assert m, why
        line = int(m.group(1))
        assert m.group(2) in src[line - 1], (line, src[line - 1])
        assert any("Cout < 64 && !narrow" in l and "return false" in l for l in src[line:line + 4]), src[line:line + 4]
    assert not any(r.gemm == "n32" and wc.env_of(r)["TH_WINO_SPLIT"] == "0" for r in wc.ROWS)


def test_nets_are_what_the_rows_say():
    """the builder: the convolution under test has the row's widths and reads what the row says; a `mid` row has its second layer"""
    for r in wc.ROWS:
        net = wc.build(r)
        layers = {l["name"]: l for l in net.cfg["config"]["layers"]}
        w = net.weights[net.conv]
        assert w[0].shape == (3, 3, 3, r.cin, r.cout) and w[1].shape == (r.cout,) and w[1].any(), r.id
        src = layers[net.conv]["inbound_nodes"][0][0][0]
        assert (layers[src]["class_name"] == "ReLU") == (r.pre == "bn_relu"), r.id
        assert (net.next_conv is not None) == (r.tail == "mid"), r.id
        if net.next_conv:
            assert net.weights[net.next_conv][0].shape == (3, 3, 3, r.cout, wc.MID_COUT[r.gemm]), r.id
        cats = [l for l in layers.values() if l["class_name"] == "Concatenate"]
        assert len(cats) == {"none": 0, "write": 1, "read": 2}[r.arena], r.id
        if r.arena == "read":                  # the row reads the SECOND input of the first arena
            assert [i[0] for i in cats[0]["inbound_nodes"][0]].index(src) == 1, r.id
        if r.arena != "none":                  # and writes an input of the last one: behind the model input, or in front of a sibling
            assert [i[0] for i in cats[-1]["inbound_nodes"][0]].index(net.layer) == (1 if r.arena == "write" else 0), r.id
        x = wc.frames(r)
        assert x.shape[0] == r.n and x.dtype.name == "float32" and 0.4 < (x == 0).mean() < 0.6, r.id
        c = wc.chunk_for(r.n)
        assert (c is None) == (r.n <= 2) and (c is None or (c < r.n and r.n % c)), r.id
