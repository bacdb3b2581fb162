"""The planner's rule for the two brick kernels, asked through th_conv_brick_pick / th_conv_brick_kernels (host code of
csrc/planner.hip, conv_mfma.hip and conv_n16.hip, no GPU): every row of tests/brick_cases.py gets the instantiation and the brick it is
in the table for, the rows reach every compiled instantiation and nothing outside the tables, and every staging mode that only
the plan arithmetic selects occurs in a row.  tests/test_gpu_conv_brick.py runs the same rows."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brick_cases as bc  # noqa: E402


def _plans(lib):
    return [(r, bc.parse(bc.pick(lib, r), r)) for r in bc.ROWS]


def _args(name):
    return [int(v) for v in name[name.index("<") + 1:-1].split(",")]


def _writes_behind_another_concat_input(r):
    """the row's net as it is built: the convolution's chain ends as an input of a Concatenate, and not as its first"""
    cfg, _, cur = bc.build(r, 0)
    layers = cfg["config"]["layers"]
    while True:
        readers = [l for l in layers if l["inbound_nodes"] and cur in [i[0] for i in l["inbound_nodes"][0]]]
        if len(readers) != 1:
            return False
        if readers[0]["class_name"] == "Concatenate":
            return [i[0] for i in readers[0]["inbound_nodes"][0]].index(cur) > 0
        cur = readers[0]["name"]


def test_every_row_gets_its_instantiation_and_brick(lib):
    assert len({r.id for r in bc.ROWS}) == len(bc.ROWS)
    bad = []
    for r in bc.ROWS:
        label = bc.pick(lib, r)
        print(f"{r.id}: {label}")
        if not label:
            bad.append((r.id, "neither kernel plans the layer"))
            continue
        p = bc.parse(label, r)
        if (p.kernels, p.FB, p.ZB, p.nzb) != (r.kernel, r.FB, r.ZB, r.nzb):
            bad.append((r.id, label, r.kernel, r.FB, r.ZB, r.nzb))
        # the table's own limits: small volumes, small batches that still end on a ragged group
        voxels, ch = r.vol[0] * r.vol[1] * r.vol[2], max(r.cin, bc.FRONT_CH if r.front != "input" else 0)
        assert voxels * ch <= 21 ** 3 * 8 or (voxels <= 19 * 14 * 14 and ch <= 40), r.id
        assert 3 <= r.n <= 2 * r.FB + 3, r.id
        assert set(r.env) <= {"TH_WINOGRAD", "TH_WFUSED", "TH_CONV_GL", "TH_N16_RESIDENT"}, r.id
    assert not bad, bad


def test_rows_and_unreachable_cover_the_kernel_tables_exactly(lib):
    """48 instantiations today: 11 tile configurations x 3 pool modes + 4 compile-time geometries of k_conv_mfma, 7 + 4 of k_conv_n16"""
    names = bc.kernels(lib)
    assert len(names) == len(set(names)) == 48, names
    assert sum(n.startswith("k_conv_mfma<") for n in names) == 37 and sum(n.startswith("k_conv_n16<") for n in names) == 11
    assert sum(_args(n)[-1] != 0 for n in names) == 8                  # the geometry variants
    assert not any(n.startswith("k_conv_n16<") and _args(n)[3] == 4 and _args(n)[2] != 0 for n in names)   # side channels: no pooled kernel
    picked = {}
    for r, p in _plans(lib):
        for k in p.kernels:
            picked.setdefault(k, []).append(r.id)
    assert len(bc.UNREACHABLE) <= 3 and not set(bc.UNREACHABLE) & set(picked), (bc.UNREACHABLE, picked)
    have = set(picked) | set(bc.UNREACHABLE)
    missing, foreign = sorted(set(names) - have), sorted(have - set(names))
    print(f"{len(set(picked))} of {len(names)} instantiations reached by {len(bc.ROWS)} rows; missing {missing}; outside the tables {foreign}")
    assert not missing and not foreign


def test_boundaries_of_the_rule(lib):
    """where a layer changes kernel, and what neither kernel plans"""
    base = next(r for r in bc.ROWS if r.id == "n16-w4-cout9")._replace(vol=(4, 4, 4), cin=24, cout=16)

    def k(**kw):
        r = base._replace(**kw)
        label = bc.pick(lib, r)
        return bc.parse(label, r).kernels if label else ()

    assert k() == ("k_conv_n16<4,4,0,0,0>",) and k(cout=17) == k(cout=20) == ("k_conv_n16<4,4,0,4,0>",)
    assert k(cout=21) == ("k_conv_mfma<4,2,1,1,16,2,0,0>",)
    # the side-channel kernel does not pool: a pooled 17..20-channel layer stays on k_conv_mfma with its pool
    assert k(cout=16, pool="max") == ("k_conv_n16<4,4,1,0,0>",) and k(cout=20, pool="max") == ("k_conv_mfma<4,2,1,1,16,2,1,0>",)
    # k_conv_n16 wants more than 8 input channels, a 3x3x3 kernel and stride 1
    assert k(cin=9) == ("k_conv_n16<4,4,0,0,0>",) and k(cin=8) == ("k_conv_mfma<8,1,1,1,8,1,0,0>",)
    assert k(k=(3, 3, 1))[0].startswith("k_conv_mfma<") and k(stride=2)[0].startswith("k_conv_mfma<")
    # 8-channel chunks up to 64 output channels, then the 16-channel configurations
    assert k(cin=8, cout=64) == ("k_conv_mfma<8,2,2,2,8,1,0,0>",) and k(cin=8, cout=65) == ("k_conv_mfma<4,4,2,4,16,2,0,0>",)
    # a strided convolution does not pool, a pooled layer needs two planes per axis, and nothing here dilates
    assert k(stride=2, pool="max") == () and k(vol=(1, 4, 4), pool="avg") == () and k(vol=(1, 4, 4)) != ()
    buf = bc.C.create_string_buffer(512)
    three = (bc.C.c_int * 3)
    assert lib.th_conv_brick_pick(4, 4, 4, 24, 16, 3, 3, 3, three(1, 1, 1), three(2, 2, 2), 1, 0, 0, 0, buf, 512) == 0 and buf.value == b""
    assert lib.th_conv_brick_pick(4, 4, 4, 24, 16, 3, 3, 3, three(1, 1, 1), three(1, 1, 1), 1, 3, 0, 0, buf, 512) != 0      # no such pool mode
    assert lib.th_conv_brick_pick(4, 4, 4, 24, 16, 3, 3, 3, three(1, 1, 1), three(1, 1, 1), 1, 0, 0, 0, buf, 8) != 0        # buffer too small
    assert lib.th_conv_brick_pick(2, 2, 2, 24, 16, 3, 3, 3, three(1, 1, 1), three(1, 1, 1), 0, 0, 0, 0, buf, 512) == 0 and buf.value == b""   # 'valid': no output


def test_staging_geometry_view_and_n16_cases_are_present(lib):
    """each case is computed from the pick's label and the row's shape, not from a flag of the row"""
    plans = _plans(lib)
    mf = [(r, p) for r, p in plans if p.kernels[0].startswith("k_conv_mfma<")]
    n16 = [(r, p) for r, p in plans if p.kernels[0].startswith("k_conv_n16<")]
    assert len(mf) + len(n16) == len(bc.ROWS)
    k3 = lambda r: bc._triple(r.k)        # noqa: E731
    s3 = lambda r: bc._triple(r.stride)   # noqa: E731
    has_bn = lambda r: r.epi in ("elu_bn", "bn_relu", "bn_neg")   # noqa: E731
    geo = lambda p: _args(p.kernels[0])[-1]   # noqa: E731

    def some(rows, cond, what):
        hit = [r.id for r, p in rows if cond(r, p)]
        print(f"{what}: {hit}")
        assert hit, what

    # ---- staging modes of k_conv_mfma ----
    some(mf, lambda r, p: p.nzb > 1 and r.pool == "none" and p.Dc % p.ZB != 0, "z-bricks, unpooled, ragged last brick")
    some(mf, lambda r, p: p.nzb > 1 and r.pool == "max" and r.vol[0] % 2 == 1 and p.Dc == r.vol[0] - 1, "z-bricks, max pool, odd depth")
    some(mf, lambda r, p: p.nzb > 1 and r.pool == "avg", "z-bricks, average pool")
    some(mf, lambda r, p: p.nzb > 1 and s3(r) == (2, 2, 2), "z-bricks, stride 2")
    some(mf, lambda r, p: p.nzb > 1 and p.nnb > 1, "z-bricks and several Cout blocks")
    some(mf, lambda r, p: p.FB > 1 and r.n % p.FB != 0, "several frames per workgroup, ragged last group")
    some(mf, lambda r, p: p.FB == 16, "16 frames per workgroup")
    some(mf, lambda r, p: p.nchunks >= 3 and r.cin % _args(p.kernels[0])[4] != 0, "three Cin chunks, the last ragged")
    some(mf, lambda r, p: r.cout % 32 != 0 and has_bn(r), "Cout % 32 != 0 under a per-channel BatchNorm epilogue")
    some(mf, lambda r, p: not r.bias, "no bias")
    # ---- geometry and views ----
    some(mf, lambda r, p: r.pre == "bn_relu" and r.padding == "same" and max(k3(r)) > 1, "BN -> ReLU prologue over a zero halo")
    some(mf, lambda r, p: r.padding == "valid", "'valid' padding")
    some(mf, lambda r, p: r.padding == "same" and any(k % 2 == 0 for k in k3(r)), "even kernel, asymmetric 'same'")
    some(mf, lambda r, p: len(set(k3(r))) > 1, "anisotropic kernel")
    some(mf, lambda r, p: s3(r) == (3, 3, 3), "stride 3")
    some(mf, lambda r, p: r.front == "slice" and bc.in_view(r)[1] % 4 != 0 and bc.in_view(r)[0] > r.cin, "input: a slice of a concat arena at an offset that is no multiple of 4")
    some(mf, lambda r, p: _writes_behind_another_concat_input(r), "output at a channel offset into an arena")
    # geo_compact (launch_conv_mfma): a geometry kernel, 'same', the whole frame in one brick, 16-byte aligned full chunks
    compact = lambda r, p: geo(p) == r.vol[1] + 2 == r.vol[2] + 2 and r.padding == "same" and p.nzb == 1 and bc.in_view(r)[0] % 4 == 0 and bc.in_view(r)[1] % 4 == 0   # noqa: E731
    some(mf, lambda r, p: compact(r, p) and r.cin % 16 == 0, "geo_compact")
    cvols = {r.vol for r, p in mf if compact(r, p) and r.cin % 16 == 0}
    some(mf, lambda r, p: compact(r, p) and r.cin % 16 != 0 and r.vol in cvols, "the geo_compact geometry with Cin % 16 != 0")
    # ---- k_conv_n16 ----
    na = lambda p: _args(p.kernels[0])    # noqa: E731
    some(n16, lambda r, p: na(p)[:3] == [8, 8, 1], "8 waves, max pool")
    some(n16, lambda r, p: na(p)[:3] == [8, 8, 2], "8 waves, average pool")
    some(n16, lambda r, p: na(p) == [4, 4, 2, 0, 0], "<4,4,2>")
    some(n16, lambda r, p: na(p) == [8, 8, 0, 0, 0] and r.vol[1] != r.vol[2], "<8,8,0> at Hp != Wp")
    # three resident workgroups: ceil(units / 3) trips each; a ragged last group
    some(n16, lambda r, p: na(p)[0] == 8 and r.env.get("TH_N16_RESIDENT") == "3" and -(-r.n // p.FB) > 3 and r.n % p.FB != 0, "8 waves, several trips per workgroup")
    for cout in (1, 9, 16):
        some(n16, lambda r, p: r.cout == cout and na(p)[3] == 0, f"Cout {cout}")
    for cout in (17, 20):
        some(n16, lambda r, p: r.cout == cout and na(p)[3] == 4, f"side channels, Cout {cout}")
