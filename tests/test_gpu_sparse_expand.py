"""k_sparse_expand (csrc/sparse_frames.hip) off the 21^3 geometry, and th_predict_sparse_async's refusals (csrc/predict.hip).

The reference of every comparison is the input itself: frames that travelled sparse are fetched back from the device and compared
with the frames as BYTES, so no tolerance is involved.  The model is Flatten -> Dense(20) -> Softmax directly on the input: no
first-layer convolution reads the caller's frames, so the runtime keeps the float32 copy of the input node (need_convert) and
th_model_fetch returns it — k_convert_frames and the fetch copy move float32 unchanged, which the dense control of every test
asserts first.  Between two runs the input node and the three ring buffers are overwritten with other frames: what is fetched
was written by the run under test."""
import ctypes as C

import numpy as np
import pytest

from timed_hip import _lib, engine, synth
from test_sparse_frames import _gaussianish, _nasty

# frame shape -> (E, W, words per thread): computed with SparseFrames.from_dense, asserted below so the table cannot drift
SHAPES = {
    (1, 1, 1, 1): (1, 4, 1),                 # four frames share one quad; every store is element-wise
    (1, 1, 1, 3): (3, 4, 1),                 # a frame never fills a quad; head cycles 0, 3, 2, 1
    (3, 3, 3, 1): (27, 4, 1),                # E % 4 = 3, E % 32 = 27: partial last word
    (2, 2, 2, 4): (32, 4, 1),                # exactly one word, three padding words
    (3, 3, 3, 5): (135, 8, 1),               # E % 4 = 3, E % 32 = 7
    (5, 4, 3, 7): (420, 16, 1),              # E % 4 = 0, E % 32 = 4; 240 threads own no word
    (16, 16, 8, 4): (8192, 256, 1),          # every thread owns exactly one word
    (13, 13, 13, 4): (8788, 276, 2),         # two words per thread; threads 138-255 own none
    (21, 21, 21, 5): (46305, 1448, 6),       # the shape of tests/test_sparse_frames.py, now compared as bytes
    (32, 32, 32, 4): (131072, 4096, 16),     # exactly the kernel's LDS limit
}
ODD = (3, 3, 3, 5)                           # the small shape of the further cases: frames start at every offset inside a quad

# -0.0, a NaN with a payload, +inf, -inf, two denormals: bit patterns the transport stores and must hand back untouched
_SPECIALS = np.array([0x80000000, 0x7fc12345, 0x7f800000, 0xff800000, 0x000002ca, 0x80000001], np.uint32)


def _positions(E):
    """element 0, element E - 1, both sides of the first 32-element word boundary and of the last one, where E has them"""
    b = (E - 1) // 32 * 32
    out = []
    for p in (0, E - 1, 31, 32, b - 1, b):
        if 0 <= p < E and p not in out:
            out.append(p)
    return out


def _frames(shape, seed=11):
    """_nasty's six frames (from 8 elements per frame on: it writes eight values) or an empty and a full frame, then a frame whose
    only stored element is element 0, one whose only stored element is element E - 1, and six frames of ~8 % fill in which every
    special value visits every position of _positions(E)"""
    E = int(np.prod(shape))
    if E >= 8:
        base = _nasty(shape, seed + 100).reshape(6, E)
    else:
        base = np.zeros((2, E), np.float32)
        base[1] = np.random.default_rng(seed).standard_normal(E).astype(np.float32)
    own = _gaussianish(8, shape, seed).reshape(8, E)
    own[0] = 0.0
    own[0, 0] = 2.5
    own[1] = 0.0
    own[1, E - 1] = -3.5
    for j in range(6):
        u = own[2 + j].view(np.uint32)
        for i, p in enumerate(_positions(E)):
            u[p] = _SPECIALS[(i + j) % 6]
    return np.concatenate([base, own]).reshape(-1, *shape)


def _model(shape, gpu):
    b = synth.KerasGraphBuilder(shape, seed=7, bias_std=0.1)
    cfg, weights = b.finish(b.softmax(b.dense(b.flatten(b.input_name), 20)))
    return engine.HipFrameModel.from_keras(cfg, weights, device=gpu), b.input_name


def _poison(m, n, shape):
    """other frames, nothing of them +0.0, through the input node and all three ring buffers"""
    junk = np.full((n, *shape), 1.5, np.float32)
    for _ in range(3):
        m.predict(junk)


def _dense_control(m, name, x):
    """frames that travel dense come back from the input node byte for byte; returns their probabilities"""
    want = m.predict(x)
    k = (len(x) - 1) % m.chunk + 1
    assert m.fetch(name, k, x.shape[1:]).tobytes() == x[len(x) - k:].tobytes()
    _poison(m, len(x), x.shape[1:])
    return want


def _sparse_equals(m, name, sf, x, want):
    """the batch `sf` (the frames x in the sparse form): the last piece as the device holds it, the probabilities of all frames"""
    got = m.predict(sf)
    k = (len(x) - 1) % m.chunk + 1
    tail = m.fetch(name, k, x.shape[1:])
    assert tail.tobytes() == x[len(x) - k:].tobytes(), np.flatnonzero(tail.view(np.uint32).ravel() != x[len(x) - k:].view(np.uint32).ravel())[:8]
    assert got.tobytes() == want.tobytes()
    _poison(m, len(x), x.shape[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES), ids=["x".join(map(str, s)) for s in SHAPES])
def test_frames_expanded_on_the_device_are_the_frames(gpu, shape):
    E, W, per = SHAPES[shape]
    x = _frames(shape)
    sf = engine.SparseFrames.from_dense(x)
    assert (int(np.prod(shape)), sf.bits.shape[1], -(-sf.bits.shape[1] // 256)) == (E, W, per)
    stored = np.diff(sf.rank.astype(np.int64))
    assert stored.min() == 0 and stored.max() == E and sf.dense().tobytes() == x.tobytes()
    m, name = _model(shape, gpu)
    want = _dense_control(m, name, x)
    _sparse_equals(m, name, sf, x, want)
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [ODD, (21, 21, 21, 5)], ids=["3x3x3x5", "21x21x21x5"])
def test_pieces_rank_bases_and_wider_bitmaps(gpu, shape):
    """11 frames in pieces of 2 and of 3 (more pieces than ring buffers, a ragged last piece); a slice of a batch, whose ranks do
    not start at 0, in one piece and in several; bitmaps with four more (zero) words per frame than the frame needs"""
    x = _frames(shape)
    x = np.concatenate([x[:8], x[-3:]])
    sf = engine.SparseFrames.from_dense(x)
    m, name = _model(shape, gpu)
    for chunk in (2, 3):
        m.set_chunk(chunk)
        want = _dense_control(m, name, x)
        _sparse_equals(m, name, sf, x, want)
    part = engine.SparseFrames(sf.bits[2:7], sf.rank[2:8], sf.values[int(sf.rank[2]):int(sf.rank[7])], shape)
    assert int(part.rank[0]) > 0 and part.dense().tobytes() == x[2:7].tobytes()
    for chunk in (1024, 2):
        m.set_chunk(chunk)
        want = _dense_control(m, name, x[2:7])
        _sparse_equals(m, name, part, x[2:7], want)
    wide = engine.SparseFrames(np.concatenate([sf.bits, np.zeros((len(x), 4), np.uint32)], axis=1), sf.rank, sf.values, shape)
    assert wide.bits.shape[1] == sf.bits.shape[1] + 4 and wide.dense().tobytes() == x.tobytes()
    for chunk in (1024, 3):
        m.set_chunk(chunk)
        want = _dense_control(m, name, x)
        _sparse_equals(m, name, wide, x, want)
    m.close()


def _piece_bytes(frames, W, stored):
    """device bytes of one piece as th_predict_sparse_async lays it out (bitmaps, ranks and values, each from a 16-byte boundary,
    16 bytes of slack): what the sparse ring must hold"""
    o_rank = (frames * W * 4 + 15) // 16 * 16
    o_val = (o_rank + (frames + 1) * 8 + 15) // 16 * 16
    return o_val + stored * 4 + 16


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [ODD, (21, 21, 21, 5)], ids=["3x3x3x5", "21x21x21x5"])
def test_the_sparse_ring_grows_while_earlier_pieces_are_queued(gpu, shape):
    """one frame per piece, every frame storing so much more than the one before that its piece does not fit the ring the runtime
    sized (with a quarter of headroom) for the one before: the ring is replaced in front of every piece of ONE call, while the
    pieces before it are queued.  From an empty frame to a full one."""
    E, W, _ = SHAPES[shape]
    counts = [0]
    while True:
        nxt = (_piece_bytes(1, W, counts[-1]) * 13 // 10 - _piece_bytes(1, W, 0)) // 4 + 1
        if nxt >= E:
            break
        counts.append(int(nxt))
    if _piece_bytes(1, W, E) * 4 > _piece_bytes(1, W, counts[-1]) * 5:
        counts.append(E)
    need = [_piece_bytes(1, W, c) for c in counts]
    assert len(counts) > 4 and all(4 * b > 5 * a for a, b in zip(need, need[1:]))       # each piece outgrows 1.25 x the last
    rng = np.random.default_rng(31)
    x = np.zeros((len(counts), E), np.float32)
    for i, c in enumerate(counts):
        x[i, rng.permutation(E)[:c]] = rng.uniform(0.5, 1.5, c).astype(np.float32)
    x = x.reshape(-1, *shape)
    sf = engine.SparseFrames.from_dense(x)
    assert np.array_equal(np.diff(sf.rank.astype(np.int64)), counts)
    m, name = _model(shape, gpu)                   # a handle that has not seen a sparse batch: its sparse ring is empty
    m.set_chunk(1)
    got = m.predict(sf)
    assert m.fetch(name, 1, shape).tobytes() == x[-1:].tobytes()
    _poison(m, 1, shape)
    want = _dense_control(m, name, x)
    assert got.tobytes() == want.tobytes()
    _sparse_equals(m, name, sf, x, want)           # and once more through the ring as it has grown
    m.close()


@pytest.mark.gpu
def test_two_sparse_tickets_in_flight_waited_out_of_order(gpu):
    xa = _frames(ODD, 41)
    xb = _frames(ODD, 42)[::-1][:9].copy()
    m, name = _model(ODD, gpu)
    wa, wb = _dense_control(m, name, xa), _dense_control(m, name, xb)
    a = m.predict_async(engine.SparseFrames.from_dense(xa))
    b = m.predict_async(engine.SparseFrames.from_dense(xb))
    gb, ga = b.result(), a.result()
    assert m.fetch(name, len(xb), ODD).tobytes() == xb.tobytes()          # the batch submitted last is the last chunk
    assert ga.tobytes() == wa.tobytes() and gb.tobytes() == wb.tobytes()
    m.close()


@pytest.mark.gpu
def test_frames_over_the_bitmap_word_limit_are_refused_before_anything_is_queued(gpu):
    """(33, 32, 32, 4): 4224 bitmap words per frame, the kernel holds 4096 in LDS.  TH_EINVAL that names the limit, in front of
    the first piece (chunk 2: the refusal used to come from inside the piece loop); the handle, its rings and tickets go on"""
    shape = (33, 32, 32, 4)
    x = _frames(shape)[5:10]
    sf = engine.SparseFrames.from_dense(x)
    assert sf.bits.shape[1] == 4224
    m, name = _model(shape, gpu)
    m.set_chunk(2)
    want = _dense_control(m, name, x)
    lib = _lib.load()
    blob = sf.blob()
    out = np.full((len(x), 20), -7.0, np.float32)
    t = C.c_int(-1)
    for _ in range(5):                             # more refusals than the model has tickets: none was taken
        assert lib.th_predict_sparse_async(m._h, blob.ctypes.data, blob.nbytes, out.ctypes.data, 0, C.byref(t)) == _lib.TH_EINVAL
        assert "4096 words" in lib.th_last_error().decode()
    assert t.value == -1 and np.all(out == -7.0)
    with pytest.raises(_lib.TimedHipError, match="4096 words"):
        m.predict(sf)
    got = m.predict(x)
    assert got.tobytes() == want.tobytes() and m.fetch(name, 1, shape).tobytes() == x[-1:].tobytes()
    m.close()


@pytest.mark.gpu
def test_blobs_whose_bitmaps_and_ranks_disagree_are_refused(gpu):
    """k_sparse_expand reads as many values as a frame's bitmap has bits: a bitmap that disagrees with the rank table, or has
    bits beyond element E, must never reach it.  TH_EINVAL that names the frame; `out` and the ticket untouched; handle usable."""
    shape = ODD
    E, W, _ = SHAPES[shape]
    x = _gaussianish(4, shape, 51, fill=0.3)
    sf = engine.SparseFrames.from_dense(x)
    stored = np.diff(sf.rank.astype(np.int64))
    assert stored[1] != stored[2] and 0 < stored.min() and stored.max() < E
    m, name = _model(shape, gpu)
    lib = _lib.load()
    good = sf.blob().copy()
    o_rank, o_bits, o_val, total = engine.sparse_blob_layout(4, W, sf.n_values)
    out = np.full((4, 20), -7.0, np.float32)
    t = C.c_int(-1)

    def call(buf, nbytes=None):
        buf = np.require(buf, requirements="A")
        assert buf.ctypes.data % 16 == 0
        return lib.th_predict_sparse_async(m._h, buf.ctypes.data, buf.nbytes if nbytes is None else nbytes, out.ctypes.data, 0, C.byref(t))

    def refused(buf, frame=None, nbytes=None):
        assert call(buf, nbytes) == _lib.TH_EINVAL
        assert t.value == -1 and np.all(out == -7.0)
        if frame is not None:
            assert f"frame {frame} " in lib.th_last_error().decode()

    def bits_of(buf, frame):
        return buf[o_bits + frame * W * 4:o_bits + (frame + 1) * W * 4].view(np.uint32)

    def flip(buf, frame, element):
        bits_of(buf, frame)[element // 32] ^= np.uint32(1 << (element % 32))

    mask = x.reshape(4, E).view(np.uint32) != 0
    zero1, set1 = int(np.flatnonzero(~mask[1])[3]), int(np.flatnonzero(mask[1])[3])
    bad = good.copy(); flip(bad, 1, zero1)
    refused(bad, 1)                                                     # one extra bit inside a frame
    bad = good.copy(); flip(bad, 1, set1)
    refused(bad, 1)                                                     # one bit cleared
    bad = good.copy(); flip(bad, 2, E + 9)
    refused(bad, 2)                                                     # a bit in the tail of the last real word (E % 32 = 7)
    bad = good.copy(); flip(bad, 2, E + 9); flip(bad, 2, int(np.flatnonzero(mask[2])[0]))
    refused(bad, 2)                                                     # ... with the frame's count kept right
    bad = good.copy(); flip(bad, 3, 32 * (W - 1) + 5)
    refused(bad, 3)                                                     # a bit in a padding word
    bad = good.copy(); flip(bad, 3, 32 * (W - 1) + 5); flip(bad, 3, int(np.flatnonzero(mask[3])[0]))
    refused(bad, 3)                                                     # ... with the frame's count kept right
    bad = good.copy()
    bad[o_rank:o_rank + 5 * 8].view(np.uint64)[2] = sf.rank[1] + np.uint64(stored[2])
    refused(bad, 1)                                                     # frames 1 and 2 swap their counts, the total is right
    bad = good.copy(); bad[24:32].view(np.uint64)[0] = 2 ** 62
    refused(bad)                                                        # a value count whose byte size wraps
    bad = np.zeros(total + 16, np.uint8); bad[:total] = good
    bad[24:32].view(np.uint64)[0] = sf.n_values + 1
    refused(bad)                                                        # one value too many, the blob long enough
    assert call(good) == _lib.TH_OK and t.value >= 0
    _lib.check(lib.th_predict_wait(m._h, t.value))
    assert out.tobytes() == m.predict(x).tobytes() and m.fetch(name, 4, shape).tobytes() == x.tobytes()
    m.close()
