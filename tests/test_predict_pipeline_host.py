"""predict.py's pipeline without a GPU: load_dataset_and_predict on the 26-frame fixture with a model double that READS ITS INPUT
LATE — predict_async keeps the batch by reference, result() computes from it — so a host buffer that is handed to a later group
before its ticket has completed changes bytes in the output files.  And the page-locked rings of timed_hip.engine against a
recording stand-in for the library's register / unregister calls."""
import os
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

from design_utils import utils as du
from timed_hip import engine

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL, DATA, N_FRAMES = Path(os.path.join(G, "keras_tiny.h5")), os.path.join(G, "frames_tiny.hdf5"), 26
FILES = ("keras_tiny.csv", "keras_tiny.fasta", "keras_tiny.txt", "dataset.fasta", "datasetmap.txt", "encoded_labels.csv")


class Boom(Exception):
    pass


class _Ticket:
    def __init__(self, model, X):
        self.model, self.X = model, X

    def result(self):
        if self.X is not None:
            X, self.X = self.X, None
            s = np.asarray(X, dtype=np.float64).reshape(len(X), -1).sum(axis=1)        # each row from its own frame alone
            rows = np.cos(np.arange(1, 21)[None, :] * s[:, None]) ** 2 + 1e-3
            self.value = (rows / rows.sum(axis=1, keepdims=True)).astype(np.float32)
            with self.model.lock:
                self.model.in_flight -= 1
        return self.value


class LateModel:
    n_classes = 20
    made = []           # every handle the loader made
    calls = []          # (device, rows) per predict_async, in call order
    raise_at = None     # the predict_async call (counted from 1, over all handles) that raises Boom

    def __init__(self, path, device=0):
        self.device, self.in_flight, self.most, self.closed, self.lock = device, 0, 0, 0, threading.Lock()
        LateModel.made.append(self)

    def predict_async(self, X):
        LateModel.calls.append((self.device, len(X)))
        if len(LateModel.calls) == LateModel.raise_at:
            raise Boom("predict_async")
        with self.lock:
            self.in_flight += 1
            self.most = max(self.most, self.in_flight)
        return _Ticket(self, X)

    def close(self):
        self.closed += 1


def _run(out, batch_size, frames_per_call, devices, loaders):
    import predict
    LateModel.made, LateModel.calls = [], []
    out.mkdir()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TIMED_LOADERS", str(loaders))
        return predict.load_dataset_and_predict([MODEL], DATA, batch_size=batch_size, frames_per_call=frames_per_call, devices=devices,
                                                dataset_map_path=out / "datasetmap.txt", path_to_output=out, model_loader=LateModel)


@pytest.fixture(scope="module")
def reference_files(tmp_path_factory):
    out = tmp_path_factory.mktemp("pipeline") / "ref"
    _run(out, 5, 5, None, 1)
    return {fn: (out / fn).read_bytes() for fn in FILES}


@pytest.mark.parametrize("batch_size,frames_per_call,devices,loaders", [
    (3, 7, [0, 1, 2], 2), (26, 1024, None, 1), (1, 1, None, 1), (1, 1, None, 3), (1, 1, [0, 1], 3), (2, 2, None, 2)])
def test_every_grouping_writes_the_same_six_files(reference_files, tmp_path, batch_size, frames_per_call, devices, loaders):
    """whatever the reference batch, the call size, the number of handles and of loader threads: the files of the (5, 5) run, as
    bytes; calls dealt round-robin with the row counts of whole reference batches; never more than 3 tickets per handle"""
    _run(tmp_path / "out", batch_size, frames_per_call, devices, loaders)
    for fn in FILES:
        assert (tmp_path / "out" / fn).read_bytes() == reference_files[fn], fn
    ids = devices or [0]
    per_call = max(1, frames_per_call // batch_size) * batch_size         # (below 1024: no ramp-up groups)
    want = [(ids[k % len(ids)], min(per_call, N_FRAMES - lo)) for k, lo in enumerate(range(0, N_FRAMES, per_call))]
    assert LateModel.calls == want
    assert [m.device for m in LateModel.made] == ids
    assert all(1 <= m.most <= 3 and m.in_flight == 0 and m.closed for m in LateModel.made), [(m.most, m.in_flight) for m in LateModel.made]


def test_host_buffers_go_by_group_order(tmp_path, monkeypatch):
    """26 one-frame groups, three loader threads, one handle: a ring of R = 3 + 1 + 3 = 7 host buffers, and group j fills buffer
    j mod R whichever loader thread got to the reader first"""
    seen = []
    real = du.load_batch

    def spy(dataset_path, rows, **kw):
        X, y = real(dataset_path, rows, **kw)
        seen.append((tuple(str(v) for v in rows[0]), X.ctypes.data))
        return X, y
    monkeypatch.setattr(du, "load_batch", spy)
    res = _run(tmp_path / "out", 1, 1, None, 3)
    group_of = {tuple(str(v) for v in row): j for j, row in enumerate(res[0])}
    assert len(group_of) == N_FRAMES == len(seen)
    addr = dict((group_of[row], a) for row, a in seen)
    R = 7
    assert len({addr[j] for j in range(R)}) == R
    for j in range(N_FRAMES - R):
        assert addr[j + R] == addr[j], (j, "the buffer of group j is the buffer of group j + R")
        assert all(addr[i] != addr[j] for i in range(j + 1, j + R)), (j, "and of none of the groups between them")


@pytest.mark.parametrize("where", ["predict_async", "load_batch", "append_outputs"])
def test_an_error_in_any_stage_surfaces_and_leaves_nothing_behind(tmp_path, monkeypatch, where):
    import predict      # noqa: F401  (the patched functions are looked up through design_utils.utils at call time)
    count = {"load_batch": 0, "append_outputs": 0}

    def failing(name, at):
        real = getattr(du, name)

        def f(*a, **kw):
            count[name] += 1
            if count[name] == at:
                raise Boom(name)
            return real(*a, **kw)
        monkeypatch.setattr(du, name, f)
    if where == "predict_async":
        monkeypatch.setattr(LateModel, "raise_at", 4)
    else:
        failing(where, 4 if where == "load_batch" else 2)
    switch = sys.getswitchinterval()
    with pytest.raises(Boom, match=where):
        _run(tmp_path / "out", 2, 2, None, 1)
    assert sys.getswitchinterval() == switch
    assert not [t.name for t in threading.enumerate() if t.name.startswith(("load_batch", "write_outputs"))]
    assert LateModel.made and all(m.closed for m in LateModel.made)


# ---- the page-locked rings --------------------------------------------------------------------------------------
class _RecordingLib:
    """th_host_register / th_host_unregister of the library, recorded"""

    def __init__(self):
        self.events, self.fail = [], False

    def th_host_register(self, p, nbytes):
        if self.fail:
            return 1
        self.events.append(("register", p.value, int(nbytes)))
        return 0

    def th_host_unregister(self, p):
        self.events.append(("unregister", p.value))
        return 0

    def live(self):
        blocks = []
        for e in self.events:
            if e[0] == "register":
                blocks.append(e[1])
            else:
                blocks.remove(e[1])          # (raises on a block that is not registered)
        return blocks


@pytest.fixture
def host_lib(monkeypatch):
    lib = _RecordingLib()
    monkeypatch.setattr(engine._lib, "load", lambda: lib)
    return lib


def test_staging_ring_slots(host_lib):
    ring = engine.StagingRing(2, 4, (3, 3, 3, 1), np.float32, threads=2)
    rng = np.random.default_rng(0)
    rows = rng.random((3, 3, 3, 3, 1), dtype=np.float32)
    got, slot = ring.stage(rows)
    assert slot is not None and np.array_equal(got, rows) and got.shape == rows.shape and got.dtype == rows.dtype
    assert np.shares_memory(got, ring._arrays[slot]) and not np.shares_memory(got, rows)
    assert host_lib.events[0][:2] == ("register", ring._arrays[slot].ctypes.data) and host_lib.events[0][2] >= 4 * 27 * 4
    for other in (rng.random((5, 3, 3, 3, 1), dtype=np.float32), rows.astype(np.float64), rows[:0]):
        back, none = ring.stage(other)
        assert back is other and none is None
    got2, slot2 = ring.stage(rows[:1] + 1)
    assert slot2 not in (None, slot) and np.array_equal(got, rows), "the second batch went into the first one's slot"
    ring.release(slot)                       # (a third stage without it would wait for a slot)
    got3, slot3 = ring.stage(rows[1:])
    assert slot3 == slot and np.array_equal(got3, rows[1:]) and np.array_equal(got2, rows[:1] + 1)
    assert ring.enabled and sum(ring._pinned) == 2 and len(host_lib.events) == 2, "a slot is registered once, on its first fill"
    registered = host_lib.live()
    ring.close()
    assert sorted(e[1] for e in host_lib.events[2:]) == sorted(registered) and not host_lib.live() and not ring.enabled
    assert all(e[0] == "unregister" for e in host_lib.events[2:])


def test_staging_ring_switches_itself_off_when_registration_fails(host_lib):
    host_lib.fail = True
    ring = engine.StagingRing(2, 4, (3, 3, 3, 1), np.float32, threads=2)
    rows = np.ones((3, 3, 3, 3, 1), np.float32)
    for _ in range(3):                       # the slot went back: the third call does not wait for one
        got, slot = ring.stage(rows)
        assert got is rows and slot is None and not ring.enabled
    assert ring._free.qsize() == 2 and not any(ring._pinned)
    ring.close()
    assert host_lib.events == []


def test_blob_ring_grows_a_slot(host_lib):
    ring = engine.BlobRing(2, 2)
    rng = np.random.default_rng(1)
    # (odd frame counts: the rank table then ends on a 16-byte boundary and a blob has no padding bytes, which nobody writes)
    small = [engine.SparseFrames.from_dense(rng.random((3, 3, 3, 3, 1), dtype=np.float32) * (rng.random((3, 3, 3, 3, 1)) < 0.5))
             for _ in range(2)]
    big = engine.SparseFrames.from_dense(rng.random((9, 7, 7, 7, 5), dtype=np.float32) * (rng.random((9, 7, 7, 7, 5)) < 0.7))
    slots = []
    for X in small:
        got, slot = ring.stage(X)
        assert slot is not None and got.blob().tobytes() == X.blob().tobytes() and np.shares_memory(got.blob(), ring._arrays[slot])
        assert got.shape == X.shape and np.array_equal(got.dense(), X.dense())
        slots.append(slot)
    assert sorted(slots) == [0, 1] and [e[0] for e in host_lib.events] == ["register"] * 2
    first_block = ring._arrays[slots[0]].ctypes.data
    assert big.blob_bytes > ring._arrays[slots[0]].nbytes
    for slot in slots:
        ring.release(slot)
    got, slot = ring.stage(big)
    assert slot == slots[0] and got.blob().tobytes() == big.blob().tobytes()
    assert host_lib.events[2] == ("unregister", first_block), "the old block is unregistered before the new one is registered"
    assert host_lib.events[3][:2] == ("register", ring._arrays[slot].ctypes.data) and host_lib.events[3][2] >= big.blob_bytes
    assert len(host_lib.events) == 4
    empty, none = ring.stage(engine.SparseFrames.from_dense(np.zeros((0, 3, 3, 3, 1), np.float32)))
    assert none is None
    live = host_lib.live()
    assert len(live) == 2
    ring.close()
    assert sorted(e[1] for e in host_lib.events[4:]) == sorted(live) and not host_lib.live() and not ring.enabled
