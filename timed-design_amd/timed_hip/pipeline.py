"""predict.py's pipeline over GPU calls (no reference counterpart: reference predict.py:125-155 loads, predicts and writes one
batch after the other).  ``row_groups`` cuts the dataset map into calls, a ``GroupLoader`` builds the batch of a call from
whichever source the dataset offers, ``run_groups`` overlaps loading, the GPU and the writer.  ``_RowsOnDevice`` / ``_ToDevice`` let a
sharded run (predict._predict_sharded) leave its probability rows in device memory for the gather."""
import os
import sys
import threading
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from contextlib import contextmanager
from functools import partial

import numpy as np

from design_utils import utils as du
from . import _lib, engine, framepack


def call_spans(lo, n_rows, per_call):
    """[a, b) ranges of ``per_call`` rows from ``lo`` up to ``n_rows`` (the last one ragged)"""
    return [(a, min(a + per_call, n_rows)) for a in range(lo, n_rows, per_call)]


def row_groups(n_rows, batch_size, start_batch, frames_per_call):
    """[lo, hi) row ranges, each a whole number of reference batches (so resuming at ``start_batch`` lines up)"""
    per_call = max(1, int(frames_per_call) // max(1, batch_size)) * batch_size
    first = start_batch * batch_size
    groups, lo = [], first
    # a run of several large calls starts with a quarter- and a half-size one: the GPU gets its first frames after a quarter of
    # a group's load time instead of a whole one (the first load and the last forward pass are the two stages nothing overlaps)
    ramp = [per_call // 4, per_call // 2] if per_call >= 1024 and n_rows - first > per_call else []
    for size in ramp:
        size = size // batch_size * batch_size
        if size >= batch_size and lo + size < n_rows:
            groups.append((lo, lo + size))
            lo += size
    return groups + call_spans(lo, n_rows, per_call)


def _models_take_sparse(models) -> bool:
    """every model of the round-robin is a HIP engine handle (or the sharded wrapper around one): only those read SparseFrames"""
    for m in models:
        inner = getattr(m, "sparse_ok", None)
        if inner is None:
            inner = hasattr(m, "_predict_async_sparse")
        if not inner:
            return False
    return True


class GroupLoader:
    """``load(k)`` builds the batch of call group k: (frames, labels, release) — ``release`` gives a page-locked staging slot
    back once the prediction that read it has completed (None: nothing was staged).  Any loader thread may call it.  Sources,
    in this order: a sparse pack's SparseFrames, a structure set's DeviceFrames (voxelised in HBM), the GPU inflater's DeviceFrames,
    the host reader's ndarray / mapped rows."""

    def __init__(self, models, dataset_path, flat_dataset_map, groups, gpu_decode=False):
        self.models, self.dataset_path, self.flat_dataset_map, self.groups = models, dataset_path, flat_dataset_map, groups
        # a folder of structures (or one structure with a property channel): the frames of a group are built in HBM
        self.structure_set = None if framepack.is_pack(dataset_path) else du.structure_set_of(dataset_path)
        plain_h5 = not framepack.is_pack(dataset_path) and not framepack.is_structure(dataset_path) and self.structure_set is None
        on_device = getattr(models[0], "device", None) is not None
        self._frames_born_on_device = self.structure_set is not None and all(getattr(m, "takes_device_frames", False) for m in models)
        # a float32 pack with sparse transport files (framepack.sparsify): the loader hands out SparseFrames batches — a tenth of the
        # bytes cross PCIe, the device rebuilds the dense frames (th_predict_sparse_async).  TIMED_SPARSE=0: the dense rows as before
        self.sparse_pack = None
        if framepack.is_pack(dataset_path) and os.environ.get("TIMED_SPARSE", "1") != "0" and on_device:
            fp = du._frame_pack(dataset_path)
            if fp.sparse is not None and _models_take_sparse(models):
                self.sparse_pack = fp
        # gzip .hdf5: until load_batch_device first declines (an unsupported file, TH_ENOMEM); then the host reader serves the rest
        self.decode_on_gpu = bool(gpu_decode) and plain_h5
        # Loader threads: two on GPU-inflated datasets, one elsewhere.  Two: the host part of batch g+2 (object headers, B-trees,
        # descriptors, ~6 ms of Python per 4096 frames) and its pageable upload run while the inflate kernels of batch g+1 hold the
        # decoder's scratch set.  Measured on 40 k gzip float64 frames (tools/trace_predict_e2e.py): the loop takes 0.229 s with one
        # loader, 0.178 s with two — 17.8 ms per 4096 frames, which is the inflate kernels (8 ms) plus the CNN (10.3 ms) one after
        # the other on the GPU — and 0.19 s with three.  (When the CNN took twice as long the second loader bought nothing.)  One
        # loader elsewhere: the host reader fills its buffers under a lock anyway, and frame packs hand out mapped rows.
        self.loaders = max(1, int(os.environ.get("TIMED_LOADERS", "2" if self.decode_on_gpu else "1")))
        self.seconds = 0.0                     # spent in load(), over all loader threads

        # Batches of an .hdf5 dataset are built in a small ring of reused buffers: a fresh 0.2-0.5 GB NumPy batch costs more
        # in first-touch page faults than its inflation does.  The first full-size batch of every slot simply becomes its buffer
        # (no extra allocation); a buffer is reused only after the ticket that read it has completed: at most 3 groups per model
        # are outstanding (run_groups) + the one waiting to be submitted + the ones being loaded.  The ring is sized for ALL
        # loaders: when the device decode falls back to the host reader mid-run, every loader fills host buffers.  Slots go by
        # GROUP order (the k-th full-size group takes slot k mod ring size), not by the order in which loader threads get the
        # lock, which can invert and would hand a group the buffer of one whose ticket is still outstanding.  Only full-size
        # groups take slots: the smaller ramp-up groups in front and the ragged last one get buffers of their own.
        # Pageable memory on purpose: host->device copies from it already run at the PCIe rate here, and page-locking 1 GB costs
        # more than a short run takes (th_host_alloc exists for callers that keep their buffers).  Frame packs hand out
        # memory-mapped rows instead.
        ring_size = 3 * len(models) + 1 + self.loaders
        self.max_rows = max((hi - lo for lo, hi in groups), default=0)
        self._host_slot = {}
        if len(groups) > ring_size and plain_h5:
            full = [k for k, (lo, hi) in enumerate(groups) if hi - lo == self.max_rows]
            self._host_slot = {k: i % ring_size for i, k in enumerate(full)}
        self._host_buffers = {}                # slot -> the first full-size batch that was loaded for it
        self._host_lock = threading.Lock()     # the host reader's buffers are filled by one loader at a time

        # Memory-mapped rows of a frame pack go through a ring of page-locked buffers (engine.StagingRing; sparse batches:
        # engine.BlobRing): the copy to the device then runs at the PCIe rate instead of the rate at which the driver pins pages it
        # has never seen.  3 groups per model outstanding + the one waiting to be submitted + the one being filled.
        # TIMED_STAGING=0 hands out the mapped rows as before.
        self._staging_slots = 3 * len(models) + 2
        self._stage_dense = on_device
        self._rings = {}                       # "dense" / "sparse" -> the ring of this run, None once it is off

    def load(self, k):
        t0 = time.perf_counter()
        try:
            X, y = self._rows(k)
            X, release = self._stage(X)
            return X, y, release
        finally:
            self.seconds += time.perf_counter() - t0

    def _rows(self, k):
        lo, hi = self.groups[k]
        rows = self.flat_dataset_map[lo:hi]
        if self.sparse_pack is not None:
            span = self.sparse_pack.contiguous_rows(rows)
            if span is not None:
                return self.sparse_pack.sparse_batch(*span), self.sparse_pack.labels[span[0]:span[1]].astype(float)
        if self._frames_born_on_device:
            # ONE th_voxelise_batch call on the GPU that will predict the group: the atoms of the structures these rows touch go
            # up, the frames are written into a pooled device buffer and never cross PCIe.  The call waits for its own stream only
            return self.structure_set.device_batch(rows, self.models[k % len(self.models)].device, du._DEVICE_POOL)
        if self.decode_on_gpu:
            # the chunks of this group are inflated ON the GPU that will predict it (th_h5_decode_device) — the frames never
            # exist on the host; a dataset that cannot take the path (other filters, a layout h5lite does not read ...) says so once
            got = du.load_batch_device(self.dataset_path, rows, device=self.models[k % len(self.models)].device)
            if got is not None:
                return got
            self.decode_on_gpu = False
        with self._host_lock:
            slot = self._host_slot.get(k)
            # float32 frames: the rounding Keras applies to load_batch's float64 anyway, done while the chunks are placed
            X, y = du.load_batch(self.dataset_path, rows, dtype=np.float32, out=self._host_buffers.get(slot))
            if (slot is not None and slot not in self._host_buffers and isinstance(X, np.ndarray) and X.base is None
                    and len(X) == self.max_rows):
                self._host_buffers[slot] = X
            return X, y

    def _stage(self, X):
        if isinstance(X, engine.SparseFrames):
            # a sparse batch (views of the memory-mapped transport files) is assembled into ONE page-locked blob: rank table, bitmaps, values
            ring = self._ring("sparse", 1, lambda threads: engine.BlobRing(self._staging_slots, threads))
        elif isinstance(X, np.memmap) and self._stage_dense:
            ring = self._ring("dense", 0, lambda threads: du.take_staging_ring(self._staging_slots, self.max_rows, X.shape[1:], X.dtype, threads)
                              if threads >= 2 and len(self.groups) > 2 else None)
        else:
            return X, None
        if ring is None:
            return X, None
        X, slot = ring.stage(X)
        return X, (None if slot is None else partial(ring.release, slot))

    def _ring(self, kind, least_threads, make):
        """the staging ring of one kind, made when the first batch asks for it; whatever goes wrong then: off for this run"""
        if kind not in self._rings:
            self._rings[kind] = None
            try:
                cpus = int(_lib.load().th_host_cpus())
                ranks_here = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1))          # one process per GPU shares the host's cores
                threads = int(os.environ.get("TIMED_STAGING_THREADS", str(max(least_threads, min(8, (cpus - 2) // ranks_here)))))
                if os.environ.get("TIMED_STAGING", "1") != "0":
                    self._rings[kind] = make(threads)
            except Exception:
                pass
        return self._rings[kind]

    def close(self, completed, pending):
        """``pending``: (ticket, ...) of what was submitted and not consumed (after an error)."""
        rings = {kind: ring for kind, ring in self._rings.items() if ring is not None}
        if rings and not completed:
            for ticket, *_rest in pending:           # nothing may still be copying out of a slot
                try:
                    ticket.result()
                except Exception:
                    pass
        if "dense" in rings:
            if completed:
                du.give_back_staging_ring(rings["dense"])    # kept for the next call; du.release_device_memory() (the CLI, at its end) closes it
            else:
                rings["dense"].close()
        if "sparse" in rings:
            rings["sparse"].close()
        self._rings = {}
        self._host_buffers = {}


class _Laps(dict):
    """seconds per named part of the pipeline, for TIMED_PIPELINE_TRACE"""

    @contextmanager
    def lap(self, name):
        t0 = time.perf_counter()
        try:
            yield
        finally:
            self[name] = self.get(name, 0.0) + time.perf_counter() - t0


def run_groups(models, loader, consume):
    """Pipeline over the call groups, three stages on three threads:
         loader thread(s)  ``loader.load(k)``: load_batch of group g+1 (reference utils.py:487-530)
         this thread       th_predict_async of group g, round-robin over ``models`` (the host->device copy of pageable
                           frames blocks here while the kernels of group g-1 run)
         writer thread     ``consume(probs, labels)`` for group g-1, strictly in group order (formats and appends)
    An exception in any stage surfaces here."""
    n_groups, loaders = len(loader.groups), loader.loaders
    if not n_groups:
        return
    depth = 2 * len(models)
    laps = _Laps()

    def finish(ticket, labels, release):
        with laps.lap("result"):
            probs = ticket.result()
            if release is not None:
                release()
        with laps.lap("consume"):
            consume(probs, labels)

    pending = deque()          # tickets submitted to a GPU, oldest first
    writing = deque()          # futures of the writer thread, oldest first
    # three Python threads share the interpreter lock; with the default 5 ms switch interval the submitter can sit behind
    # the writer for longer than a whole group takes on the GPU (4.6 ms per 1024 frames)
    switch = sys.getswitchinterval()
    sys.setswitchinterval(2e-4)
    completed = False
    try:
        with ThreadPoolExecutor(max_workers=loaders, thread_name_prefix="load_batch") as pool, \
                ThreadPoolExecutor(max_workers=1, thread_name_prefix="write_outputs") as writer:
            ahead = deque(pool.submit(loader.load, j) for j in range(min(loaders, n_groups)))     # groups being loaded, in order
            for k in range(n_groups):
                with laps.lap("loader"):
                    X, y, release = ahead.popleft().result()
                    if k + loaders < n_groups:
                        ahead.append(pool.submit(loader.load, k + loaders))
                # a model has 4 tickets (th_predict_async): at most 3 consecutive groups per model are outstanding here,
                # 2 on the GPU queue and 1 with the writer
                with laps.lap("writer"):
                    while len(pending) + len(writing) >= 3 * len(models):
                        if not writing:
                            writing.append(writer.submit(finish, *pending.popleft()))
                        writing.popleft().result()
                with laps.lap("submit"):
                    pending.append((models[k % len(models)].predict_async(X), y, release))
                    del X
                if len(pending) >= depth:
                    writing.append(writer.submit(finish, *pending.popleft()))
            while pending:
                writing.append(writer.submit(finish, *pending.popleft()))
            while writing:
                writing.popleft().result()
        completed = True
    finally:
        sys.setswitchinterval(switch)
        loader.close(completed, pending)
    if os.environ.get("TIMED_PIPELINE_TRACE"):
        print(f"[pipeline] {n_groups} groups: waiting for the loader {laps['loader']:.3f} s, for the writer/GPU {laps['writer']:.3f} s, "
              f"submitting (incl. pageable host->device copies) {laps['submit']:.3f} s", file=sys.stderr)
        print(f"[pipeline] load_batch calls took {loader.seconds:.3f} s in the loader thread(s); the writer thread waited {laps['result']:.3f} s "
              f"for results and spent {laps['consume']:.3f} s formatting / appending", file=sys.stderr)
        if loader.decode_on_gpu and any(du._LOAD_TRACE):
            a = du._LOAD_TRACE
            print(f"[pipeline] load_batch_device: group links {a[0]:.3f} s, object headers (resolve_many) {a[1]:.3f} s, device buffer {a[2]:.3f} s, "
                  f"B-trees + upload + inflate {a[3]:.3f} s", file=sys.stderr)
            a[:] = (0.0, 0.0, 0.0, 0.0)


class _RowsOnDevice:
    """a ticket whose rows sit in the shard buffer ``d_local``: result() brings them to the host for formatting"""

    def __init__(self, ticket, d_local, width, row, rows):
        self.ticket, self.d_local, self.width, self.row, self.rows = ticket, d_local, width, row, rows

    def result(self):
        self.ticket.result()
        return self.d_local.download((self.rows, self.width), np.float32, offset=self.row * self.width * 4)


class _ToDevice:
    """the model facade run_groups drives in a sharded run: the outputs of call after call land in ``d_local`` at the shard row"""
    sparse_ok = True          # predict_async_device reads SparseFrames batches too

    @property
    def takes_device_frames(self):
        return getattr(self.model, "takes_device_frames", False)

    def __init__(self, model, d_local, width):
        self.model, self.d_local, self.width = model, d_local, width
        self.row = 0
        self.device = model.device

    def predict_async(self, X):
        t = _RowsOnDevice(self.model.predict_async_device(X, self.d_local.ptr + self.row * self.width * 4), self.d_local, self.width,
                          self.row, len(X))
        self.row += len(X)
        return t
