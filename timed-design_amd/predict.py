"""predict.py — the reference's command line, ``load_dataset_and_predict`` signature and output files, with the Keras
model object replaced by the HIP engine and the strictly sequential batch loop replaced by a pipeline:

    reference predict.py:121   frame_model = tf.keras.models.load_model(Path(m))
    reference predict.py:142   y_pred_batch = frame_model.predict(X_batch)
    here                       engine.load_model(m) ; frame_model.predict_async(X) ... .result()

    python3 predict.py --path_to_dataset data.hdf5 --path_to_model TIMED.h5 --path_to_output .

``--path_to_model`` takes a Keras legacy ``.h5`` (converted on the fly) or a ``.pack``; ``--path_to_dataset`` an
aposteriori ``.hdf5``, a frame pack, or a PDB file (``.pdb[.gz]`` / ``.pdb1[.gz]`` / ``.ent``: voxelised on the GPU by
timed_hip.voxeliser — parity unpinned against aposteriori).  Outputs (reference README.md:119-131): <model>.csv, <model>.fasta, <model>.txt,
dataset.fasta, datasetmap.txt, encoded_labels.csv, plus <model>_rot.csv in rotamer mode.

How a run is organised (all of it invisible in the files, which are byte-identical to a batch-by-batch run; the
pipeline itself — call groups, loader, staging, the loader / submitter / writer loop — is timed_hip/pipeline.py, which has no
counterpart in the reference):
  * consecutive reference batches are grouped into GPU calls of about ``frames_per_call`` frames;
  * a loader thread builds group g+1 (reference load_batch, utils.py:487-530) while the GPU computes group g and the
    main thread formats and appends the outputs of group g-1 (th_predict_async / th_predict_wait);
  * ``devices=[0, 1, ...]`` (``--devices 0,1``): one model handle per GPU in this process, groups dealt round-robin;
  * one process per GPU (WORLD_SIZE > 1: ``torch.distributed.run`` or any launcher that sets RANK / WORLD_SIZE /
    MASTER_ADDR / MASTER_PORT; the product itself needs no PyTorch): the flat dataset map is cut into contiguous per-rank
    shards, every rank predicts its shard into device memory AND formats the text of its own rows, ONE gather (RCCL over
    xGMI, th_comm_gather_rows) assembles the [N, n_classes] matrix on rank 0 for the per-chain sequences, every rank
    writes its text at its byte offset of the shared files; other ranks return only the dataset map.

Deliberate differences from the reference: the raw rotamer probabilities go to
``<model_name>_rot.csv`` (the reference's missing f-string writes a file literally called "{model_name}_rot.csv",
predict.py:123 — the UI and scripts expect the real name); the consensus files honour --path_to_output.
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from design_utils import utils as du
from timed_hip import engine, textio
from timed_hip.pipeline import GroupLoader, _RowsOnDevice, _ToDevice, call_spans, row_groups, run_groups

N_RESIDUE_CLASSES, N_ROTAMER_CLASSES = 20, 338


# ---- one model over one dataset --------------------------------------------------------------------------------
class _TextSink:
    """Append-only files held in memory: what one rank of a sharded run formats for ITS rows (put into the real files,
    at this rank's byte offset, by _assemble_shard_files)."""

    class _Handle:
        def __init__(self, blocks):
            self._blocks = blocks

        def write(self, data):
            # textio hands out views of a scratch buffer it reuses: keep a copy
            self._blocks.append(data.encode("ascii") if isinstance(data, str) else bytes(data))

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    def __init__(self):
        self.blocks = {}

    def opener(self, path):
        return self._Handle(self.blocks.setdefault(str(path), []))

    def size(self, path) -> int:
        return sum(len(b) for b in self.blocks.get(str(path), ()))


class _OutputFiles:
    """The per-model files of reference predict.py:123,145-155 / utils.save_outputs_to_file, appended group by group in
    row order, and the float16 matrix the reference re-reads from the CSV afterwards (predict.py:163).  With a ``sink``
    (sharded runs) the text of this rank's rows is collected in memory instead of being appended to the files."""

    def __init__(self, model_index, model_name, flat_dataset_map, path_to_output, predict_rotamers, codec, resume, sink=None,
                 device=None):
        self.model_index, self.model_name = model_index, model_name
        self.flat_dataset_map, self.path_to_output = flat_dataset_map, path_to_output
        self.codec = codec
        self.sink = sink
        # the GPU that formats the full-precision rotamer matrix (th_format_csv_device); None / TIMED_GPU_FORMAT=0: host threads
        self.device = device if os.environ.get("TIMED_GPU_FORMAT", "1") != "0" else None
        self.matrix_path = path_to_output / (f"{model_name}_rot.csv" if predict_rotamers else f"{model_name}.csv")
        # rows already in the file (an earlier, interrupted or repeated run) are part of what the reference reads back
        self.must_reread = resume or (self.matrix_path.exists() and self.matrix_path.stat().st_size > 0)
        self._f16_rows = []
        self._scratch = textio.TextScratch()        # the writer thread's text buffer (page-locked when the GPU formats into it)
        self._codec_matrix = (np.array([codec[k] for k in range(len(codec))], dtype=np.float16) if codec is not None else None)

    def paths(self):
        """the files ``append`` writes, in a fixed order (the dataset map is not one of them)"""
        out = [self.path_to_output / "encoded_labels.csv"] if self.model_index == 0 else []
        if self.codec is not None:
            out.append(self.matrix_path)
        return out + [self.path_to_output / f"{self.model_name}.csv"]

    def _open(self, path):
        return self.sink.opener(path) if self.sink is not None else open(path, "ab")

    def append(self, probs: np.ndarray, labels: np.ndarray):
        f16 = probs.astype(np.float16)
        if self.sink is None:
            self._f16_rows.append(f16)      # (sharded runs take the matrix from the gather instead)
        if self.codec is not None:
            with self._open(self.matrix_path) as f:
                # = np.savetxt(f, y_pred_batch, delimiter=","), full precision: 338 '%.18e' values per residue, formatted on the GPU
                textio.savetxt_csv(f, probs, device=self.device, scratch=self._scratch)     # (float32 rows only; anything else stays on the host threads)
            f16 = self._codec_matrix[np.argmax(probs, axis=1)]      # one-hot residue of the arg-max rotamer
        # the appends of utils.save_outputs_to_file, on arrays: no list-of-lists round trip under the GIL while the
        # submitter thread is waiting to launch the next group
        du.append_outputs(labels, f16, self.flat_dataset_map, self.model_index, self.model_name, self.path_to_output,
                          opener=self._open, write_map=self.sink is None)

    def close(self):
        self._scratch.close()

    def set_gathered(self, probs: np.ndarray):
        """sharded runs, rank 0: the [N, n_classes] float32 rows of every rank in map order (the RCCL gather)"""
        self._f16_rows = [probs.astype(np.float16)]

    def prediction_matrix(self) -> np.ndarray:
        """what np.genfromtxt(matrix_path, delimiter=",", dtype=np.float16) would return: '%.18e' text round-trips every
        float16/float32 exactly, so for a fresh file it is the float16 cast of what was written; a file that already
        held rows is read back."""
        if self.must_reread or not self._f16_rows:
            return textio.loadtxt_f16(self.matrix_path)
        return np.concatenate(self._f16_rows, axis=0)


def _assemble_shard_files(files, gather, rank, world):
    """Sharded runs: every rank formatted the text of its OWN rows (rows are independent, so the files of the 1-rank run
    are the concatenation of the ranks' texts in rank order).  The ranks tell each other how many bytes each file part
    has, and every rank writes its part at its byte offset — no text travels through rank 0 (config 4's _rot.csv is
    8.5 GB of '%.18e' text; formatted and written by one core it would idle eight GPUs).  One node, one file system."""
    paths = files.paths()
    mine = [files.sink.size(p) for p in paths]
    # rank 0 also reports what the files hold already (append semantics of utils.py:758,770: a resumed or repeated run)
    bases = [(p.stat().st_size if p.exists() else 0) if rank == 0 else 0 for p in paths]
    table = gather.allgather_ints(mine + bases)             # doubles as the barrier between "stat" and "write"
    if rank == 0 and not (files.path_to_output / "datasetmap.txt").exists():
        with open(files.path_to_output / "datasetmap.txt", "a") as f:
            du._savetxt_strings(f, files.flat_dataset_map)
    for j, p in enumerate(paths):
        offset = table[0][len(paths) + j] + sum(table[r][j] for r in range(rank))
        blocks = files.sink.blocks.get(str(p), [])
        if not blocks and rank != 0:
            continue                                        # (rank 0 always creates the file, even an empty one)
        fd = os.open(p, os.O_WRONLY | os.O_CREAT, 0o666)
        try:
            for b in blocks:
                view = memoryview(b)
                while len(view):
                    done = os.pwrite(fd, view, offset)
                    offset += done
                    view = view[done:]
        finally:
            os.close(fd)
    files.sink.blocks.clear()
    gather.barrier()                                        # rank 0 reads the assembled files from here on


def _distributed_context(gather):
    """(rank, world, local_rank, gather): world > 1 when launched one process per GPU (torch.distributed.run)."""
    from timed_hip import distributed as td
    if gather is not None:
        return gather.rank, gather.world, int(os.environ.get("LOCAL_RANK", gather.rank)), gather
    rank, world, local = td.env_rank_world()
    return rank, world, local, None


def load_dataset_and_predict(
    models: list,
    dataset_path: Path,
    batch_size: int = 20,
    start_batch: int = 0,
    dataset_map_path: Path = "datasetmap.txt",
    blacklist: Path = None,
    predict_rotamers: bool = False,
    model_name_suffix: str = "",
    is_consensus: bool = False,
    path_to_output: Path = Path.cwd(),
    device: int = 0,
    frames_per_call: int = None,
    devices=None,
    model_loader=None,
    gather=None,
    output_analysis: bool = False,
    output_auc: bool = False,
    property: str = None,
    property_map=None,
) -> (np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray):
    """reference predict.py:28-194 — same leading parameters and return tuple (flat_dataset_map, pdb_to_sequence,
    pdb_to_probability, pdb_to_real_sequence, pdb_to_consensus, pdb_to_consensus_prob).  ``start_batch`` keeps the
    reference's resume semantics (batches before it are skipped, outputs are appended).

    Opt-in extras: ``device`` / ``devices`` (HIP device indices for this process), ``frames_per_call`` (frames handed to
    a GPU per call), ``model_loader(path, device=...)`` (default ``timed_hip.engine.load_model``) and ``gather`` (a
    row-gather transport from ``timed_hip.distributed``; default: RCCL when WORLD_SIZE > 1) and ``output_analysis``
    (after each model's FASTA, rank 0 writes <model>_analysis.json, <model>_entropy.csv and <model>_per_structure.csv — see
    _write_analysis) and ``output_auc`` (20-class models with a 4-column map: rank 0 also writes <model>_auc.json — see
    _write_auc; rotamer models are evaluated per class by analyse_rotamers.py).

    ``dataset_path`` may be a directory of structures (a *structure set*, timed_hip/structureset.py): every file is parsed once,
    the frames of each call group are voxelised in HBM by one th_voxelise_batch call on the GPU that predicts the group.
    ``property`` ("polarity" / "charge") adds the reference's sixth channel (TIMED_polar / TIMED_charge; voxeliser spec item 8,
    PARITY UNPINNED AGAINST AMPAL AND APOSTERIORI) and also makes a single structure file a set; ``property_map``:
    {pdb_code: [ints]}, a list for a single structure, or the path of a JSON file with either — one integer per frame in
    dataset-map order; without it every residue carries the value of its own name."""
    path_to_output = Path(path_to_output)
    from timed_hip import structureset
    structure_set = None
    if property_map is not None and property is None:
        raise ValueError("a property map needs --property polarity or --property charge")
    if structureset.is_structure_set(dataset_path, property):
        if is_consensus:
            raise ValueError("--is_structure_nmr: a structure set voxelises model 1 of every file only; NMR ensembles go through a single file")
        structure_set = du.open_structure_set(dataset_path, property=property, property_map=property_map)
    else:
        du.forget_structure_set(dataset_path)          # (a file that an earlier call opened with a property)
    if structure_set is None and property is not None:
        raise ValueError(f"--property needs structures (a directory or a PDB file), {dataset_path} holds frames that exist already")
    if output_auc and predict_rotamers:
        raise ValueError("--output_auc scores the 20 residue classes; evaluate a rotamer model per class with analyse_rotamers.py")
    n_classes = N_ROTAMER_CLASSES if predict_rotamers else N_RESIDUE_CLASSES
    rank, world, local_rank, gather = _distributed_context(gather)
    sharded = world > 1 or gather is not None      # an explicit transport selects the shard + gather path even for 1 rank
    if rank == 0:
        print(f"Predicting {n_classes} classes per residue ({'rotamer' if predict_rotamers else 'residue'} mode)")
    loader = model_loader or engine.load_model
    # gzip .hdf5 datasets are inflated on the GPU unless TIMED_GPU_INFLATE=0 (or a model double without a device is in use)
    gpu_decode = model_loader is None and os.environ.get("TIMED_GPU_INFLATE", "1") != "0"
    if frames_per_call is None:
        # frames handed to a GPU per call: 1024 keeps the host->device copies of a call hidden behind the previous call's
        # kernels; a batch that is inflated ON the GPU is better large — one stream's Huffman layer is a
        # 5 ms serial chain whatever the batch, so 4096 frames cost 31 ms of decode where 4 x 1024 cost 45
        from timed_hip import framepack as _fp
        on_gpu = gpu_decode and not _fp.is_pack(dataset_path) and not _fp.is_structure(dataset_path)
        frames_per_call = 4096 if on_gpu else 1024
    if world > 1:
        device_ids = [local_rank if devices is None else list(devices)[local_rank % len(devices)]]
        if model_loader is None:
            from timed_hip import _lib
            visible = _lib.device_count()
            if device_ids[0] >= visible:
                raise RuntimeError(f"rank {rank} (local rank {local_rank}) needs HIP device {device_ids[0]} but only {visible} "
                                   f"device(s) are visible: launch one process per GPU")
    elif sharded:
        device_ids = [device]
    else:
        device_ids = [device] if not devices else list(devices)
    # the first model is loaded (device allocations, weight upload: native code) while this thread builds the dataset map
    side = ThreadPoolExecutor(max_workers=1, thread_name_prefix="predict_side")
    pending_handles = side.submit(lambda m=models[0]: [loader(Path(m), device=d) for d in device_ids]) if models else None
    if Path(dataset_map_path).exists():
        flat_dataset_map = du.read_flat_dataset_map(dataset_map_path)
    else:
        excluded = du.get_pdb_keys_to_filter(blacklist) if blacklist else []
        flat_dataset_map = du.flat_dataset_map_array(dataset_path, excluded)
    # (the reference converts to an array after the first model; rows slice as arrays)
    # what the sequence extraction needs from the map alone is prepared on the side thread, under the GPU's work
    plan = side.submit(du.SequencePlan, flat_dataset_map) if rank == 0 else None
    old_datasetmap = len(flat_dataset_map[0]) == 4
    codec, flat_categories = du.get_rotamer_codec() if predict_rotamers else (None, None)
    outputs = (None,) * 5
    try:
        for index, model_path in enumerate(models):
            model_name = (model_path.stem if isinstance(model_path, Path) else str(model_path)) + model_name_suffix
            handles = pending_handles.result()
            pending_handles = None
            if index + 1 < len(models):      # the next model loads while this one runs
                pending_handles = side.submit(lambda m=models[index + 1]: [loader(Path(m), device=d) for d in device_ids])
            srb = None
            files = None
            try:
                for h in handles:
                    if h.n_classes != n_classes:
                        raise ValueError(f"{model_path}: the model has {h.n_classes} outputs, predict_rotamers="
                                         f"{predict_rotamers} needs {n_classes}")
                    shape = getattr(h, "input_shape", None)
                    if structure_set is not None and shape is not None and tuple(shape) != tuple(structure_set.frame_dims):
                        raise ValueError(f"{model_path}: the model reads frames of {shape[-1]} channels {tuple(shape)}, the structures are "
                                         f"voxelised with {structure_set.n_channels} {tuple(structure_set.frame_dims)}"
                                         + (f" (--property {property} adds the sixth)" if property else " (a 6-channel model needs --property)"))
                if rank == 0:
                    # <model>.txt depends on the map only: written on the side thread while the GPU works
                    srb = side.submit(du.convert_dataset_map_for_srb, flat_dataset_map, model_name, path_to_output)
                if sharded:
                    files = _OutputFiles(index, model_name, flat_dataset_map, path_to_output, predict_rotamers, codec,
                                         resume=start_batch > 0, sink=_TextSink(), device=getattr(handles[0], "device", None))
                    gathered = _predict_sharded(handles[0], gather, rank, world, dataset_path, flat_dataset_map, batch_size,
                                                start_batch, frames_per_call, files, gpu_decode=gpu_decode)
                    if rank != 0:
                        continue
                    files.set_gathered(gathered)
                else:
                    files = _OutputFiles(index, model_name, flat_dataset_map, path_to_output, predict_rotamers, codec,
                                         resume=start_batch > 0, device=getattr(handles[0], "device", None))
                    groups = row_groups(len(flat_dataset_map), batch_size, start_batch, frames_per_call)
                    run_groups(handles, GroupLoader(handles, dataset_path, flat_dataset_map, groups, gpu_decode), files.append)
            finally:
                if files is not None:
                    files.close()
                for h in handles:
                    h.close()
                if srb is not None:
                    srb.result()
            matrix = files.prediction_matrix()
            outputs = du.extract_sequence_from_pred_matrix(
                flat_dataset_map, matrix, rotamers_categories=flat_categories if predict_rotamers else None,
                old_datasetmap=old_datasetmap, is_consensus=is_consensus, plan=plan.result())
            pdb_to_sequence, _prob, pdb_to_real_sequence, pdb_to_consensus, pdb_to_consensus_prob = outputs
            du.save_dict_to_fasta(pdb_to_sequence, model_name, path_to_output)
            du.save_dict_to_fasta(pdb_to_real_sequence, "dataset", path_to_output)
            if pdb_to_consensus:
                du.save_dict_to_fasta(pdb_to_consensus, model_name + "_consensus", path_to_output)
                du.save_consensus_probs(pdb_to_consensus_prob, model_name, path_to_output)
            if output_analysis:
                _write_analysis(matrix, flat_dataset_map, plan.result(), model_name, path_to_output, predict_rotamers,
                                flat_categories, device_ids[0])
            if output_auc:
                _write_auc(matrix, flat_dataset_map, plan.result(), model_name, path_to_output, device_ids[0])
    finally:
        if pending_handles is not None:          # a model that was prefetched but never used (an error above)
            try:
                for h in pending_handles.result():
                    h.close()
            except Exception:
                pass
        side.shutdown(wait=True)
    return (flat_dataset_map, *outputs)


def _write_analysis(matrix, flat_dataset_map, plan, model_name, path_to_output, predict_rotamers, flat_categories, device):
    """--output_analysis for one model: the float16 matrix the FASTA was read off (so resumed and sharded runs are covered) against
    the residue column of a 4-column map, on the GPU (timed_hip.analysis, th_analyse_probs).  Rotamer matrices are ranked per
    residue through the codec's column owners; their entropy is over all 338 columns.  A "<pdb> <count>" map carries no truth:
    entropies only, n_labelled 0 and every metric null.  Writes <model>_analysis.json, <model>_entropy.csv (one float64 per row
    in map order, np.savetxt's format) and <model>_per_structure.csv (one line per key in key order)."""
    import json
    from timed_hip import analysis
    n = matrix.shape[0]
    if n != plan.n_rows:
        raise ValueError(f"{model_name}: the prediction matrix has {n} rows, the dataset map {plan.n_rows}")
    if plan.old_datasetmap:
        true_res = analysis.residue_indices(np.asarray(flat_dataset_map)[:, 3])
    else:
        true_res = np.full(n, -1, np.int8)
    col_res = analysis.rotamer_columns(flat_categories) if predict_rotamers else analysis.identity_columns()
    got = analysis.analyse_probs(matrix, true_res, col_res, device=device)
    metrics = {"model": model_name, "rotamer_mode": bool(predict_rotamers),
               **analysis.metrics_from_totals(got.confusion, got.rank_hist, got.n_labelled, got.n_nonfinite, got.n_similar, n,
                                              got.entropy)}
    with open(path_to_output / f"{model_name}_analysis.json", "w") as f:
        json.dump(metrics, f, indent=1, allow_nan=False)
        f.write("\n")
    # np.savetxt's text of one value per row; rows are independent, so large vectors are formatted in parts on parallel threads
    parts = np.array_split(got.entropy, max(1, min(8, n // 16384)))
    with ThreadPoolExecutor(max_workers=len(parts)) as pool, open(path_to_output / f"{model_name}_entropy.csv", "wb") as f:
        for text in pool.map(textio.format_csv, parts):
            f.write(text)
    labelled = true_res >= 0
    similar = np.zeros(n, dtype=bool)
    similar[labelled] = analysis.BLOSUM62[true_res[labelled], got.pred[labelled]] > 0
    # per key (runs of rows, SequencePlan order): counts and sums by bincount over the key index of every row
    key_of_row = np.empty(n, dtype=np.int64)
    for i, key in enumerate(plan.keys):
        for lo, hi in plan.runs[key]:
            key_of_row[lo:hi] = i
    n_keys = len(plan.keys)

    def per_key(mask, weights=None):
        return np.bincount(key_of_row[mask], weights=None if weights is None else weights[mask], minlength=n_keys)
    finite = ~np.isnan(got.entropy)
    rows, n_lab = per_key(slice(None)), per_key(labelled)
    n_ent = per_key(finite).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        accuracy = per_key(labelled & (got.rank == 0)) / n_lab
        similarity = per_key(similar) / n_lab
        mean = per_key(finite, got.entropy) / n_ent
        dev = np.where(finite, got.entropy - mean[key_of_row], 0.0)
        std = np.sqrt(per_key(finite, dev * dev) / n_ent)           # ddof = 0
    lines = ["key,n_residues,n_labelled,accuracy,similarity,mean_entropy,std_entropy\n"]
    lines += [f"{key},{r},{nl},{a!r},{s!r},{m!r},{d!r}\n" for key, r, nl, a, s, m, d in
              zip(plan.keys, rows.tolist(), n_lab.tolist(), accuracy.tolist(), similarity.tolist(), mean.tolist(), std.tolist())]
    with open(path_to_output / f"{model_name}_per_structure.csv", "w") as f:
        f.write("".join(lines))

    def show(v):
        return "n/a" if v is None else f"{v:.4f}"
    print(f"[analysis] {model_name}: top-1 {show(metrics['accuracy_1'])}  top-3 {show(metrics['accuracy_3'])}  "
          f"macro recall {show(metrics['recall'])}  mean entropy {show(metrics['mean_entropy'])} bits  N={got.n_labelled}")


def _write_auc(matrix, flat_dataset_map, plan, model_name, path_to_output, device):
    """--output_auc for one 20-class model: ROC AUC one-vs-one and one-vs-rest of the float16 matrix the FASTA was read off against
    the residue column of a 4-column map, on the GPU (timed_hip.analysis, th_analyse_classes).  Writes <model>_auc.json: the keys
    of roc_auc_from_pairs (auc_ovo, auc_ovr, auc_ovr_present, auc_ovr_per_class in the order ACDEFGHIKLMNPQRSTVWY,
    n_classes_present) plus n_scored.  A "<pdb> <count>" map carries no truth: every value null."""
    import json
    from timed_hip import analysis
    n = matrix.shape[0]
    if n != plan.n_rows:
        raise ValueError(f"{model_name}: the prediction matrix has {n} rows, the dataset map {plan.n_rows}")
    if plan.old_datasetmap:
        true_res = analysis.residue_indices(np.asarray(flat_dataset_map)[:, 3])
    else:
        true_res = np.full(n, -1, np.int8)
    got = analysis.analyse_classes(matrix, true_res, device=device, auc=True, rows=False)
    result = {"model": model_name, "n_scored": got.n_scored, **analysis.roc_auc_from_pairs(got.pair_u2, got.scored_count)}
    with open(path_to_output / f"{model_name}_auc.json", "w") as f:
        json.dump(result, f, indent=1, allow_nan=False)
        f.write("\n")

    def show(v):
        return "n/a" if v is None else f"{v:.4f}"
    print(f"[auc] {model_name}: OvO {show(result['auc_ovo'])}  OvR {show(result['auc_ovr'])}  "
          f"classes present {result['n_classes_present']}  N={got.n_scored}")


def _predict_sharded(model, gather, rank, world, dataset_path, flat_dataset_map, batch_size, start_batch, frames_per_call, files,
                     gpu_decode=False):
    """One process per GPU: rows [row0, N) are cut into ``world`` contiguous shards (timed_hip.distributed.shard_bounds);
    this rank predicts its shard, formats the text of its own rows (``files``, an in-memory sink) while the GPU works,
    the probability shards are gathered to rank 0 in rank order = map order and the file parts are put
    together by _assemble_shard_files.  With the default transport the probabilities stay on the GPUs for the gather:
    predict_async writes them into a device shard buffer, th_comm_gather_rows moves them over xGMI, and the writer
    thread fetches each group's rows from the shard buffer for formatting.  Returns the [n, n_classes] float32 matrix
    on rank 0, None elsewhere."""
    from timed_hip import distributed as td
    row0 = min(start_batch * batch_size, len(flat_dataset_map))
    n = len(flat_dataset_map) - row0
    counts = td.shard_counts(n, world)
    lo, hi = td.shard_bounds(n, world)[rank]
    shard = flat_dataset_map[row0 + lo: row0 + hi]
    groups = call_spans(0, len(shard), max(1, int(frames_per_call)))      # (no ramp-up, and not in whole reference batches)
    own_transport = gather is None
    if own_transport:
        if os.environ.get("TIMED_GATHER", "rccl") == "host":
            # explicit opt-in for ranks that share a GPU (RCCL refuses two ranks on one device): rows travel over the TCP rendezvous
            gather = td.HostGather(rank, world)
        else:
            gather = td.RcclGather.from_environment(rank, world, model.device)     # raises when RCCL cannot be brought up
    try:
        if isinstance(gather, td.RcclGather):
            width = model.n_classes
            d_local = engine.DeviceBuffer(max(1, len(shard) * width * 4), model.device)
            to_device = _ToDevice(model, d_local, width)         # outputs land in d_local at the shard row
            run_groups([to_device], GroupLoader([to_device], dataset_path, shard, groups, gpu_decode), files.append)
            d_all = engine.DeviceBuffer(max(1, n * width * 4), model.device) if rank == 0 else None
            gather.gather_rows_device(d_local.ptr, counts, width, 0, d_all.ptr if d_all else 0)
            probs = d_all.download((n, width), np.float32) if rank == 0 else None
        else:                     # host transport (distributed.HostGather; tests/_gloo_transport.GlooGather): rows are on the host already
            local = np.zeros((len(shard), model.n_classes), dtype=np.float32)
            cursor = 0

            def keep(p, y):
                nonlocal cursor
                local[cursor:cursor + len(y)] = p
                cursor += len(y)
                files.append(p, y)
            run_groups([model], GroupLoader([model], dataset_path, shard, groups, gpu_decode), keep)
            probs = gather.gather_rows(local, counts, 0)
        _assemble_shard_files(files, gather, rank, world)
    finally:
        if own_transport:
            gather.close()
    return probs if rank == 0 else None


# ---- command line ----------------------------------------------------------------------------------------------
# (flag, argparse keywords): names, types and defaults are the reference's (predict.py:251-296); --device/--devices and
# --frames_per_call are additions of this build.
CLI_FLAGS = (
    ("--batch_size", dict(type=int, default=12, help="frames per reference batch; also the unit --start_batch-style resumes count in")),
    ("--path_to_dataset", dict(type=str, help="aposteriori frame dataset (.hdf5), frame pack, PDB file, or a directory of PDB files (voxelised on the GPU, group by group)")),
    ("--property", dict(type=str, default=None, choices=["polarity", "charge"], help="structures only: add the property channel of TIMED_polar / TIMED_charge (6-channel models). PARITY UNPINNED AGAINST AMPAL AND APOSTERIORI")),
    ("--path_to_property_map", dict(type=str, default=None, help="JSON {pdb_code: [ints]} (or a bare list for one structure): one value per frame in dataset-map order, {0,1} for polarity, {-1,0,1} for charge; default: each residue's own value")),
    ("--path_to_datasetmap", dict(type=str, default="datasetmap.txt", help="flat dataset map (.txt); created when missing")),
    ("--path_to_model", dict(type=str, help="Keras legacy .h5 model or converted .pack")),
    ("--path_to_blacklist", dict(type=str, default=None, help="directory of PDB lists to refuse (training-set structures)")),
    ("--path_to_output", dict(type=str, default=".", help="output directory (asked before it is created)")),
    ("--output_analysis", dict(action="store_true", help="also write <model>_analysis.json (top-k accuracy, macro precision / recall, confusion, bias, BLOSUM62 similarity), <model>_entropy.csv and <model>_per_structure.csv")),
    ("--output_auc", dict(action="store_true", help="also write <model>_auc.json (ROC AUC one-vs-one and one-vs-rest of the 20 residue classes; rotamer models: analyse_rotamers.py)")),
    ("--predict_rotamers", dict(action="store_true", help="the model predicts 338 rotamer classes instead of 20 residues")),
    ("--is_structure_nmr", dict(action="store_true", help="merge the states of an NMR ensemble into a consensus")),
    ("--device", dict(type=int, default=0, help="HIP device index")),
    ("--devices", dict(type=str, default=None, help="comma-separated HIP device indices to spread the frames over")),
    ("--frames_per_call", dict(type=int, default=None, help="frames handed to a GPU per call (default 1024; 4096 for .hdf5 datasets inflated on the GPU)")),
)


def build_parser():
    parser = argparse.ArgumentParser(description="Residue / rotamer probabilities for every frame of a dataset (MI355X)")
    for flag, keywords in CLI_FLAGS:
        parser.add_argument(flag, **keywords)
    return parser


def _confirm_output_directory(directory: Path):
    if directory.exists():
        return
    print(f"{directory} does not exist yet - create it? (y/n)")
    if input() != "y":
        print("Nothing written.")
        sys.exit()
    directory.mkdir(parents=True, exist_ok=True)


def main(args):
    required = {"model": Path(args.path_to_model), "dataset": Path(args.path_to_dataset)}
    if args.path_to_blacklist:
        required["blacklist"] = Path(args.path_to_blacklist)
    _confirm_output_directory(Path(args.path_to_output))
    for what, path in required.items():
        assert path.exists(), f"No {what} at {path}"
    assert args.batch_size > 0, f"--batch_size must be positive, got {args.batch_size}"
    devices = [int(d) for d in args.devices.split(",")] if getattr(args, "devices", None) else None
    try:
        return _main_predict(args, required, devices)
    finally:
        du.release_device_memory()           # pooled batch buffers + the GPU decoder's scratch: a CLI run keeps nothing


def _main_predict(args, required, devices):
    return load_dataset_and_predict(
        [required["model"]], required["dataset"], batch_size=args.batch_size, start_batch=0,
        dataset_map_path=Path(args.path_to_datasetmap), blacklist=required.get("blacklist"),
        predict_rotamers=args.predict_rotamers, is_consensus=args.is_structure_nmr,
        path_to_output=Path(args.path_to_output), device=getattr(args, "device", 0), devices=devices,
        frames_per_call=getattr(args, "frames_per_call", None), output_analysis=bool(getattr(args, "output_analysis", False)),
        output_auc=bool(getattr(args, "output_auc", False)), property=getattr(args, "property", None),
        property_map=getattr(args, "path_to_property_map", None))


if __name__ == "__main__":
    main(build_parser().parse_args())
