"""Diversity and native recovery of the sequences drawn by sample.py, on the GPU (timed_hip.seqset, th_seqset): how close the draws
are to the native, how different from one another and how many are the same sequence twice, which few to fold, and the per-position
profile of the ensemble — the step between sample.py and analyse_models.py.

    python analyse_samples.py --path_to_samples FILE [FILE ...] --path_to_output DIR [--path_to_datasetmap MAP [--support_old_datasetmap]]
                              [--path_to_native_fasta F] [--cluster_identity 0.9] [--matrix] [--device N]

The samples are the ``.json`` or ``.fasta`` files of sample.py; a key in several files keeps its draws in file order.  Natives come
from the 4-column dataset map (the true sequences of ``SequencePlan``) or from a FASTA whose names are the keys; a key without one is
scored without a native.  Written: ``sample_scores.csv`` (one row per draw), ``set_scores.csv`` (one row per key),
``position_profile.csv`` (key, position, native letter, consensus, entropy in bits, native count, the 21 counts),
``representatives.fasta`` (the cluster representatives under their sample.py names, ready to be folded) and, with ``--matrix``,
``<key>_identity.csv`` (the N x N matching positions).

The clustering is greedy, in input order, at ``--cluster_identity`` of the length: the incremental scheme of CD-HIT-like tools in its
plainest form — THIS PROJECT'S OWN RULE, NOT THEIR CODE: no word filter, no length sorting, no alignment.  A key whose draws have unequal
lengths, or whose native has another length, carries its error and does not stop the others."""
import argparse
import csv
import os

import numpy as np

from timed_hip import seqset

SAMPLE_COLUMNS = ["key", "sample", "name", "identity_to_native", "similarity_to_native", "native_score", "mean_identity_to_others",
                  "nearest_identity", "nearest_index", "first_equal", "distinct", "cluster", "representative"]
SET_COLUMNS = ["key", "n", "length", "mean_identity_to_native", "mean_pairwise_identity", "n_distinct", "n_clusters", "min_matches", "error"]
PROFILE_COLUMNS = ["key", "position", "native", "consensus", "entropy_bits", "native_count"] + [f"n_{c}" for c in seqset.LETTERS]


def load_natives(args) -> dict:
    natives = {}
    if args.path_to_datasetmap:
        from design_utils import utils as du
        plan = du.SequencePlan(du.load_datasetmap(args.path_to_datasetmap, is_old=args.support_old_datasetmap))
        natives.update({k: v for k, v in plan.real.items() if v})
    if args.path_to_native_fasta:
        natives.update(seqset.read_native_fasta(args.path_to_native_fasta))
    return natives


def _number(v) -> str:
    return "" if v != v else repr(float(v))


def main(args):
    samples = {}
    for path in args.path_to_samples:
        for key, draws in seqset.read_samples(path).items():
            samples.setdefault(key, []).extend(draws)
    natives = load_natives(args)
    keys = list(samples)
    stats = {}
    results = seqset.analyse([samples[k] for k in keys], [natives.get(k) for k in keys], cluster_identity=args.cluster_identity,
                             matrix=args.matrix, device=args.device, stats=stats)
    out = args.path_to_output
    os.makedirs(out, exist_ok=True)
    paths = [os.path.join(out, name) for name in ("sample_scores.csv", "set_scores.csv", "position_profile.csv", "representatives.fasta")]
    with open(paths[0], "w", newline="") as fd, open(paths[1], "w", newline="") as fs, open(paths[2], "w", newline="") as fp, open(paths[3], "w") as fr:
        wd, ws, wp = csv.writer(fd), csv.writer(fs), csv.writer(fp)
        wd.writerow(SAMPLE_COLUMNS)
        ws.writerow(SET_COLUMNS)
        wp.writerow(PROFILE_COLUMNS)
        for key, res in zip(keys, results):
            if res.error:
                ws.writerow([key, len(samples[key]), "", "", "", "", "", "", res.error])
                continue
            ws.writerow([key, res.n, res.length, _number(res.mean_identity_to_native), _number(res.mean_pairwise_identity), res.n_distinct,
                         res.n_clusters, res.min_matches, ""])
            columns = [res.identity_to_native, res.similarity_to_native, res.native_score, res.mean_identity_to_others, res.nearest_identity]
            for i in range(res.n):
                wd.writerow([key, i, f"{key}_{i}"] + [_number(c[i]) for c in columns] +
                            [int(res.nearest_index[i]), int(res.first_equal[i]), int(res.first_equal[i] == i), int(res.cluster[i]), int(res.cluster[i] == i)])
            consensus, entropy, count = res.consensus, res.position_entropy, res.native_count
            for p in range(res.length):
                wp.writerow([key, p, "" if res.native is None else seqset.LETTERS[res.native[p]], seqset.LETTERS[consensus[p]], _number(entropy[p]),
                             "" if res.native is None else int(count[p])] + res.profile[p].tolist())
            for i in res.representatives.tolist():
                fr.write(f">{key}_{i}\n{samples[key][i]}\n")
            if args.matrix:
                paths.append(os.path.join(out, f"{key}_identity.csv"))
                np.savetxt(paths[-1], res.matrix, fmt="%d", delimiter=",")
    failed = sum(1 for res in results if res.error)
    print(f"{len(keys)} keys ({failed} with an error), {sum(res.n for res in results)} sequences in {stats.get('submissions', 0)} GPU submission(s) -> {out}")
    return paths


CLI_FLAGS = (
    ("--path_to_samples", dict(type=str, nargs="+", required=True, help="the .json or .fasta files written by sample.py")),
    ("--path_to_output", dict(type=str, required=True, help="folder for the tables (created)")),
    ("--path_to_datasetmap", dict(type=str, default=None, help="4-column dataset map (.txt): its true sequences are the natives")),
    ("--support_old_datasetmap", dict(action="store_true", default=False, help="the dataset map is the old 4-column csv")),
    ("--path_to_native_fasta", dict(type=str, default=None, help="FASTA of natives whose names are the keys (wins over the map)")),
    ("--cluster_identity", dict(type=float, default=0.9, help="a draw joins the first representative it matches at this share of the positions (taken in per-mille)")),
    ("--matrix", dict(action="store_true", default=False, help="also write <key>_identity.csv, the N x N matching positions")),
    ("--device", dict(type=int, default=0, help="HIP device")),
)


def build_parser():
    parser = argparse.ArgumentParser(description="Diversity and native recovery of sampled sequences, batched on the GPU (MI355X).  Greedy "
                                                 "clustering in input order: THIS PROJECT'S OWN RULE, NOT THEIR CODE (CD-HIT-like tools)",
                                     epilog=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flag, keywords in CLI_FLAGS:
        parser.add_argument(flag, **keywords)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
