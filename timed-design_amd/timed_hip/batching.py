"""Host-side batching shared by the structure analyses (timed_hip.structure, .superpose, .lddt, .tmscore): files are parsed on host threads,
the work is cut into runs of consecutive items whose flat arrays fit a byte budget, and each run is one GPU submission.  An
analysis supplies its layouts, its cost per unit in bytes and a ``submit(part, timing)`` closure that concatenates one run, makes
the one call and slices the outputs back.  No GPU and no ctypes here."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import Callable, List, Optional, Sequence, Tuple

BATCH_BYTES = 256 << 20            # host bytes of flat arrays handed to one call


def parse_each(fn: Callable, items, workers: int) -> list:
    """``[fn(item) for item in items]`` on at most ``workers`` host threads (at least 1, at most 16), in the order of ``items``;
    an exception of ``fn`` is raised here."""
    items = list(items)
    if not items:
        return []
    with ThreadPoolExecutor(max_workers=max(1, min(int(workers), 16))) as pool:
        return list(pool.map(fn, items))


def cut_batches(sizes: Sequence[int], budget_bytes: int, item_bytes: int) -> List[Tuple[int, int]]:
    """[lo, hi) runs of consecutive items whose arrays — ``item_bytes`` per unit of ``sizes`` — fit ``budget_bytes`` (an item above
    it goes alone)."""
    runs, lo, used = [], 0, 0
    for k, n in enumerate(sizes):
        need = int(n) * item_bytes
        if k > lo and used + need > budget_bytes:
            runs.append((lo, k))
            lo, used = k, 0
        used += need
    if len(sizes) > lo:
        runs.append((lo, len(sizes)))
    return runs


def run_batches(items: Sequence, sizes: Sequence[int], budget_bytes: int, item_bytes: int, submit: Callable, stats: Optional[dict] = None) -> None:
    """``submit(items[lo:hi], timing)`` for every run of ``cut_batches``, in order.  ``timing`` is a dict whose ``kernel_ms`` the
    calls add to, or None when nobody asks; ``stats`` grows by ``submissions`` and ``kernel_ms``."""
    runs = cut_batches(sizes, budget_bytes, item_bytes)
    timing = {} if stats is not None else None
    for lo, hi in runs:
        submit(items[lo:hi], timing)
    if stats is not None:
        stats["submissions"] = stats.get("submissions", 0) + len(runs)
        stats["kernel_ms"] = stats.get("kernel_ms", 0.0) + timing.get("kernel_ms", 0.0)
