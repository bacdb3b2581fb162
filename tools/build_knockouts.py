#!/usr/bin/env python
"""Build the knock-out library: the product's sources and flags plus -DTH_KNOCKOUTS=1 (csrc/common.h).

    python tools/build_knockouts.py [--force]

Objects go to timed-design_amd/csrc/build_knock/, the library to timed-design_amd/timed_hip/libtimedhip_knock.so; the product
library is not touched.  Only this library has the TH_WF_DBG / TH_FIRST_DBG / TH_WINO_DBG / TH_CONV_DBG / TH_PW_DBG knobs (the
product refuses to load a model while one is set).  Its results are WRONG by design whenever one of them is set: it is for timing
experiments, loaded in a process of its own through the last line printed here:

    TIMED_HIP_LIB=.../libtimedhip_knock.so TH_WF_DBG=2 python tools/bench_layer.py 10 32 64 3 8192 1

It also has TH_TM_STAGE=1 (th_tmscore with the coordinates staged in LDS; right results, see profiles/tmscore.txt).

A library newer than every source and header is left alone (the objects may be gone: nothing is compiled then)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry

OBJDIR = os.path.join(entry.CSRC, "build_knock")
LIB = os.path.join(entry.PKG, "timed_hip", "libtimedhip_knock.so")


def main() -> None:
    force = "--force" in sys.argv[1:]
    deps = [os.path.join(entry.CSRC, f) for f in os.listdir(entry.CSRC) if f.endswith((".hip", ".h"))]
    deps.append(os.path.join(ROOT, "include", "timed_hip.h"))
    if force or not entry._newer(LIB, deps):
        entry.build_lib(force=force, objdir=OBJDIR, lib=LIB, extra_flags=["-DTH_KNOCKOUTS=1"], max_jobs=16)
    print(f"TIMED_HIP_LIB={LIB}")


if __name__ == "__main__":
    main()
