#!/usr/bin/env python3
"""Records tests/golden/pair_layout_c54d474.npz and tests/golden/pair_estimate_c54d474.npz: the arrays tests/test_pair_layout_gpu.py and
tests/test_pair_estimate_gpu.py hold the layout of a routed scan call to.  Run on the GPU, from the repository root, with ANDI_HIP_LIB
naming libandihip_test.so of a build of commit c54d474 -- for the layout's arrays with the reading hook andi_hip_test_pair_layout added to
it (api.hip, api_internal.h: last_items, scan_call.hip: launch_routed, as they stand in this tree); pair_class and pair_cost come through
andi_hip_test_coop_items, which that commit has.

usage: record_parent_layout.py [layout|estimate ...]   (default: both)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
which = sys.argv[1:] or ["layout", "estimate"]
if "layout" in which:
    import test_pair_layout_gpu as T
    out = {}
    for name, (seqs, subjects) in T.cases().items():
        got = T.layout_of(seqs, subjects)
        for arr in T.ARRAYS:
            out[name + "." + arr] = np.asarray(got[arr])
        print(name, "pairs", len(got["pair_class"]), "of the wavefront kernel", int(((got["pair_class"] & 0x40) != 0).sum()), "counters", got["counts"].tolist())
    np.savez_compressed(T.FIXTURE, **out)
    print("wrote", T.FIXTURE, os.path.getsize(T.FIXTURE))
if "estimate" in which:
    import test_pair_estimate_gpu as E
    out = {}
    for name, (seqs, switches) in E.cases().items():
        cls, cost = E.verdicts_of(seqs, switches)
        out[name + ".pair_class"], out[name + ".pair_cost"] = cls, cost
        n = len(seqs)
        print(name, "pairs", len(cls), "of the wavefront kernel", int(((cls & 0x40) != 0).sum()), "class bytes", np.unique(cls).tolist(), "cost classes", len(np.unique(cost)))
        if n <= 6:
            print(((cls & 0x40) != 0).reshape(n, n).astype(int).tolist())
    np.savez_compressed(E.FIXTURE, **out)
    print("wrote", E.FIXTURE, os.path.getsize(E.FIXTURE))
