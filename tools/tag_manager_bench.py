#!/usr/bin/env python3
"""Tag Manager on one MI355X: wall time of this build's mergedTagList, compareTagSets and consolidateTagSets (device
backend) on seeded synthetic databases, the device ms of K1 (pack), K2 (radix sort), K3 (lookup walks) and K4
(variable sites) inside them, and beside them the reference's CPU time.  The reference's figures are the rates measured
on one core of a build-host Xeon for 10^5 markers of two 64-bp tags (mergedTagList 4.3 s, compareTagSets 5.4 s,
consolidateTagSets 15.7 s), scaled linearly in markers: a lower bound, since compareTagSets grows faster than n, and
not measured on the GPU box.  One JSON line per (markers, tag length, function).

    python tools/tag_manager_bench.py [--markers 100000,1000000] [--lengths 64,150] [--funcs merged,compare,consolidate]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF_S_PER_1E5 = {"merged": 4.3, "compare": 5.4, "consolidate": 15.7}


def synth(n, L, seed):
    """An old database of n markers (two L-bp tags, one SNP) and a new study of n markers: 40 % the same tags, 20 %
    shorter versions, 40 % new."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    a = alpha[rng.integers(0, 4, (n, L), dtype=np.uint8)]
    p = rng.integers(5, L - 5, n)
    b = a.copy()
    b[np.arange(n), p] = alpha[(np.searchsorted(alpha, a[np.arange(n), p]) + rng.integers(1, 4, n)) % 4]
    c = alpha[rng.integers(0, 4, (n, L), dtype=np.uint8)]
    d = c.copy()
    d[:, L // 2] = alpha[(np.searchsorted(alpha, c[:, L // 2]) + 1) % 4]
    A = [x.decode() for x in a.view(f"S{L}").ravel()]
    B = [x.decode() for x in b.view(f"S{L}").ravel()]
    C = [x.decode() for x in c.view(f"S{L}").ravel()]
    D = [x.decode() for x in d.view(f"S{L}").ravel()]
    old = [[], []]
    new = [[], []]
    kind = rng.random(n)
    cut = L - 10
    for i in range(n):
        old[0] += ["M%07d_0" % i, "M%07d_1" % i]
        old[1] += [A[i], B[i]]
        if kind[i] < 0.4:
            na, nb = A[i], B[i]
        elif kind[i] < 0.6 and p[i] < cut:
            na, nb = A[i][:cut], B[i][:cut]
        else:
            na, nb = C[i], D[i]
        new[0] += ["N%07d_0" % i, "N%07d_1" % i]
        new[1] += [na, nb]
    return old, new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markers", default="100000,1000000")
    ap.add_argument("--lengths", default="64,150")
    ap.add_argument("--funcs", default="merged,compare,consolidate")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from tagdigger_amd import tagdigger_fun as tf
    from tagdigger_amd import tagset
    from tagdigger_amd.engine import default_engine
    default_engine(args.device)
    warm = synth(1000, 64, 0)                      # code objects loaded, allocator warm
    with contextlib.redirect_stdout(io.StringIO()):
        tf.consolidateTagSets(warm[0], warm[1], device=args.device)
        tf.mergedTagList(warm[0], device=args.device)
    for n in [int(x) for x in args.markers.split(",")]:
        for L in [int(x) for x in args.lengths.split(",")]:
            old, new = synth(n, L, 1)
            for f in args.funcs.split(","):
                tagset.stage_ms.clear()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    if f == "merged":
                        tf.mergedTagList(old, device=args.device)
                    elif f == "compare":
                        tf.compareTagSets(old, new, device=args.device)
                    else:
                        tf.consolidateTagSets(old, new, device=args.device)
                wall = time.perf_counter() - t0
                ref = REF_S_PER_1E5[f] * n / 1e5
                print(json.dumps({"func": f, "markers": n, "tag_bp": L, "tags_per_set": 2 * n, "wall_s": round(wall, 3),
                                  "device_ms": {k: round(v, 3) for k, v in sorted(tagset.stage_ms.items())},
                                  "reference_cpu_s": round(ref, 1) if L == 64 else None,
                                  "reference_note": ("issue's build-host rate x markers / 10^5 (lower bound; not "
                                                     "measured on the GPU box)" if L == 64 else
                                                     "not measured (the issue's rates are for 64-bp tags)"),
                                  "speedup_vs_reference": round(ref / wall, 2) if L == 64 else None}), flush=True)


if __name__ == "__main__":
    main()
