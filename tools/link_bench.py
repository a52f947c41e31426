#!/usr/bin/env python3
"""Measures the linkage kernels (linkage_map, csrc/link.hip) on one GPU against td_ld_pairs over the same resident
matrix and writes profiles/link/bench_mi355x.txt.

    python tools/link_bench.py [--repeat 5] [--out FILE]

Calls resident on the device: a doubled-haploid population (codes 0 / 2) of linkage groups of 200 markers, neighbours
4 % recombination apart, a random phase per marker, 5 % of the cells missing; every marker takes part with the class
pair (0, 2).  Thresholds: the defaults of tag_linkage (LOD 3, rf 0.25, 50 shared) for td_link_pairs, min_r2 0.8 and
min_shared 50 for td_ld_pairs.
Per kernel, device time by HIP events inside the library, best and median of --repeat calls after a warm-up of the same
shape: k_link_counts, k_link_gather, k_link_pairs; beside them k_calls_transpose<true> and k_ld_pairs of td_ld_pairs in
the same process on the same buffer, the calls of the two alternating, and the ratio of the medians of the two pair
kernels.  A second run of each with min_shared above the rows leaves the epilogues nothing past their first exit: the
ratio of those is the ratio of the loops (two MFMA chains over two planes against six over three).
(a) 384 x 50 000        (b) 2 000 x 5 000"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tagdigger_amd import tagdigger_fun as tf                    # noqa: E402
from tagdigger_amd.engine import LINK_LOD_MIN, LINK_TILE, default_engine  # noqa: E402


def population(rng, S, M, per_group=200, step=0.04, missing=0.05):
    C = np.empty((S, M), dtype=np.uint8)
    strand = None
    for m in range(M):
        if m % per_group == 0:
            strand = rng.integers(0, 2, size=S)
        else:
            strand = strand ^ (rng.random(S) < step)
        C[:, m] = (strand ^ int(rng.integers(0, 2))) * 2
    C[rng.random((S, M)) < missing] = 3
    return C


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link", "bench_mi355x.txt"))
    args = ap.parse_args(argv)
    eng = default_engine(args.device)
    rng = np.random.default_rng(4240)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def stat(values):
        v = sorted(values)
        return v[0], v[len(v) // 2]

    say("linkage, tools/link_bench.py; TILE %d; device ms: HIP events inside td_link_counts, td_link_pairs and td_ld_pairs" % LINK_TILE)
    min_lod16 = tf.linkage_min_lod16("3")

    def measure(label, S, M):
        calls = population(rng, S, M)
        cls = np.full(M, 2, dtype=np.uint8)
        lodtab = np.array(tf.linkage_tables(S), dtype=np.int64)
        link = dict(max_rf_ppm=250000, min_lod16=min_lod16, min_shared=50)
        ld = dict(min_r2_ppm=800000, min_shared=50)
        d = eng.dev_alloc(S * M)
        try:
            eng.h2d(d, calls.tobytes())
            n_link = eng.link_pairs(d, cls, lodtab, shape=(S, M), count_only=True, **link).n          # warm-up, and the buffers' sizes
            n_ld = eng.ld_pairs(d, shape=(S, M), count_only=True, **ld).n
            eng.link_counts(d, shape=(S, M))
            t = {k: [] for k in ("counts", "gather", "link", "sort", "transpose", "ld", "ld_sort", "link0", "ld0")}
            for _ in range(args.repeat):                   # the two alternate
                t["counts"].append(eng.link_counts(d, shape=(S, M))[1])
                r = eng.link_pairs(d, cls, lodtab, shape=(S, M), capacity=n_link, retry=False, **link)
                t["gather"].append(r.times["gather_ms"]), t["link"].append(r.times["pairs_ms"]), t["sort"].append(r.times["sort_ms"])
                r = eng.ld_pairs(d, shape=(S, M), capacity=n_ld, retry=False, **ld)
                t["transpose"].append(r.times["transpose_ms"]), t["ld"].append(r.times["pairs_ms"]), t["ld_sort"].append(r.times["sort_ms"])
                r = eng.link_pairs(d, cls, lodtab, shape=(S, M), count_only=True, max_rf_ppm=0, min_lod16=LINK_LOD_MIN, min_shared=S + 1)
                t["link0"].append(r.times["pairs_ms"])
                r = eng.ld_pairs(d, shape=(S, M), count_only=True, min_r2_ppm=1000000, min_shared=S + 1)
                t["ld0"].append(r.times["pairs_ms"])
        finally:
            eng.dev_free(d)
        tiles = -(-M // LINK_TILE)
        say("%s: %d x %d, %d tile pairs; %d linkage edges (LOD 3, rf 0.25, 50 shared), %d LD edges (r2 0.8, 50 shared) of %d pairs" % (
            label, S, M, tiles * (tiles + 1) // 2, n_link, n_ld, M * (M - 1) // 2))
        for name, key in (("k_link_counts", "counts"), ("k_link_gather", "gather"), ("k_link_pairs", "link"),
                          ("k_calls_transpose (LD)", "transpose"), ("k_ld_pairs", "ld"),
                          ("k_link_pairs, no pair past the first exit", "link0"), ("k_ld_pairs, no pair past the first exit", "ld0")):
            say("  %-44s device ms over %d calls: best %.3f median %.3f" % ((name, args.repeat) + stat(t[key])))
        say("  k_link_counts reads %.1f MB: %.0f GB/s (median)" % (S * M / 1e6, S * M / 1e9 / (stat(t["counts"])[1] * 1e-3)))
        say("  ratio k_link_pairs / k_ld_pairs (medians): %.3f with their edges, %.3f with no pair past the first exit" % (
            stat(t["link"])[1] / stat(t["ld"])[1], stat(t["link0"])[1] / stat(t["ld0"])[1]))
        say("  sort of the edges on the host, wall ms (median): linkage %.3f, LD %.3f" % (stat(t["sort"])[1], stat(t["ld_sort"])[1]))

    measure("(a)", 384, 50000)
    measure("(b) many offspring", 2000, 5000)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
