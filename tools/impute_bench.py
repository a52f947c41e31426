#!/usr/bin/env python3
"""Measures LD-kNN imputation (impute_calls, csrc/impute.hip) on one GPU and writes profiles/impute/bench_mi355x.txt.

    python tools/impute_bench.py [--shapes 384x50000,2000x5000] [--repeat 5] [--no-host] [--out FILE]

Calls structured as in tests/ld_cases.py, with one founder column per 25 markers instead of 8 in all, so that a marker is
in LD with some two dozen others and not with an eighth of the matrix: every marker a copy of a founder with 10 % of its
cells redrawn, then 10 % of the cells missing.  l = 20, k = 10, min_overlap = 4, min_conf = 0.6, neighbours at r^2 >= 0.5
over at least 50 samples.
Per shape:
  - device time by HIP events inside td_impute_knn, best and median of --repeat calls after a warm-up of the same shape, the
    calls resident on the device and the table made beforehand: the transpose pre-pass, k_impute;
  - wall time of impute_calls from a host matrix, its own marker_ld included, on the gpu backend (three calls) and on the
    host backend (one call) with the CPUs this process may use; the filled matrices and the statistics are compared
    before a time is printed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tagdigger_amd import tagdigger_fun as tf                    # noqa: E402
from tagdigger_amd.engine import default_engine                  # noqa: E402


def structured(rng, S, M):
    nf = max(2, M // 25)
    founders = rng.integers(0, 3, size=(S, nf), dtype=np.uint8)
    C = founders[:, rng.integers(0, nf, size=M)].copy()
    noise = rng.random((S, M)) < 0.1
    C[noise] = rng.integers(0, 3, size=int(noise.sum()), dtype=np.uint8)
    C[rng.random((S, M)) < 0.1] = 3
    return C


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="384x50000,2000x5000")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="leave the host backend's wall time out")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impute", "bench_mi355x.txt"))
    args = ap.parse_args(argv)
    eng = default_engine(args.device)
    rng = np.random.default_rng(4170)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    kw = dict(l=20, k=10, min_overlap=4, min_conf=0.6, min_r2=0.5, ld_min_shared=50)
    say("LD-kNN imputation, tools/impute_bench.py; l 20, k 10, min_overlap 4, min_conf 0.6, neighbours at r^2 >= 0.5 over >= 50 samples")
    say("device ms: HIP events around k_calls_transpose<false> and k_impute inside td_impute_knn")
    for shape in args.shapes.split(","):
        S, M = (int(x) for x in shape.split("x"))
        calls = structured(rng, S, M)
        names = ["m%d" % m for m in range(M)]
        d = eng.dev_alloc(S * M)
        try:
            eng.h2d(d, calls.tobytes())
            ld = tf.marker_ld(tf.DeviceCalls(d, (S, M)), names, min_r2=kw["min_r2"], min_shared=kw["ld_min_shared"], device=args.device)
            nbr = tf.ld_neighbours(ld, kw["l"])
            knn = dict(k=kw["k"], min_overlap=kw["min_overlap"], min_conf_ppm=600000, fetch=False)
            first = eng.impute_knn(d, nbr, shape=(S, M), **knn)                                  # warm-up
            runs = [eng.impute_knn(d, nbr, shape=(S, M), **knn) for _ in range(args.repeat)]
        finally:
            eng.dev_free(d)
        tot = first.stats.sum(axis=0, dtype=np.uint64)
        t = {key: sorted(r.times[key] for r in runs) for key in ("transpose_ms", "vote_ms")}
        say()
        say("%d x %d: %d edges, %.1f neighbours a marker of %d; missing %d, imputed %d, no_donor %d, undecided %d" % (
            S, M, len(ld.edges), (nbr >= 0).sum() / max(1, M), kw["l"], *(int(x) for x in tot)))
        say("  transpose pre-pass  device ms over %d calls: best %.3f median %.3f" % (
            args.repeat, t["transpose_ms"][0], t["transpose_ms"][len(runs) // 2]))
        say("  k_impute            device ms over %d calls: best %.3f median %.3f (%.1f ns a missing cell)" % (
            args.repeat, t["vote_ms"][0], t["vote_ms"][len(runs) // 2], 1e6 * t["vote_ms"][len(runs) // 2] / max(1, int(tot[0]))))
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            dev = tf.impute_calls(calls, names, device=args.device, **kw)
            walls.append(time.perf_counter() - t0)
        say("  wall: impute_calls(backend='gpu') from a host matrix, marker_ld included: %s s (kernels of the imputation %.3f ms)" % (
            " ".join("%.3f" % w for w in walls), dev.ms))
        if args.no_host:
            say("  wall: impute_calls(backend='host'): not measured")
            continue
        t0 = time.perf_counter()
        host = tf.impute_calls(calls, names, backend="host", **kw)
        t_host = time.perf_counter() - t0
        if dev.calls.tobytes() != host.calls.tobytes() or not np.array_equal(dev.stats, host.stats) or not np.array_equal(dev.neighbours, host.neighbours):
            raise SystemExit("device and host results differ at %s" % shape)
        say("  wall: impute_calls(backend='host') %.3f s with %s CPUs; device and host agree on every byte and every count" % (
            t_host, os.environ.get("OMP_NUM_THREADS", "all")))
    say()
    say("what bounds k_impute: not measured (no counter run was made)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
