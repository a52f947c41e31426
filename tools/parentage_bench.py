#!/usr/bin/env python3
"""Measures the Mendelian trio counts (parentage, csrc/parent.hip) on one GPU and writes profiles/parentage/bench_mi355x.txt.

    python tools/parentage_bench.py [--cases 384x50000x32,384x50000x128,2000x5000x32] [--repeat 5] [--no-host] [--out FILE]

A case is samples x markers x candidates.  Calls drawn uniformly from 0 / 1 / 2 with 10 % of the cells missing; every
sample is an offspring.  The time of the kernels depends on the shape alone, not on the calls, so no pedigree is simulated:
for the device times every offspring gets C distinct candidates drawn at random; for the wall times the pair test is
opened (max_pair_err 1, min_shared 1), so that parentage keeps max_candidates = C candidates of every offspring.
Per case:
  - device time by HIP events inside td_parent_trios, best and median of --repeat calls after a warm-up of the same shape,
    the calls resident on the device: k_par_pack, k_par_trios, k_par_rank;
  - wall time of parentage from a host matrix, its relate_joint included, on the gpu backend (three calls) and on the host
    backend (one call) with the CPUs this process may use; the results are compared before a time is printed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tagdigger_amd import tagdigger_fun as tf                    # noqa: E402
from tagdigger_amd.engine import default_engine                  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="384x50000x32,384x50000x128,2000x5000x32")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="leave the host backend's wall time out")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parentage", "bench_mi355x.txt"))
    args = ap.parse_args(argv)
    eng = default_engine(args.device)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("Mendelian trio counts, tools/parentage_bench.py; selfing allowed, top 2, uniform calls with 10 % missing")
    say("device ms: HIP events around k_par_pack, k_par_trios and k_par_rank inside td_parent_trios")
    for case in args.cases.split(","):
        S, M, C = (int(x) for x in case.split("x"))
        rng = np.random.default_rng(4180 + S + M + C)
        calls = rng.integers(0, 3, size=(S, M), dtype=np.uint8)
        calls[rng.random((S, M)) < 0.1] = 3
        names = ["s%d" % s for s in range(S)]
        cand = np.stack([rng.permutation(np.delete(np.arange(S), o))[:C] for o in range(S)]).astype(np.int32)
        d = eng.dev_alloc(S * M)
        try:
            eng.h2d(d, calls.tobytes())
            kw = dict(shape=(S, M), top=2, min_shared=50)
            eng.parent_trios(d, np.arange(S), cand, **kw)                                        # warm-up
            runs = [eng.parent_trios(d, np.arange(S), cand, **kw) for _ in range(args.repeat)]
        finally:
            eng.dev_free(d)
        t = {key: sorted(r.times[key] for r in runs) for key in ("pack_ms", "trio_ms", "rank_ms")}
        T = C * (C + 1) // 2
        words = S * T * ((M + 63) // 64)
        say()
        say("%d x %d, C = %d: %d offspring x %d trios x %d words = %.3g trio-words" % (S, M, C, S, T, (M + 63) // 64, words))
        for key, name in (("pack_ms", "k_par_pack "), ("trio_ms", "k_par_trios"), ("rank_ms", "k_par_rank ")):
            extra = " (%.2f ps a trio-word)" % (1e9 * t[key][len(runs) // 2] / words) if key == "trio_ms" else ""
            say("  %s  device ms over %d calls: best %.3f median %.3f%s" % (name, args.repeat, t[key][0], t[key][len(runs) // 2], extra))
        pk = dict(max_pair_err=1.0, max_trio_err=0.03, min_shared=1, max_candidates=C, top=2)
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            dev = tf.parentage(calls, names, device=args.device, **pk)
            walls.append(time.perf_counter() - t0)
        say("  wall: parentage(backend='gpu') from a host matrix, relate_joint included: %s s (kernels %.3f ms)" % (
            " ".join("%.3f" % w for w in walls), dev.stats["ms"]))
        if args.no_host:
            say("  wall: parentage(backend='host'): not measured")
            continue
        t0 = time.perf_counter()
        host = tf.parentage(calls, names, backend="host", **pk)
        t_host = time.perf_counter() - t0
        if any(getattr(dev, k) != getattr(host, k) for k in ("offspring", "status", "trios", "passes", "single", "candidates")):
            raise SystemExit("device and host results differ at %s" % case)
        say("  wall: parentage(backend='host') %.3f s with %s CPUs; device and host agree on every status, trio and count" % (
            t_host, os.environ.get("OMP_NUM_THREADS", "all")))
    say()
    say("what bounds k_par_trios: not measured (no counter run was made)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
