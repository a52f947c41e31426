#!/usr/bin/env python3
"""Measures polyploid dosage calling (call_dosage, csrc/dosage.hip) on one GPU and writes profiles/dosage/bench_mi355x.txt.

    python tools/dosage_bench.py [--samples 384] [--tags 2000000] [--out FILE]

Synthetic counts of --samples x --tags uint32 resident on the device (tools/genocall_bench.py's matrix), markers at
adjacent columns, calls left on the device.  For P = 2, 4, 6, 8 and both priors: device time by HIP events (what
td_dose_call reports, best and median of --repeat calls after a warm-up), its ratio to td_geno_call over the same
matrix in the same run, and the bytes the rule has to move -- S T 4 read (twice with the HWE prior: the depth pass) + S M
written, 2 S M with the diploidised buffer -- over that time.  The bytes do not change with P, the arithmetic does (P + 1
costs of two 64-bit multiply-adds per cell): the change of time from P = 2 to P = 8 says which of the two bounds the
kernel."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from genocall_bench import COPY_RATE, pattern_rows, upload   # noqa: E402
from tagdigger_amd import tagdigger_fun as tf                # noqa: E402
from tagdigger_amd.engine import default_engine              # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=384)
    ap.add_argument("--tags", type=int, default=2000000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dosage", "bench_mi355x.txt"))
    args = ap.parse_args(argv)
    eng = default_engine(args.device)
    rng = np.random.default_rng(20260)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    S, T = args.samples, args.tags - args.tags % 2
    M = T // 2
    say("dosage calling, tools/dosage_bench.py --samples %d --tags %d: %d markers at adjacent columns, calls left on the device" % (S, T, M))
    say("device ms: HIP events around the kernels inside td_dose_call / td_geno_call; best and median of %d calls after a warm-up" % args.repeat)
    rows = pattern_rows(rng, T)
    i0, i1 = np.arange(0, T, 2, dtype=np.uint32), np.arange(1, T, 2, dtype=np.uint32)
    filters = dict(min_depth=2, min_call_ppm=800000, min_maf_ppm=50000)
    d = upload(eng, rows, S)
    try:
        def geno():
            return eng.geno_call(d, i0, i1, tf.het_threshold_table(0.01), shape=(S, T), fetch_calls=False, **filters)

        def dose(P, prior, diploid=False):
            CA, CB, CP = tf.dosage_tables(P, 0.01)
            return eng.dose_call(d, i0, i1, CA, CB, CP if prior else None, shape=(S, T), ploidy=P, prior=prior, fetch_calls=False,
                                 diploid=diploid, min_margin=tf.dosage_margin(10), **filters)

        def timed(fn):
            fn()                                           # warm-up: module load, first full-size call
            ms = sorted(fn().ms for _ in range(args.repeat))
            return ms[0], ms[len(ms) // 2]

        g_best, g_med = timed(geno)
        g_bytes = S * T * 4 + S * M
        say("td_geno_call (likelihood rule): best %.3f median %.3f ms; %.3f GB (S T 4 + S M) = %.2f TB/s at the median" % (
            g_best, g_med, g_bytes / 1e9, g_bytes / (g_med * 1e-3) / 1e12))
        say("P  prior diploid  best ms  median ms  / geno   GB moved  TB/s at the median  (% of the copy rate 6.29 TB/s)   passed")
        for P in (2, 4, 6, 8):
            for prior in (0, 1):
                for diploid in (False, True) if P in (4, 8) else (False,):
                    best, med = timed(lambda: dose(P, prior, diploid))
                    moved = S * T * 4 * (2 if prior else 1) + S * M * (2 if diploid else 1)
                    say("%d  %-5s %-7s  %7.3f  %9.3f  %6.2f  %9.3f  %6.2f (%.0f %%)   %d" % (
                        P, ("flat", "hwe")[prior], ("no", "yes")[diploid], best, med, med / g_med, moved / 1e9,
                        moved / (med * 1e-3) / 1e12, 100 * moved / (med * 1e-3) / COPY_RATE, dose(P, prior, diploid).passed))
    finally:
        eng.dev_free(d)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
