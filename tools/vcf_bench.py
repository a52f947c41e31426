#!/usr/bin/env python3
"""Measures the VCF export (writeVCF, csrc/vcf.hip) on one GPU and writes profiles/vcf/bench_mi355x.txt.

    python tools/vcf_bench.py [--samples 384] [--tags 2000000 100000] [--tmp /dev/shm] [--out FILE]

Synthetic counts of --samples x tags uint32 resident on the device (tools/genocall_bench.py's matrix), markers at
adjacent columns, the calls where td_geno_call left them, every marker a line with a prefix of the size writeVCF builds.
Per size: the device ms of the measure, scan and emit kernels by HIP events (what td_vcf_file reports; emit is the sum
over the ranges), median of --repeat calls after a warm-up; the bytes of the text and the emit kernel's bytes per second;
td_geno_call's ms over the same matrix in the same run; the wall time of the file route to a path under --tmp with the
wall ms it spent in write().  Then writeVCF(backend="host") over 384 x --host-markers markers, wall time."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from genocall_bench import PATTERNS, pattern_rows, upload    # noqa: E402
from tagdigger_amd import tagdigger_fun as tf                # noqa: E402
from tagdigger_amd.engine import default_engine              # noqa: E402


def prefixes(M, fmt):
    """(bytes, offsets) of M prefixes as writeVCF builds them without positions."""
    parts = [("0\t%d\tMk%07d\tN\t<ALLELE1>\t.\tPASS\tNS=%d;DP=%d;AC=%d;AN=%d\t%s" % (m + 1, m, 300 + m % 80, 9000 + m % 977, m % 600,
                                                                                      600 + 2 * (m % 80), fmt)).encode("ascii") for m in range(M)]
    off = np.zeros(M + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return b"".join(parts), off


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=384)
    ap.add_argument("--tags", type=int, nargs="+", default=[2000000, 100000])
    ap.add_argument("--host-markers", type=int, default=50000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--tmp", default="/dev/shm", help="a tmpfs directory for the file route")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf", "bench_mi355x.txt"))
    args = ap.parse_args(argv)
    eng = default_engine(args.device)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    S = args.samples
    CA, CB, _ = tf.dosage_tables(2, 0.01)
    path = os.path.join(args.tmp, "vcf_bench_%d.vcf" % os.getpid())
    say("VCF export, tools/vcf_bench.py --samples %d --tags %s: markers at adjacent columns, every marker a line, matrix and calls resident" % (
        S, " ".join(str(t) for t in args.tags)))
    say("device ms: HIP events around the kernels inside td_vcf_file (emit: summed over the ranges of 256 MiB); median of %d calls after a "
        "warm-up; the file goes to %s" % (args.repeat, args.tmp))
    say("tags      cells       form            measure ms  scan ms  emit ms   text GB  emit GB/s  geno_call ms  ranges  file wall s  in write() s")
    try:
        for tags in args.tags:
            T = tags - tags % 2
            M = T // 2
            rows = pattern_rows(np.random.default_rng(20260), T)
            i0, i1 = np.arange(0, T, 2, dtype=np.uint32), np.arange(1, T, 2, dtype=np.uint32)
            sel = np.arange(M, dtype=np.uint32)
            d = upload(eng, rows, S)
            d_calls = None
            try:
                def geno(keep=False):
                    return eng.geno_call(d, i0, i1, tf.het_threshold_table(0.01), shape=(S, T), fetch_calls=False, keep_device=keep, min_depth=2)
                geno()
                g_ms = median([geno().ms for _ in range(args.repeat)])
                d_calls = geno(keep=True).d_calls
                for lik in (False, True) if tags == min(args.tags) else (False,):
                    pre = prefixes(M, "GT:AD:DP:GQ:PL" if lik else "GT:AD:DP")

                    def to_file():
                        t0 = time.perf_counter()
                        res = eng.vcf_file(path, d, d_calls, i0, i1, sel, pre, shape=(S, T), ploidy=2, likelihoods=lik, ca=CA, cb=CB)
                        return res, time.perf_counter() - t0
                    to_file()
                    runs = [to_file() for _ in range(args.repeat)]
                    res = runs[0][0]
                    assert os.path.getsize(path) == res.nbytes
                    ms = {k: median([r.ms[k] for r, _ in runs]) for k in ("measure", "scan", "emit", "write")}
                    say("%-9d %-11d %-15s %10.3f  %7.3f  %7.3f  %8.3f  %9.1f  %12.3f  %6d  %11.3f  %12.3f" % (
                        T, S * M, "GT:AD:DP:GQ:PL" if lik else "GT:AD:DP", ms["measure"], ms["scan"], ms["emit"], res.nbytes / 1e9,
                        res.nbytes / (ms["emit"] * 1e-3) / 1e9, g_ms, res.ranges, median([w for _, w in runs]), ms["write"] / 1e3))
            finally:
                if d_calls:
                    eng.dev_free(d_calls)
                eng.dev_free(d)
    finally:
        if os.path.exists(path):
            os.remove(path)
    # the host backend
    M = args.host_markers
    rows = pattern_rows(np.random.default_rng(20260), 2 * M)
    counts = rows[np.arange(S) % PATTERNS]
    names = [n for m in range(M) for n in ("Mk%07d_0" % m, "Mk%07d_1" % m)]
    result = tf.call_genotypes(counts, ["s%03d" % s for s in range(S)], names, backend="host", min_depth=2)
    try:
        t0 = time.perf_counter()
        info = tf.writeVCF(path, result, counts, passing_only=False, backend="host")
        wall = time.perf_counter() - t0
    finally:
        if os.path.exists(path):
            os.remove(path)
    say("")
    say("writeVCF(backend=\"host\"), %d x %d markers (numpy and Python strings): %.1f s wall for %.3f GB = %.3f GB/s, %.1f M cells/s" % (
        S, M, wall, info["bytes"] / 1e9, info["bytes"] / wall / 1e9, S * M / wall / 1e6))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
