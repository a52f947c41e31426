#!/usr/bin/env python3
"""Measures genotype calling (call_genotypes, csrc/genocall.hip) on one GPU and writes profiles/genocall/bench_mi355x.txt.

    python tools/genocall_bench.py [--samples 384] [--tags 2000000] [--host-markers 200000] [--out FILE]

(a) synthetic counts of --samples x --tags uint32 resident on the device, markers at adjacent columns (census_markers'
    layout): kernel time by HIP events (what td_geno_call reports), with the calls left on the device, and the bytes the
    rule has to move, S T 4 read + S M written, over that time -- next to the 6.29 TB/s a copy kernel reaches on this
    card
(b) the first --host-markers markers of the same matrix: wall time of call_genotypes(backend="gpu") from a host matrix
    (upload, kernels, calls back) against backend="host"; the two results are compared before any time is printed
(c) 1 000 markers x 10 000 samples once: few markers, many sample chunks
(d) the first 1 024 .. 262 144 markers of (a)'s matrix: device time against the number of markers
Device time is what the library measures with HIP events around its two kernels; wall time is the clock around the call."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tagdigger_amd import tagdigger_fun as tf          # noqa: E402
from tagdigger_amd.engine import default_engine        # noqa: E402

COPY_RATE = 6.29e12          # bytes/s of a copy kernel on this card
PATTERNS = 16                # distinct sample rows; row s of the matrix is pattern s % PATTERNS


def pattern_rows(rng, T):
    """PATTERNS rows of T counts: per marker (two adjacent columns) an allele frequency, per sample a genotype drawn from
    it and a depth (a tenth of the cells empty, most between 1 and 60 reads, one in fifty between 128 and 5 000)."""
    M = T // 2
    freq = rng.random(M)
    rows = np.zeros((PATTERNS, T), dtype=np.uint32)
    for r in range(PATTERNS):
        dose = (rng.random(M) < freq).astype(np.int64) + (rng.random(M) < freq)
        depth = rng.geometric(0.08, M)
        depth[rng.random(M) < 0.1] = 0
        deep = rng.random(M) < 0.02
        depth[deep] = rng.integers(128, 5001, int(deep.sum()))
        b = rng.binomial(depth, np.array([0.01, 0.5, 0.99])[dose])
        rows[r, 0:2 * M:2] = depth - b
        rows[r, 1:2 * M:2] = b
    return rows


def upload(eng, rows, S):
    """The S x T matrix (row s = rows[s % PATTERNS]) in device memory."""
    T = rows.shape[1]
    d = eng.dev_alloc(S * T * 4)
    for s in range(S):
        eng.h2d(d + s * T * 4, rows[s % PATTERNS].tobytes())
    return d


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=384)
    ap.add_argument("--tags", type=int, default=2000000)
    ap.add_argument("--host-markers", type=int, default=200000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "genocall", "bench_mi355x.txt"))
    args = ap.parse_args(argv)
    eng = default_engine(args.device)
    rng = np.random.default_rng(20260)
    table = tf.het_threshold_table(0.01)
    par = dict(min_depth=2, min_call_ppm=800000, min_maf_ppm=50000)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    S, T = args.samples, args.tags - args.tags % 2
    M = T // 2
    say("genotype calling, tools/genocall_bench.py --samples %d --tags %d --host-markers %d" % (S, T, args.host_markers))
    say("device ms: HIP events around k_gc_call + k_gc_filter inside td_geno_call; rates are bytes the rule must move over that time")
    rows = pattern_rows(rng, T)
    i0, i1 = np.arange(0, T, 2, dtype=np.uint32), np.arange(1, T, 2, dtype=np.uint32)

    def timed(d, S, T, i0, i1, repeat, **kw):
        return [eng.geno_call(d, i0, i1, table, shape=(S, T), fetch_calls=False, **dict(par, **kw)) for _ in range(repeat)]

    # (a) the full matrix, resident
    d = upload(eng, rows, S)
    try:
        eng.geno_call(d, i0[:1024], i1[:1024], table, shape=(S, T), fetch_calls=False, **par)      # warm-up: module load
        for rule in (0, 1):
            runs = timed(d, S, T, i0, i1, args.repeat + 1, rule=rule)[1:]                          # the first full-size call warms up too
            ms = sorted(r.ms for r in runs)
            moved = S * T * 4 + S * M
            say("(a) %s rule, %d samples x %d tags, %d markers at adjacent columns: passed %d" % (
                ("likelihood", "presence")[rule], S, T, M, runs[0].passed))
            say("  device ms over %d calls: min %.3f median %.3f max %.3f" % (len(ms), ms[0], ms[len(ms) // 2], ms[-1]))
            say("  bytes moved %.3f GB (S T 4 + S M): %.2f TB/s at the median = %.0f %% of the copy rate 6.29 TB/s, %.0f %% of 8 TB/s" % (
                moved / 1e9, moved / (ms[len(ms) // 2] * 1e-3) / 1e12, 100 * moved / (ms[len(ms) // 2] * 1e-3) / COPY_RATE,
                100 * moved / (ms[len(ms) // 2] * 1e-3) / 8e12))
        # fewer markers of the same matrix
        say("(d) the first M markers of that matrix, likelihood rule: M, device ms (median of %d)" % args.repeat)
        for Md in (1024, 4096, 16384, 65536, 262144):
            if Md > M:
                break
            ms = sorted(r.ms for r in timed(d, S, T, i0[:Md], i1[:Md], args.repeat + 1)[1:])
            say("  %7d  %.4f" % (Md, ms[len(ms) // 2]))
        # the same markers under a random permutation of their order (columns no longer adjacent between neighbours)
        perm = rng.permutation(M)
        runs = timed(d, S, T, i0[perm], i1[perm], 3)[1:]
        say("(a') markers in random order (a wave's loads scatter over the row): device ms %s" % " ".join("%.3f" % r.ms for r in runs))
    finally:
        eng.dev_free(d)

    # (b) against the host backend, on the first --host-markers markers
    say()
    Mh = min(M, args.host_markers)
    host_matrix = rows[np.arange(S) % PATTERNS][:, :2 * Mh]
    names = [n for m in range(Mh) for n in ("M%07d_0" % m, "M%07d_1" % m)]
    samples = ["s%d" % s for s in range(S)]
    kw = dict(min_depth=2, min_call_rate=0.8, min_maf=0.05)
    t0 = time.perf_counter()
    host = tf.call_genotypes(host_matrix, samples, names, backend="host", **kw)
    t_host = time.perf_counter() - t0
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        dev = tf.call_genotypes(host_matrix, samples, names, backend="gpu", device=args.device, **kw)
        walls.append(time.perf_counter() - t0)
    same = (np.array_equal(dev.calls, host.calls) and np.array_equal(dev.mask, host.mask) and
            all(np.array_equal(dev.stats[k], host.stats[k]) for k in tf.GENO_STATS))
    if not same:
        raise SystemExit("(b) device and host results differ")
    say("(b) %d samples x %d markers from a host matrix: device and host agree on calls, statistics and mask (passed %d)" % (
        S, Mh, host.stats["passed"]))
    say("  wall: call_genotypes(backend='gpu') %s s (name handling, upload, kernels %.3f ms, calls back); backend='host' %.3f s" % (
        " ".join("%.3f" % w for w in walls), dev.stats["ms"], t_host))

    # (c) few markers, many samples: the sample-chunk path
    say()
    S2, M2 = 10000, 1000
    rows2 = pattern_rows(rng, 2 * M2)
    d = upload(eng, rows2, S2)
    try:
        j0, j1 = np.arange(0, 2 * M2, 2, dtype=np.uint32), np.arange(1, 2 * M2, 2, dtype=np.uint32)
        r = timed(d, S2, 2 * M2, j0, j1, 1)[0]
        moved = S2 * 2 * M2 * 4 + S2 * M2
        say("(c) %d samples x %d markers, once: device ms %.3f, %.3f GB moved, %.2f TB/s; passed %d" % (
            S2, M2, r.ms, moved / 1e9, moved / (r.ms * 1e-3) / 1e12, r.passed))
    finally:
        eng.dev_free(d)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
