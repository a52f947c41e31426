#!/usr/bin/env python3
"""Measures the pairwise sample relations (sample_relations, csrc/relate.hip) on one GPU and writes
profiles/relate/bench_mi355x.txt.

    python tools/relate_bench.py [--clock-ghz F] [--host-markers 200000] [--out FILE]

Calls resident on the device, device time by HIP events around k_relate (what td_relate_joint reports), best and median
of --repeat calls after a warm-up of the same shape:
(a) 384 samples x 10^6 markers, all passing     (b) the same with every second marker masked
(c) 10 000 x 1 000                              (d) 96 x 50 000
Next to each time the two floors: the S M bytes of the calls at the 6.29 TB/s a copy kernel reaches on this card
(DESIGN 4.2), and the multiply-adds the kernel issues (192 x 192 x 64 per tile pair and 64-marker step, masked markers
and the padding of a tile included) at the int8 MFMA rate, 1024 multiply-adds per clock and SIMD = twice bf16, on 1024
SIMDs at --clock-ghz: the clock the chip holds under this kernel as tools/relate_clock.hip measures it (without the
option the floor is printed at the 2.4 GHz of the specification and marked so).
(e) 384 x --host-markers from a host matrix: wall time of sample_relations(backend="gpu") (upload, kernel, table back,
    derived arrays) against backend="host" on this machine's CPUs; the two tables are compared before a time is printed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tagdigger_amd import tagdigger_fun as tf                              # noqa: E402
from tagdigger_amd.engine import RELATE_KCHUNK, RELATE_TILE, default_engine  # noqa: E402

COPY_RATE = 6.29e12          # bytes/s of a copy kernel on this card
MAC_PER_CLOCK = 1024 * 1024  # int8 MFMA: 32 x 32 x 32 in 32 cycles per SIMD, 4 SIMDs on each of 256 CUs
PATTERNS = 16                # distinct sample rows; row s of the matrix is pattern s % PATTERNS


def pattern_rows(rng, M):
    """PATTERNS rows of M calls: per marker an allele frequency, per sample a genotype drawn from it, 15 % missing."""
    freq = rng.random(M)
    rows = np.zeros((PATTERNS, M), dtype=np.uint8)
    for r in range(PATTERNS):
        rows[r] = (rng.random(M) < freq).astype(np.uint8) + (rng.random(M) < freq)
        rows[r][rng.random(M) < 0.15] = 3
    return rows


def upload(eng, rows, S):
    M = rows.shape[1]
    d = eng.dev_alloc(S * M)
    for s in range(S):
        eng.h2d(d + s * M, rows[s % PATTERNS].tobytes())
    return d


def issued_macs(S, M):
    tiles = -(-S // RELATE_TILE)
    steps = (M // RELATE_KCHUNK) * (RELATE_KCHUNK // 64) + -(-(M % RELATE_KCHUNK) // 64)
    return tiles * (tiles + 1) // 2 * steps * (3 * RELATE_TILE) ** 2 * 64


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clock-ghz", type=float, default=None, help="core clock under this kernel (tools/relate_clock.hip)")
    ap.add_argument("--host-markers", type=int, default=200000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relate", "bench_mi355x.txt"))
    args = ap.parse_args(argv)
    eng = default_engine(args.device)
    rng = np.random.default_rng(4150)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    clock = args.clock_ghz or 2.4
    say("sample relations, tools/relate_bench.py; TILE %d KCHUNK %d; device ms: HIP events around k_relate inside td_relate_joint" % (
        RELATE_TILE, RELATE_KCHUNK))
    say("MFMA floor at %.3f GHz %s" % (clock, "(measured under this kernel, tools/relate_clock.hip)" if args.clock_ghz else
                                       "(the specification's clock: the clock under load was NOT measured)"))

    def measure(label, d, S, M, use):
        eng.relate_joint(d, shape=(S, M), use=use, fetch=False)                 # warm-up at this shape
        ms = sorted(eng.relate_joint(d, shape=(S, M), use=use, fetch=False).ms for _ in range(args.repeat))
        best, med = ms[0], ms[len(ms) // 2]
        f_bytes = S * M / COPY_RATE * 1e3
        macs = issued_macs(S, M)
        f_mfma = macs / (MAC_PER_CLOCK * clock * 1e9) * 1e3
        tiles = -(-S // RELATE_TILE)
        say("%s: %d x %d, %d workgroups" % (label, S, M, tiles * (tiles + 1) // 2 * -(-M // RELATE_KCHUNK)))
        say("  device ms over %d calls: best %.3f median %.3f" % (len(ms), best, med))
        say("  floor, calls read once: %.3f GB at 6.29 TB/s = %.4f ms -> %.1f %% of it reached (median)" % (
            S * M / 1e9, f_bytes, 100 * f_bytes / med))
        say("  floor, MFMA: %.3e multiply-adds issued = %.4f ms -> %.1f %% of it reached (median); %.1f int8 TOP/s" % (
            macs, f_mfma, 100 * f_mfma / med, 2 * macs / (med * 1e-3) / 1e12))
        return med

    S, M = 384, 1000000
    rows = pattern_rows(rng, M)
    d = upload(eng, rows, S)
    try:
        measure("(a) all markers pass", d, S, M, None)
        half = (np.arange(M) % 2 == 0).astype(np.uint8)
        measure("(b) every second marker masked", d, S, M, half)
        measure("(d) one plate", d, 96, 50000, None)                             # the first 96 x 50 000 bytes as a matrix of its own
        small = np.frombuffer(eng.d2h(d, 96 * 50000), dtype=np.uint8).reshape(96, 50000)
        same = np.array_equal(eng.relate_joint(d, shape=(96, 50000)).joint, tf._relations_host(small))
        say("  device and host tables of (d) agree: %s" % same)
        if not same:
            raise SystemExit("(d) device and host results differ")
    finally:
        eng.dev_free(d)
    S2, M2 = 10000, 1000
    d = upload(eng, pattern_rows(rng, M2), S2)
    try:
        measure("(c) many samples, few markers", d, S2, M2, None)
        say("  (the table itself is 9 S^2 4 = %.1f GB, zeroed before and written by atomics in the kernel)" % (9 * S2 * S2 * 4 / 1e9))
    finally:
        eng.dev_free(d)

    say()
    Mh = args.host_markers
    host_matrix = np.ascontiguousarray(rows[np.arange(384) % PATTERNS][:, :Mh])
    names = ["s%d" % s for s in range(384)]
    t0 = time.perf_counter()
    host = tf.sample_relations(host_matrix, names, backend="host")
    t_host = time.perf_counter() - t0
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        dev = tf.sample_relations(host_matrix, names, backend="gpu", device=args.device)
        walls.append(time.perf_counter() - t0)
    if not np.array_equal(dev.joint, host.joint) or dev.duplicates != host.duplicates:
        raise SystemExit("(e) device and host results differ")
    say("(e) 384 x %d from a host matrix: device and host agree on the table and on %d duplicate pairs" % (Mh, len(host.duplicates)))
    say("  wall: sample_relations(backend='gpu') %s s (check of the codes, upload, kernel %.3f ms, table back, derived arrays); "
        "backend='host' %.3f s with %s CPUs" % (" ".join("%.3f" % w for w in walls), dev.stats["ms"], t_host,
                                                  os.environ.get("OMP_NUM_THREADS", "all")))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
