#!/usr/bin/env python3
"""Measures the pairwise marker LD (marker_ld, csrc/ld.hip) on one GPU and writes profiles/ld/bench_mi355x.txt.

    python tools/ld_bench.py [--clock-ghz F] [--host-shape 2000x5000] [--out FILE]

Calls resident on the device, structured as in tests/ld_cases.py (8 founder columns, every marker a copy of one with
10 % of its cells redrawn and 10 % missing), thresholds min_r2 0.8 and min_shared 50 (10 where there are 96 samples;
min_r2 0.5 at 2 000 samples, where no pair of this generator reaches 0.8).
Per kernel, device time by HIP events inside td_ld_pairs, best and median of --repeat calls after a warm-up of the same
shape: the transpose pre-pass, the pair kernel; and the host's sort of the edges (wall time inside the library):
(a) 384 x 50 000        (b) 96 x 20 000        (c) 2 000 x 5 000
Next to the pair kernel its floor: the multiply-adds it issues (6 products of 64 x 64 x 64 per tile pair and 64-sample
step, the padding of tiles and steps included) at the int8 MFMA rate, 1024 multiply-adds per clock and SIMD, on 1024
SIMDs at --clock-ghz (the clock tools/relate_clock.hip reads under k_relate, which issues the same instruction; without
the option the floor is printed at the 2.4 GHz of the specification and marked so).  A second run of each shape with
min_r2 = 1 and min_shared above S leaves the epilogue nothing past its first exit: the difference between the two is
what the epilogue's decisions and edges cost.
(d) --host-shape from a host matrix: wall time of marker_ld(backend="gpu") (check of the codes, upload, both kernels,
    edges back, sort, r^2) against backend="host" on this machine's CPUs; the edges are compared before a time is printed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tagdigger_amd import tagdigger_fun as tf                    # noqa: E402
from tagdigger_amd.engine import LD_TILE, default_engine         # noqa: E402

MAC_PER_CLOCK = 1024 * 1024  # int8 MFMA: 32 x 32 x 32 in 32 cycles per SIMD, 4 SIMDs on each of 256 CUs


def structured(rng, S, M):
    founders = rng.integers(0, 3, size=(S, 8), dtype=np.uint8)
    C = founders[:, rng.integers(0, 8, size=M)].copy()
    noise = rng.random((S, M)) < 0.1
    C[noise] = rng.integers(0, 3, size=int(noise.sum()), dtype=np.uint8)
    C[rng.random((S, M)) < 0.1] = 3
    return C


def issued_macs(S, M):
    tiles, steps = -(-M // LD_TILE), -(-S // 64)
    return tiles * (tiles + 1) // 2 * steps * 6 * LD_TILE * LD_TILE * 64


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clock-ghz", type=float, default=None, help="core clock under the int8 MFMA loop (tools/relate_clock.hip)")
    ap.add_argument("--host-shape", default="2000x5000")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ld", "bench_mi355x.txt"))
    args = ap.parse_args(argv)
    eng = default_engine(args.device)
    rng = np.random.default_rng(4160)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    clock = args.clock_ghz or 2.4
    say("marker LD, tools/ld_bench.py; TILE %d; device ms: HIP events around k_calls_transpose<true> and k_ld_pairs inside td_ld_pairs" % LD_TILE)
    say("MFMA floor at %.3f GHz %s" % (clock, "(measured under k_relate's int8 MFMA loop, tools/relate_clock.hip)" if args.clock_ghz else
                                       "(the specification's clock: the clock under load was NOT measured)"))

    def runs(d, S, M, ppm, min_shared):
        n = eng.ld_pairs(d, shape=(S, M), min_r2_ppm=ppm, min_shared=min_shared, count_only=True).n   # warm-up, and the buffer's size
        out = [eng.ld_pairs(d, shape=(S, M), min_r2_ppm=ppm, min_shared=min_shared, capacity=n, retry=False) for _ in range(args.repeat)]
        cols = {k: sorted(r.times[k] for r in out) for k in ("transpose_ms", "pairs_ms", "sort_ms")}
        return out[0].n, {k: (v[0], v[len(v) // 2]) for k, v in cols.items()}

    def measure(label, S, M, min_shared, min_r2=0.8):
        calls = structured(rng, S, M)
        d = eng.dev_alloc(S * M)
        try:
            eng.h2d(d, calls.tobytes())
            n, t = runs(d, S, M, int(round(min_r2 * 1e6)), min_shared)
            n0, t0 = runs(d, S, M, 1000000, S + 1)
        finally:
            eng.dev_free(d)
        tiles = -(-M // LD_TILE)
        macs = issued_macs(S, M)
        f_mfma = macs / (MAC_PER_CLOCK * clock * 1e9) * 1e3
        say("%s: %d x %d, %d tile pairs, %d edges of %d pairs at min_r2 %.1f, min_shared %d" % (
            label, S, M, tiles * (tiles + 1) // 2, n, M * (M - 1) // 2, min_r2, min_shared))
        say("  transpose pre-pass  device ms over %d calls: best %.3f median %.3f (%.1f MB written)" % (
            args.repeat, t["transpose_ms"][0], t["transpose_ms"][1], tiles * LD_TILE * -(-S // 64) * 64 / 1e6))
        say("  pair kernel         device ms over %d calls: best %.3f median %.3f" % (args.repeat, t["pairs_ms"][0], t["pairs_ms"][1]))
        say("  pair kernel, no pair past the first exit (min_shared %d): best %.3f median %.3f, %d edges" % (
            S + 1, t0["pairs_ms"][0], t0["pairs_ms"][1], n0))
        say("  floor, MFMA: %.3e multiply-adds issued = %.4f ms -> %.1f %% of it reached (median); %.1f int8 TOP/s" % (
            macs, f_mfma, 100 * f_mfma / t["pairs_ms"][1], 2 * macs / (t["pairs_ms"][1] * 1e-3) / 1e12))
        say("  sort of the edges on the host, wall ms: best %.3f median %.3f" % t["sort_ms"])

    measure("(a)", 384, 50000, 50)
    measure("(b) one plate", 96, 20000, 10)
    measure("(c) many samples", 2000, 5000, 50, 0.5)

    say()
    S, M = (int(x) for x in args.host_shape.split("x"))
    matrix = structured(rng, S, M)
    names = ["m%d" % m for m in range(M)]
    t0 = time.perf_counter()
    host = tf.marker_ld(matrix, names, min_r2=0.5, backend="host")
    t_host = time.perf_counter() - t0
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        dev = tf.marker_ld(matrix, names, min_r2=0.5, backend="gpu", device=args.device)
        walls.append(time.perf_counter() - t0)
    if dev.edges.tobytes() != host.edges.tobytes() or not np.array_equal(dev.degree, host.degree) or not np.array_equal(dev.called, host.called):
        raise SystemExit("(d) device and host results differ")
    say("(d) %d x %d from a host matrix at min_r2 0.5: device and host agree on %d edges, the degrees and the called counts" % (
        S, M, len(host.edges)))
    say("  wall: marker_ld(backend='gpu') %s s (check of the codes, upload, kernels %.3f ms, edges back, sort, r^2); "
        "backend='host' %.3f s with %s CPUs" % (" ".join("%.3f" % w for w in walls), dev.stats["ms"], t_host,
                                                  os.environ.get("OMP_NUM_THREADS", "all")))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
