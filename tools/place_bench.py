#!/usr/bin/env python3
"""Measures tag placement (csrc/place.hip) on one GPU and writes profiles/place/bench_mi355x.txt.

    python tools/place_bench.py [--gb 3] [--tags 1000000] [--k 2] [--reps 5] [--out profiles/place/bench_mi355x.txt]

The genome is the synthetic one of tools/fragsize_bench.py (12 chromosomes of random ACGT), built in host memory and
uploaded as td_fasta_frame_device would leave it; the tags are 64 bases, half cut from the genome's windows with 0..2
substitutions, half random behind the remnant.  Device time per kernel is what td_place_sites and td_place_tags measure
with HIP events, best and median of --reps after one warm-up.  The site scan is set beside its floor, len(G) bytes at
the 6.29 TB/s copy rate of DESIGN 4.2.  The join is timed three times: on the plain genome (short runs), on one with a
window planted 100 000 times (the dedupe makes it one compare per tag), and on one with --family windows that share part
0, so that a tenth of the genome's tags compare with all of them (long runs: the rate the compare cap is set from).  The command line is timed against --td-backend host on a 30 MB genome."""
import argparse
import collections
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBS = 6.29
ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)


FAMILY_HEAD = 21                      # bases a planted family shares: part 0 of k = 2 over 64 bases


def genome(nbytes, nchrom, seed, repeat=0, family=0):
    """(uint8 array, rec_start).  `repeat` copies of one 64-base window behind TGCAG are planted 1 000 bases apart; or
    `family` windows that share their first FAMILY_HEAD bases and differ behind them (one long run of part 0)."""
    rng = np.random.default_rng(seed)
    g = ALPHA[rng.integers(0, 4, nbytes, dtype=np.uint8)]
    if repeat or family:
        w = np.concatenate([np.frombuffer(b"TGCAG", dtype=np.uint8), ALPHA[rng.integers(0, 4, 59, dtype=np.uint8)]])
        for i in range(repeat):
            g[1000 * i + 100:1000 * i + 164] = w
        for i in range(family):
            g[1000 * i + 100:1000 * i + 100 + FAMILY_HEAD] = w[:FAMILY_HEAD]
    clen = nbytes // nchrom
    return g, [c * clen for c in range(nchrom)] + [nbytes]


def upload(eng, g):
    d = eng.dev_alloc(len(g) + 16)
    step = 256 << 20
    for lo in range(0, len(g), step):
        eng.h2d(d + lo, g[lo:lo + step].tobytes())
    return d


def make_tags(rng, windows, ntags):
    half = ntags // 2
    pick = rng.integers(0, len(windows), half)
    tags = np.array([np.frombuffer(windows[i].encode(), dtype=np.uint8) for i in pick])
    for row in tags:
        for _ in range(int(rng.integers(0, 3))):
            row[int(rng.integers(0, 64))] = ALPHA[int(rng.integers(0, 4))]
    rand = ALPHA[rng.integers(0, 4, (ntags - half, 64), dtype=np.uint8)]
    rand[:, :5] = np.frombuffer(b"TGCAG", dtype=np.uint8)
    return np.vstack([tags, rand]).tobytes()


def best_median(rows, keys):
    return {k: (min(r[k] for r in rows), statistics.median(r[k] for r in rows)) for k in keys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=3.0)
    ap.add_argument("--tags", type=int, default=1_000_000)
    ap.add_argument("--chrom", type=int, default=12)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--family", type=int, default=200_000, help="windows of the planted long run")
    ap.add_argument("--cli-mb", type=float, default=30.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place", "bench_mi355x.txt"))
    args = ap.parse_args()
    from tagdigger_amd import Engine
    from tagdigger_amd.engine import PLACE_MS, PLACED_MS
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("tag placement, csrc/place.hip: genome %.2f GB in %d records, %d tags of 64 bases, k = %d; HIP-event ms, best / median of %d after warm-up"
        % (args.gb, args.chrom, args.tags, args.k, args.reps))
    eng = Engine(0)
    nbytes = int(args.gb * 1e9)
    rng = np.random.default_rng(7)
    for label, repeat, family in (("short runs", 0, 0), ("a window planted 100 000 times", 100_000, 0),
                                  ("long runs: %d windows that share part 0" % args.family, 0, args.family)):
        g, rec_start = genome(nbytes, args.chrom, 1, repeat, family)
        head = g[100:100 + FAMILY_HEAD].tobytes().decode()
        d = upload(eng, g)
        del g
        rows = []
        for _ in range(args.reps + 1):
            place = eng.place_sites(d, nbytes, rec_start, ["TGCAG"], 64)
            rows.append(place.ms)
            if len(rows) <= args.reps:
                place.close()
        eng.dev_free(d)
        bm = best_median(rows[1:], PLACE_MS)
        say("%s: %s" % (label, " ".join("%s=%d" % kv for kv in place.stats.items())))
        say("  sites   " + "  ".join("%s %.3f / %.3f" % ((k,) + bm[k]) for k in PLACE_MS))
        floor = nbytes / (COPY_TBS * 1e12) * 1e3
        say("  site scan: count + emit best %.3f ms for two passes over %d bytes; floor of one pass %.3f ms at %.2f TB/s"
            % (bm["count"][0] + bm["emit"][0], nbytes, floor, COPY_TBS))
        windows = eng.place_loci(place, windows=True)[3]
        if repeat:
            top = collections.Counter(windows).most_common(1)[0][0]        # a tenth of the genome's tags come from the repeat
            windows = windows + [top] * (len(windows) // 9)
        if family:                                                            # a tenth of the genome's tags come from the family
            fam = [w for w in windows if w.startswith(head)]
            rest = [w for w in windows if not w.startswith(head)]
            windows = rest + fam * max(1, len(rest) // (9 * len(fam)))
        tags = make_tags(rng, windows, args.tags)
        first = eng.place_tags(place, tags, args.tags, args.k)
        rows = [eng.place_tags(place, tags, args.tags, args.k)[4] for _ in range(args.reps)]
        bm = best_median(rows, PLACED_MS)
        st = first[3]
        say("  tags    " + " ".join("%s=%d" % kv for kv in st.items()))
        say("  first call (builds the parts' tables): " + "  ".join("%s %.3f" % (k, first[4][k]) for k in PLACED_MS))
        say("  later   " + "  ".join("%s %.3f / %.3f" % ((k,) + bm[k]) for k in PLACED_MS))
        say("  join: %d compares in %.3f ms best = %.3g compares / s" % (st["compares"], bm["join"][0], st["compares"] / (bm["join"][0] * 1e-3)))
        place.close()
    eng.close()
    # ---- the command line against the host backend
    with tempfile.TemporaryDirectory() as tmp:
        n = int(args.cli_mb * 1e6)
        g, rec_start = genome(n, 4, 3)
        fa, census, sam = (os.path.join(tmp, x) for x in ("g.fa", "census.csv", "placed.sam"))
        with open(fa, "wb") as fh:
            for c in range(4):
                fh.write(b">chr%d\n" % c)
                s = g[rec_start[c]:rec_start[c + 1]]
                s = s[:len(s) - len(s) % 60].reshape(-1, 60)
                fh.write(np.hstack([s, np.full((s.shape[0], 1), 10, np.uint8)]).tobytes())
        text = g.tobytes().decode()
        with open(census, "w") as fh:
            fh.write("Tag sequence,Count\n")
            k = text.find("TGCAG")
            seen = set()
            while k != -1 and len(seen) < 20000:
                w = text[k:k + 64]
                if len(w) == 64 and w not in seen:
                    seen.add(w)
                    fh.write("%s,%d\n" % (w, 5))
                k = text.find("TGCAG", k + 1)
        for backend in ("gpu", "host"):
            t0 = time.perf_counter()
            subprocess.run([sys.executable, "-m", "tagdigger_amd.tag_place", "-i", census, "-g", fa, "-e", "PstI", "-o", sam,
                            "--td-backend", backend], check=True, cwd=ROOT, stdout=subprocess.DEVNULL)
            say("command line, %.0f MB genome, %d tags, --td-backend %s: %.2f s wall" % (args.cli_mb, len(seen), backend, time.perf_counter() - t0))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
