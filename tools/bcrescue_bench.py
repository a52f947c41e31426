#!/usr/bin/env python3
"""Barcode rescue against the census pass and the tag-rescue pass over the same bytes, in one process.

The canonical synthetic library of tools/rescue_bench.py (SynthConfig: 384 barcodes x 100 k tags) resident in HBM,
every base of every read -- barcode and cut site included -- substituted with probability 1 % by numpy's seeded
generator (the bytes come to the host for it and go back).  HIP-event time of td_bcrescue_device at K = 1 and K = 2, of
td_census_device and of td_rescue_device (K = 1) over the same buffer (best and median of --rounds after one warm-up),
the classes, the entries compared per read without an exact entry, and min_entry_distance of the generator's barcodes.

The tool starts itself once under --limit seconds.  Everything printed is written to --out (default
profiles/bcrescue/bench_mi355x.txt, the recorded run).

    python tools/bcrescue_bench.py [--reads 4000000] [--rounds 5] [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=4_000_000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--child", action="store_true", help="measure in this process")
ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcrescue", "bench_mi355x.txt"))
args = ap.parse_args()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

if not args.child:
    with open(args.out, "w") as fh:
        fh.write("python tools/bcrescue_bench.py " + " ".join(sys.argv[1:]) + "\n")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reads", str(args.reads), "--rounds", str(args.rounds), "--out", args.out]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        rc = 124
    if rc != 0:
        with open(args.out, "a") as fh:
            fh.write("the measurement ended with status %d\n" % rc)
    sys.exit(rc)

out_fh = open(args.out, "a")


def print(*a):           # noqa: A001 -- every line goes to the recorded file as well
    line = " ".join(str(x) for x in a)
    sys.stdout.write(line + "\n")
    sys.stdout.flush()
    out_fh.write(line + "\n")
    out_fh.flush()


import torch  # noqa: E402  (events on the default stream, which every pass is launched on)
import tagdigger_amd  # noqa: E402
from tagdigger_amd import tagdigger_fun as tf  # noqa: E402
from tagdigger_amd.engine import rescue_index  # noqa: E402
from tagdigger_amd.synth import SynthConfig  # noqa: E402

eng = tagdigger_amd.Engine(0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rounds(prepare, fn):
    prepare()
    timed(fn)                                  # warm-up
    ts = []
    for _ in range(args.rounds):
        prepare()
        ts.append(timed(fn))
    return ts


def line(name, ts, nbytes):
    print("  %-16s best %.2f ms  median %.2f ms  (%s)  %.0f GB/s at the median" % (
        name, min(ts), statistics.median(ts), " ".join("%.2f" % t for t in ts), nbytes / statistics.median(ts) / 1e6))


cfg = SynthConfig(nreads=args.reads, nbar=384, nmarkers=50_000, seed=3)
nb = cfg.nbytes()
d = eng.dev_alloc(nb)
cfg.fill_device(eng, d, 0, cfg.nreads)
eng.sync()
rec = np.frombuffer(eng.d2h(d, nb), dtype=np.uint8).reshape(cfg.nreads, cfg.record_bytes).copy()
seq0 = int(np.flatnonzero(rec[0] == 10)[0]) + 1            # the sequence line follows the header's terminator
rng = np.random.default_rng(11)
letters = np.frombuffer(b"ACGT", dtype=np.uint8)
code = np.zeros(256, dtype=np.uint8)
code[letters] = np.arange(4, dtype=np.uint8)
nsub = 0
for lo in range(0, cfg.nreads, 250_000):
    block = rec[lo:lo + 250_000, seq0:seq0 + cfg.read_len]
    hit = rng.random(block.shape, dtype=np.float32) < 0.01
    shift = rng.integers(1, 4, int(hit.sum()), dtype=np.uint8)
    block[hit] = letters[(code[block[hit]] + shift) & 3]
    nsub += int(hit.sum())
eng.h2d(d, rec.tobytes())
del rec
print("%d reads, %.3f GB of FASTQ, %d barcodes x %d tags; %d substitutions, 1 %% per base over the whole read" % (
    cfg.nreads, nb / 1e9, len(cfg.barcodes), len(cfg.tags), nsub))
barcut, barnum, _, _ = rescue_index(cfg.barcodes, cfg.tags, cfg.cutsite)
entries = tf._bcrescue_entries(barcut, barnum)
print("%d entries of %d .. %d bases; min_entry_distance of the generator's barcode set: %d" % (
    len(entries), min(len(s) for s, _ in entries), max(len(s) for s, _ in entries), tf._bcrescue_min_distance(entries)))
line("census (64)", rounds(lambda: eng.census_begin(cfg.barcodes, cfg.cutsite, 64, 1 << 24), lambda: eng.census_device(d, nb)), nb)
cst = eng.census_stats()
eng.census_end()
line("tag rescue K=1", rounds(lambda: eng.rescue_begin(cfg.barcodes, cfg.tags, cfg.cutsite, 1), lambda: eng.rescue_device(d, nb)), nb)
eng.rescue_end()
for K in (1, 2):
    line("bcrescue K=%d" % K, rounds(lambda: eng.bcrescue_begin(cfg.barcodes, cfg.tags, cfg.cutsite, K), lambda: eng.bcrescue_device(d, nb)), nb)
    st = eng.bcrescue_stats()
    assert st["exact"] == cst["barcut"], (st, cst)
    assert st["reads"] == st["exact"] + st["rescued1"] + st["rescued2"] + st["ambiguous"] + st["none"]
    assert st["min_entry_distance"] == tf._bcrescue_min_distance(entries)
    print("    reads %(reads)d exact %(exact)d rescued1 %(rescued1)d rescued2 %(rescued2)d ambiguous %(ambiguous)d none %(none)d tagged %(tagged)d" % st)
    print("    reads without an exact entry: %d (%.2f %% of the reads), %d entries compared with each; exact == the census's reads with barcode + cut site" % (
        st["reads"] - st["exact"], 100.0 * (st["reads"] - st["exact"]) / max(1, st["reads"]), len(entries)))
    eng.bcrescue_end()
eng.dev_free(d)
eng.close()
