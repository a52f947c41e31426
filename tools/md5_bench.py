#!/usr/bin/env python3
"""MD5 sums of the files a split leaves behind: three routes over the same files.

Input: td_split_file on the canonical synthetic stream (seeded, 384 barcodes) -> 384 FASTQ files, and lists of the
first 1, 8, 64 and 96 of them.  Routes, alternating, ROUNDS rounds each, every file warm in the page cache (they have
just been written, and an untimed pass reads them all once more):
  (a) reference  one thread, hashlib.md5, 50 MiB reads -- the loop of the reference's writeMD5sums
  (b) host       writeMD5sums(backend="host"): hashlib on a pool of 16 threads
  (c) gpu        writeMD5sums(backend="gpu") with the device threshold at 1: td_md5_files, one file per lane
Wall time is taken around the whole call (the device route ends in a synchronise: it returns digests).  For (c) the
library's own split of the time (reading into the slots, waiting for the GPU, kernel time from events) is printed too,
and the kernel's cycles per 64-byte block per wave derived from it at the clock given by --mhz.

    python tools/md5_bench.py [--reads 40000000] [--rounds 3] [--dir DIR] [--keep] [--reuse] [--routes abc]
"""
import argparse
import contextlib
import hashlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tagdigger_amd  # noqa: E402
from tagdigger_amd import tagdigger_fun as tf  # noqa: E402
from tagdigger_amd.synth import SynthConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=40_000_000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--dir", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "md5_bench"))
ap.add_argument("--keep", action="store_true", help="leave the split files in --dir")
ap.add_argument("--reuse", action="store_true", help="use the split files a --keep run left")
ap.add_argument("--routes", default="abc")
ap.add_argument("--mhz", type=float, default=2400.0, help="shader clock assumed for cycles per block")
args = ap.parse_args()

eng = tagdigger_amd.Engine(0)
tf.default_engine(0)            # (writeMD5sums' engine: made before anything is timed)
os.makedirs(args.dir, exist_ok=True)
nbar = 384
outs = [os.path.join(args.dir, "split_%03d.fq" % i) for i in range(nbar)]
if not args.reuse:
    cfg = SynthConfig(nreads=args.reads, nbar=nbar, nmarkers=50_000, seed=3, adapter_pct=20)
    src = os.path.join(args.dir, "in.fq")
    step = 4_000_000
    d = eng.dev_alloc(step * cfg.record_bytes)
    with open(src, "wb") as fh:
        for lo in range(0, args.reads, step):
            n = min(step, args.reads - lo)
            cfg.fill_device(eng, d, lo, n)
            fh.write(eng.d2h(d, n * cfg.record_bytes))
    eng.dev_free(d)
    with contextlib.redirect_stdout(io.StringIO()):
        ends = tf._adapter_ends(tf.adapters["PstI-MspI-Hall"], cfg.barcodes)
    eng.set_splitter(cfg.barcodes, cfg.cutsite, "CCGG", "CTGCAG", ends)
    t0 = time.perf_counter()
    st = eng.split_file(src, outs)
    print("split: %d reads -> %d files in %.1f s (reads %d, barcode+site %d, clipped %d)" % (args.reads, nbar, time.perf_counter() - t0, *st))
    os.remove(src)
sizes = [os.path.getsize(o) for o in outs]
print("files: %d, %.3f GB in all, smallest %.1f MB, largest %.1f MB" % (nbar, sum(sizes) / 1e9, min(sizes) / 1e6, max(sizes) / 1e6))


def route_a(files, out):
    with open(out, "w") as fh:
        for f in files:
            m = hashlib.md5()
            with open(f, "rb") as con:
                while True:
                    chunk = con.read(50 * 1048576)
                    if chunk == b"":
                        break
                    m.update(chunk)
            fh.write("%s,%s\n" % (f, m.hexdigest()))


def route_b(files, out):
    with contextlib.redirect_stdout(io.StringIO()):
        tf.writeMD5sums(files, out, backend="host")


def route_c(files, out):
    with contextlib.redirect_stdout(io.StringIO()):
        tf.writeMD5sums(files, out, backend="gpu")


tf._MD5_DEVICE_MIN_FILES = 1                    # (route (c) on the device at every list length)
ROUTES = {"a": ("reference loop, 1 thread", route_a), "b": ("host pool, 16 threads", route_b), "c": ("gpu, file per lane", route_c)}
for f in outs:                                   # untimed pass: every file through the page cache once more
    with open(f, "rb") as con:
        while con.read(1 << 24):
            pass
sums = {}
print("%-6s %-26s %10s %10s %10s   %s" % ("files", "route", "GB", "median s", "GB/s", "rounds (s)"))
for n in (384, 96, 64, 8, 1):
    files = outs[:n]
    nbytes = sum(sizes[:n])
    times = {r: [] for r in args.routes}
    for k in range(args.rounds):
        for r in args.routes:
            out = os.path.join(args.dir, "sums_%s.csv" % r)
            t0 = time.perf_counter()
            ROUTES[r][1](files, out)
            times[r].append(time.perf_counter() - t0)
            got = [line.strip().split(",")[-1] for line in open(out).read().splitlines() if not line.startswith("File name")]
            assert sums.setdefault(n, got) == got, "routes disagree"
    for r in args.routes:
        med = statistics.median(times[r])
        print("%-6d %-26s %10.3f %10.3f %10.2f   %s  spread %.0f%%" % (
            n, ROUTES[r][0], nbytes / 1e9, med, nbytes / med / 1e9, " ".join("%.3f" % t for t in times[r]),
            100 * (max(times[r]) - min(times[r])) / med))
    if "c" in args.routes:                       # where the device route's time goes: the library's own figures
        t0 = time.perf_counter()
        _, ms = tf.default_engine(0).md5_files(files)
        wall = time.perf_counter() - t0
        blocks = max(sizes[:n]) // 64 + 1        # the longest lane's chain: every wave of a launch waits for it
        print("%-6d   td_md5_files alone: wall %.3f s = reading %.3f + waiting for the GPU %.3f + rest %.3f; kernel %.3f s "
              "(%.1f GB/s), %.0f cycles per block per wave at %.0f MHz" % (
                  n, wall, ms[0] / 1e3, ms[1] / 1e3, wall - (ms[0] + ms[1]) / 1e3, ms[2] / 1e3, nbytes / ms[2] / 1e6,
                  ms[2] * 1e-3 * args.mhz * 1e6 / blocks, args.mhz))
if not args.keep:
    for f in outs + [os.path.join(args.dir, "sums_%s.csv" % r) for r in "abc"]:
        if os.path.exists(f):
            os.remove(f)
eng.close()
