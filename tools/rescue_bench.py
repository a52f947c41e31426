#!/usr/bin/env python3
"""Tag rescue against the count pass and the census pass over the same bytes, in one process per part.

  clean   the canonical synthetic library (SynthConfig: 384 barcodes x 100 k tags) resident in HBM, no substitutions
  noisy   the same reads with every base from the read's ninth on -- behind the longest barcode -- substituted with
          probability 1 % by numpy's seeded generator (the bytes come to the host for it and go back)
          both: HIP-event time of td_rescue_device at K = 1 and K = 2, of td_count_device and of td_census_device over the
          same buffer (best and median of --rounds after one warm-up), the seven classes, directory probes and verified
          tags per read with barcode + cut site, the longest run
  sweep   16 384 tags of 40 bases in runs of r = 16 .. 16 384 that share their first part; reads one substitution from a
          tag, in the second part, so that every read walks one whole run: time per pass at K = 1

Without --part the tool starts itself once per part, each under --limit seconds, and stops at the first part that
fails.  Everything printed is appended to --out (default profiles/rescue/bench_mi355x.txt, the recorded run).

    python tools/rescue_bench.py [--reads 4000000] [--rounds 5] [--parts clean,noisy,sweep] [--out FILE]
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
ap.add_argument("--sweep-reads", type=int, default=262_144)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--parts", default="clean,noisy,sweep")
ap.add_argument("--part", help="run this one part in this process")
ap.add_argument("--limit", type=int, default=420, help="seconds a part may take")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescue", "bench_mi355x.txt"))
args = ap.parse_args()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

if args.part is None:
    with open(args.out, "w") as fh:
        fh.write("python tools/rescue_bench.py " + " ".join(sys.argv[1:]) + "\n")
    for part in args.parts.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--reads", str(args.reads), "--sweep-reads", str(args.sweep_reads),
               "--rounds", str(args.rounds), "--out", args.out]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            with open(args.out, "a") as fh:
                fh.write("part %s ended with status %d: nothing further was run\n" % (part, rc))
            sys.exit(rc)
    sys.exit(0)

out_fh = open(args.out, "a")


def print(*a):           # noqa: A001 -- every line goes to the recorded file as well
    line = " ".join(str(x) for x in a)
    sys.stdout.write(line + "\n")
    sys.stdout.flush()
    out_fh.write(line + "\n")
    out_fh.flush()


import torch  # noqa: E402  (events on the default stream, which every pass is launched on)
import tagdigger_amd  # noqa: E402
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


if args.part in ("clean", "noisy"):
    cfg = SynthConfig(nreads=args.reads, nbar=384, nmarkers=50_000, seed=3)
    nb = cfg.nbytes()
    d = eng.dev_alloc(nb)
    cfg.fill_device(eng, d, 0, cfg.nreads)
    eng.sync()
    if args.part == "noisy":
        rec = np.frombuffer(eng.d2h(d, nb), dtype=np.uint8).reshape(cfg.nreads, cfg.record_bytes).copy()
        seq0 = int(np.flatnonzero(rec[0] == 10)[0]) + 1            # the sequence line follows the header's terminator
        rng = np.random.default_rng(11)
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)
        code = np.zeros(256, dtype=np.uint8)
        code[letters] = np.arange(4, dtype=np.uint8)
        nsub = 0
        for lo in range(0, cfg.nreads, 250_000):
            block = rec[lo:lo + 250_000, seq0 + 8:seq0 + cfg.read_len]
            hit = rng.random(block.shape, dtype=np.float32) < 0.01
            shift = rng.integers(1, 4, int(hit.sum()), dtype=np.uint8)
            block[hit] = letters[(code[block[hit]] + shift) & 3]
            nsub += int(hit.sum())
        eng.h2d(d, rec.tobytes())
        del rec
        print("noisy: %d substitutions in %d bases (positions 8 .. %d of every read)" % (nsub, cfg.nreads * (cfg.read_len - 8), cfg.read_len - 1))
    print("%s: %d reads, %.3f GB of FASTQ, %d barcodes x %d tags" % (args.part, cfg.nreads, nb / 1e9, len(cfg.barcodes), len(cfg.tags)))
    eng.set_index(cfg.barcodes, cfg.tags, cfg.cutsite)
    line("count", rounds(eng.reset, lambda: eng.count_device(d, nb)), nb)
    cst = eng.stats()
    line("census (64)", rounds(lambda: eng.census_begin(cfg.barcodes, cfg.cutsite, 64, 1 << 24), lambda: eng.census_device(d, nb)), nb)
    eng.census_end()
    for K in (1, 2):
        line("rescue K=%d" % K, rounds(lambda: eng.rescue_begin(cfg.barcodes, cfg.tags, cfg.cutsite, K), lambda: eng.rescue_device(d, nb)), nb)
        st, wk = eng.rescue_stats(), eng.rescue_work()
        assert st["barcut"] == cst["barcut"] and st["exact"] == cst["tag"], (st, cst)
        assert st["barcut"] == st["exact"] + st["rescued1"] + st["rescued2"] + st["ambiguous"] + st["none"]
        print("    reads %(reads)d barcut %(barcut)d exact %(exact)d rescued1 %(rescued1)d rescued2 %(rescued2)d ambiguous %(ambiguous)d "
              "none %(none)d  longest run %(longest_run)d" % st)
        print("    per read with barcode + cut site: %.3f directory probes, %.3f verified tags; parts of %d bases; exact == the counter's tag count" % (
            wk["probes"] / max(1, st["barcut"]), wk["verified"] / max(1, st["barcut"]), wk["part_bases"]))
        eng.rescue_end()
    eng.dev_free(d)

if args.part == "sweep":
    rng = np.random.default_rng(12)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    total, n = 16384, args.sweep_reads
    eng.set_option("rescue_max_run", 1 << 20)
    print("sweep: %d tags of 40 bases, %d reads, each one substitution (in the second part) from a tag: a read walks one run" % (total, n))
    for r in (16, 64, 256, 1024, 4096, 16384):
        heads = letters[rng.integers(0, 4, (total // r, 20))]
        tails = letters[rng.integers(0, 4, (total, 20))]
        tags = np.concatenate([np.repeat(heads, r, axis=0), tails], axis=1)
        tags = np.unique(tags, axis=0)
        pick = tags[rng.integers(0, len(tags), n)].copy()
        pos = rng.integers(20, 40, n)
        pick[np.arange(n), pos] = letters[(np.searchsorted(letters, pick[np.arange(n), pos]) + rng.integers(1, 4, n)) & 3]
        rec = np.empty((n, 12 + 40 + 5), dtype=np.uint8)
        rec[:, :12] = np.frombuffer(b"@r\nACGTTGCAG", dtype=np.uint8)
        rec[:, 12:52] = pick
        rec[:, 52:] = np.frombuffer(b"\n+\nI\n", dtype=np.uint8)
        data = rec.tobytes()
        taglist = ["TGCAG" + t.tobytes().decode() for t in tags]
        d = eng.dev_alloc(len(data))
        eng.h2d(d, data)
        ts = rounds(lambda: eng.rescue_begin(["ACGT"], taglist, "TGCAG", 1), lambda: eng.rescue_device(d, len(data)))
        st, wk = eng.rescue_stats(), eng.rescue_work()
        print("  run %5d: best %.3f ms  median %.3f ms  = %.1f ns per read  (longest run %d, %.1f verified tags per read, rescued1 %d, ambiguous %d)" % (
            r, min(ts), statistics.median(ts), statistics.median(ts) * 1e6 / n, st["longest_run"], wk["verified"] / n, st["rescued1"], st["ambiguous"]))
        eng.rescue_end()
        eng.dev_free(d)
    eng.set_option("rescue_max_run", 0)
eng.close()
