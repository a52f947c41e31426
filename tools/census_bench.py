#!/usr/bin/env python3
"""Tag census against the count pass over the same bytes, in one process and alternating.

  device   the canonical synthetic library (td_synth_fill_device, the bench's 384-barcode shape) resident in HBM:
           HIP-event time of td_census_device and of td_count_device over the same buffer, `distinct`, slots, load,
           GB/s of FASTQ read, and the ratio of the two passes
  combine  wave-level combining on and off (TAGDIG_CENSUS_COMBINE, read at td_census_begin) on a library of 3 distinct
           windows and on one whose windows are all distinct
  e2e      tag_census on a plain file and on the same as gzip, against backend="host"

Everything printed is also written to --out (default profiles/census/bench_mi355x.txt, the recorded run).

    python tools/census_bench.py [--reads 200000000] [--rounds 5] [--e2e-reads 2000000] [--parts device,combine,e2e] [--out FILE]
"""
import argparse
import gzip
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tagdigger_amd  # noqa: E402
from tagdigger_amd import TagdigError, tagdigger_fun as tf  # noqa: E402
from tagdigger_amd.synth import SynthConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=200_000_000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--taglen", type=int, default=64)
ap.add_argument("--slots", type=int, default=1 << 24)
ap.add_argument("--e2e-reads", type=int, default=2_000_000)
ap.add_argument("--ab-reads", type=int, default=4_000_000)
ap.add_argument("--parts", default="device,combine,e2e")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census", "bench_mi355x.txt"))
ap.add_argument("--dir", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "census_bench"))
args = ap.parse_args()
parts = set(args.parts.split(","))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
out_fh = open(args.out, "w")


def print(*a):           # noqa: A001 -- every line goes to the recorded file as well
    line = " ".join(str(x) for x in a)
    sys.stdout.write(line + "\n")
    sys.stdout.flush()
    out_fh.write(line + "\n")
    out_fh.flush()


print("python tools/census_bench.py " + " ".join(sys.argv[1:]))

import torch  # noqa: E402  (events on the default stream, which both passes are launched on)

eng = tagdigger_amd.Engine(0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def begin_fitting(barcodes, cutsite, taglen, slots, run):
    """td_census_begin + run(), with four times the slots while the table fills up; -> the slots that held it."""
    while True:
        eng.census_begin(barcodes, cutsite, taglen, slots)
        try:
            run()
            eng.census_stats()
            return slots
        except TagdigError as exc:
            if exc.code != -7:
                raise
            slots *= 4


if "device" in parts:
    cfg = SynthConfig(nreads=args.reads, nbar=384, nmarkers=50_000, seed=3)
    nb = cfg.nbytes()
    d = eng.dev_alloc(nb)
    cfg.fill_device(eng, d, 0, cfg.nreads)
    eng.set_index(cfg.barcodes, cfg.tags, cfg.cutsite)
    eng.sync()
    slots = begin_fitting(cfg.barcodes, cfg.cutsite, args.taglen, args.slots, lambda: (eng.census_device(d, nb), eng.sync()))
    t_census, t_count = [], []
    for r in range(args.rounds):
        eng.census_begin(cfg.barcodes, cfg.cutsite, args.taglen, slots)
        t_census.append(timed(lambda: eng.census_device(d, nb)))
        eng.reset()
        t_count.append(timed(lambda: eng.count_device(d, nb)))
    st, cst = eng.census_stats(), eng.stats()
    assert st["barcut"] == cst["barcut"], (st, cst)
    mc, mk = statistics.median(t_census), statistics.median(t_count)
    print("device: %d reads, %.2f GB of FASTQ, taglen %d" % (cfg.nreads, nb / 1e9, args.taglen))
    print("  census pass  median %.2f ms (%s)  %.0f GB/s" % (mc, " ".join("%.2f" % t for t in t_census), nb / mc / 1e6))
    print("  count pass   median %.2f ms (%s)  %.0f GB/s" % (mk, " ".join("%.2f" % t for t in t_count), nb / mk / 1e6))
    print("  census / count = %.2f" % (mc / mk))
    print("  reads %(reads)d barcut %(barcut)d short %(short)d ambiguous %(ambiguous)d counted %(counted)d distinct %(distinct)d" % st)
    print("  slots %d (%.1f MiB), load %.3f" % (slots, slots * (32 if args.taglen > 32 else 16) / 2 ** 20, st["distinct"] / slots))
    eng.census_end()
    eng.dev_free(d)

if "combine" in parts:
    rng = np.random.default_rng(1)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    n = args.ab_reads
    head = np.frombuffer(b"@r\nACGTTGCAG", dtype=np.uint8)
    tailq = np.frombuffer(b"\n+\nI\n", dtype=np.uint8)
    rec = np.empty((n, len(head) + 64 + len(tailq)), dtype=np.uint8)
    rec[:, :len(head)] = head
    rec[:, len(head) + 64:] = tailq
    bodies = letters[rng.integers(0, 4, (n, 64))]
    hot = bodies[:3]
    for name, body in (("3 distinct windows", hot[rng.choice(3, n, p=[0.8, 0.15, 0.05])]), ("all windows distinct", bodies)):
        rec[:, len(head):len(head) + 64] = body
        data = rec.tobytes()
        d = eng.dev_alloc(len(data))
        eng.h2d(d, data)
        for combine in ("1", "0"):
            os.environ["TAGDIG_CENSUS_COMBINE"] = combine
            slots = begin_fitting(["ACGT"], "TGCAG", 64, 1 << 20, lambda: (eng.census_device(d, len(data)), eng.sync()))
            ts = []
            for r in range(args.rounds):
                eng.census_begin(["ACGT"], "TGCAG", 64, slots)
                ts.append(timed(lambda: eng.census_device(d, len(data))))
            st = eng.census_stats()
            print("combine=%s  %-22s %d reads: median %.3f ms (%s), distinct %d, slots %d" % (
                combine, name, n, statistics.median(ts), " ".join("%.3f" % t for t in ts), st["distinct"], slots))
        eng.census_end()
        eng.dev_free(d)
    os.environ.pop("TAGDIG_CENSUS_COMBINE", None)

if "e2e" in parts:
    os.makedirs(args.dir, exist_ok=True)
    cfg = SynthConfig(nreads=args.e2e_reads, nbar=384, nmarkers=50_000, seed=3)
    d = eng.dev_alloc(cfg.nbytes())
    cfg.fill_device(eng, d, 0, cfg.nreads)
    data = eng.d2h(d, cfg.nbytes())
    eng.dev_free(d)
    plain, gz = os.path.join(args.dir, "lib.fq"), os.path.join(args.dir, "lib.fq.gz")
    with open(plain, "wb") as fh:
        fh.write(data)
    with gzip.open(gz, "wb", compresslevel=1) as fh:
        fh.write(data)
    tf.default_engine(0)
    res = {}
    for name, path, backend in (("gpu plain", plain, "gpu"), ("gpu gzip", gz, "gpu"), ("gpu plain", plain, "gpu"), ("gpu gzip", gz, "gpu"),
                                ("host plain", plain, "host")):
        t0 = time.perf_counter()
        out = tf.tag_census(path, cfg.barcodes, cfg.cutsite, backend=backend)
        res[name] = (time.perf_counter() - t0, out)
        print("e2e %-10s %d reads: %.3f s, distinct %d" % (name, cfg.nreads, res[name][0], out.stats["distinct"]))
    assert list(res["gpu plain"][1]) == list(res["host plain"][1]) == list(res["gpu gzip"][1])
    print("e2e host / gpu plain = %.1f" % (res["host plain"][0] / res["gpu plain"][0]))
    os.remove(plain)
    os.remove(gz)
eng.close()
