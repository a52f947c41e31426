#!/usr/bin/env python3
"""Library QC against the count pass and the census pass over the same bytes, in one process and alternating.

  device   the canonical synthetic library (td_synth_fill_device, the bench's 384-barcode shape) resident in HBM:
           HIP-event time of td_qc_device, td_count_device and td_census_device over the same buffer after a warm-up
           round, median and spread, GB/s of FASTQ read, and the ratios; then the same with the quality bytes drawn
           from a skewed 40-symbol distribution instead of the generator's single symbol
  e2e      library_qc on a plain file and on the same as gzip, against backend="host"
  grid     (not in the default parts) the QC pass over 40 M reads with the grid capped at 2, 1.5, 1 and 0.5 workgroups
           per CU (option max_grid): does the time follow the resident waves?

Everything printed is also written to --out (default profiles/qc/bench_mi355x.txt, the recorded run).

    python tools/qc_bench.py [--reads 200000000] [--rounds 5] [--e2e-reads 2000000] [--parts device,e2e] [--out FILE]
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
ap.add_argument("--max-cycles", type=int, default=160)
ap.add_argument("--census-slots", type=int, default=1 << 24)
ap.add_argument("--e2e-reads", type=int, default=2_000_000)
ap.add_argument("--parts", default="device,e2e")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qc", "bench_mi355x.txt"))
ap.add_argument("--dir", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "qc_bench"))
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


print("python tools/qc_bench.py " + " ".join(sys.argv[1:]))

import torch  # noqa: E402  (events on the default stream, which the passes are launched on; the buffer is a torch tensor)

eng = tagdigger_amd.Engine(0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ts):
    return "median %.2f ms, min %.2f, max %.2f (%s)" % (statistics.median(ts), min(ts), max(ts), " ".join("%.2f" % t for t in ts))


def device_rounds(cfg, d, nb, label):
    """Warm-up round, then `rounds` rounds of the three passes alternating over the same resident buffer."""
    t = {"qc": [], "count": [], "census": []}
    while True:                                      # a census table that holds the library (four times the slots while it fills up)
        eng.census_begin(cfg.barcodes, cfg.cutsite, 64, args.census_slots)
        eng.census_device(d, nb)
        try:
            eng.census_stats()
            break
        except TagdigError as exc:
            if exc.code != -7:
                raise
            args.census_slots *= 4
    for r in range(args.rounds + 1):
        eng.qc_begin(cfg.barcodes, cfg.cutsite, args.max_cycles)
        a = timed(lambda: eng.qc_device(d, nb))
        eng.reset()
        b = timed(lambda: eng.count_device(d, nb))
        eng.census_begin(cfg.barcodes, cfg.cutsite, 64, args.census_slots)
        c = timed(lambda: eng.census_device(d, nb))
        if r:                                        # (round 0 warms up: first launches, cold caches)
            t["qc"].append(a); t["count"].append(b); t["census"].append(c)
    st, cst = eng.qc_stats(), eng.stats()
    assert st["reads"] == cst["reads"] == cfg.nreads and st["barcut"] == cst["barcut"] and st["qual_lines"] == cfg.nreads, (st, cst)
    tables = eng.qc_fetch()
    med = {k: statistics.median(v) for k, v in t.items()}
    print("device, %s: %d reads, %.2f GB of FASTQ, max_cycles %d, %d rounds after one warm-up" % (label, cfg.nreads, nb / 1e9, args.max_cycles, args.rounds))
    for k in ("qc", "count", "census"):
        print("  %-6s pass  %s  %.0f GB/s" % (k, spread(t[k]), nb / med[k] / 1e6))
    print("  qc / count = %.2f   qc / census = %.2f" % (med["qc"] / med["count"], med["qc"] / med["census"]))
    print("  reads %(reads)d barcut %(barcut)d bases %(bases)d qual_bases %(qual_bases)d qual_invalid %(qual_invalid)d" % st)
    print("  distinct quality symbols: %d" % int((tables[2].sum(axis=0)[:94] > 0).sum()))
    eng.qc_end()
    eng.census_end()


if "device" in parts:
    cfg = SynthConfig(nreads=args.reads, nbar=384, nmarkers=50_000, seed=3)
    nb = cfg.nbytes()
    buf = torch.empty(nb, dtype=torch.uint8, device="cuda")
    d = buf.data_ptr()
    cfg.fill_device(eng, d, 0, cfg.nreads)
    eng.set_index(cfg.barcodes, cfg.tags, cfg.cutsite)
    eng.sync()
    device_rounds(cfg, d, nb, "quality all one symbol")
    # the quality line of every record (records are of one size) redrawn: 40 symbols, Phred 2 .. 41, the high ones common
    rec = bytes(eng.d2h(d, cfg.record_bytes))
    q0 = rec.rstrip(b"\n").rfind(b"\n") + 1
    qlen = len(rec.rstrip(b"\n")) - q0
    assert qlen == cfg.read_len and rec[q0 - 3:q0] == b"\n+\n", rec
    w = np.arange(1, 41, dtype=np.float64) ** 3
    lut = np.repeat(np.arange(40), np.maximum(1, np.round(w / w.sum() * 4096)).astype(np.int64))[:4096]
    lut = np.concatenate([lut, np.full(4096 - len(lut), 39)]).astype(np.uint8) + 35
    d_lut = torch.from_numpy(lut).cuda()
    view = buf.view(cfg.nreads, cfg.record_bytes)
    gen = torch.Generator(device="cuda").manual_seed(5)
    step = 2_000_000
    for lo in range(0, cfg.nreads, step):
        hi = min(cfg.nreads, lo + step)
        idx = torch.randint(0, 4096, (hi - lo, qlen), device="cuda", generator=gen)
        view[lo:hi, q0:q0 + qlen] = d_lut[idx]
    del idx
    torch.cuda.synchronize()
    device_rounds(cfg, d, nb, "quality from 40 symbols")
    del view, buf

if "grid" in parts:
    cfg = SynthConfig(nreads=40_000_000, nbar=384, nmarkers=50_000, seed=3)
    nb = cfg.nbytes()
    buf = torch.empty(nb, dtype=torch.uint8, device="cuda")
    d = buf.data_ptr()
    cfg.fill_device(eng, d, 0, cfg.nreads)
    eng.sync()
    print("grid: %d reads, %.2f GB of FASTQ, three rounds after one warm-up" % (cfg.nreads, nb / 1e9))
    for grid in (0, 512, 384, 256, 128, 0):
        eng.set_option("max_grid", grid)
        ts = []
        for r in range(4):
            eng.qc_begin(cfg.barcodes, cfg.cutsite, args.max_cycles)
            t = timed(lambda: eng.qc_device(d, nb))
            if r:
                ts.append(t)
        print("  max_grid %4d: median %.2f ms (%s)" % (grid, statistics.median(ts), " ".join("%.2f" % t for t in ts)))
    eng.set_option("max_grid", 0)
    eng.qc_end()
    del buf

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
        out = tf.library_qc(path, cfg.barcodes, cfg.cutsite, args.max_cycles, backend=backend)
        res[name] = (time.perf_counter() - t0, out)
        print("e2e %-10s %d reads: %.3f s, barcut %d, bases %d" % (name, cfg.nreads, res[name][0], out.stats["barcut"], out.stats["bases"]))
    for name in ("gpu gzip", "host plain"):
        a, b = res["gpu plain"][1], res[name][1]
        assert a.stats == b.stats and all((getattr(a, t) == getattr(b, t)).all() for t in ("barcodes", "base_cycle", "qual_cycle", "lengths", "meanq"))
    print("e2e host / gpu plain = %.1f" % (res["host plain"][0] / res["gpu plain"][0]))
    os.remove(plain)
    os.remove(gz)
eng.close()
