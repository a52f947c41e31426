#!/usr/bin/env python3
"""Measures the tag network (tag_network, csrc/tagnet.hip) on one GPU and writes profiles/tagpairs/bench_mi355x.txt.

    python tools/tagpairs_bench.py [--tags 1000000] [--run 20000] [--big-run 200000] [--out FILE]

(a) a synthetic census of --tags tags of 64 bases (the recipe of tests/tagnet_cases.py library(), vectorised): the
    device path against backend="host" on the same input; the results are compared before any time is printed
(b) one run of --run tags that share part A, and one of --big-run tags: K4's compare rate and the cap it implies
(c) the tags of (a) cut to 32 bases (duplicates dropped)
Device time per kernel is what td_tagnet_build measures with HIP events; wall time is the clock around the call."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tagdigger_amd import tagdigger_fun as tf          # noqa: E402
from tagdigger_amd.engine import default_engine        # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def census_order(codes, counts):
    """(list of str, list of int): distinct rows (the first of equal ones), count descending, then sequence."""
    text = np.ascontiguousarray(ACGT[codes]).view("S%d" % codes.shape[1]).ravel()
    _, first = np.unique(text, return_index=True)
    first.sort()
    text, counts = text[first], counts[first]
    order = np.lexsort((text, -counts))
    return [s.decode("ascii") for s in text[order]], [int(c) for c in counts[order]]


def mutated(rng, codes, pos=None):
    out = codes.copy()
    rows = np.arange(len(codes))
    pos = rng.integers(0, codes.shape[1], len(codes)) if pos is None else pos
    out[rows, pos] = (out[rows, pos] + rng.integers(1, 4, len(codes))) & 3
    return out, pos


def synthetic_census(rng, ntags, L):
    """About ntags tags: loci with counts 50-400, a second allele for every other one (20-400), a third at the same
    position for one in ten, and three error tags per locus at distance 1 from a tag drawn so far (counts 1-3)."""
    nloci = max(1, int(ntags / 4.6))
    loci = rng.integers(0, 4, (nloci, L), dtype=np.uint8)
    second, pos = mutated(rng, loci[::2])
    third, _ = mutated(rng, loci[::10], pos[::5])
    real = np.concatenate([loci, second, third])
    real_counts = np.concatenate([rng.integers(50, 401, nloci), rng.integers(20, 401, len(second)),
                                  rng.integers(20, 401, len(third))])
    errors, _ = mutated(rng, real[rng.integers(0, len(real), 3 * nloci)])
    codes = np.concatenate([real, errors])
    counts = np.concatenate([real_counts, rng.integers(1, 4, len(errors))])
    return census_order(codes, counts)


def one_run(rng, m, L=64):
    """m distinct tags that share part A (the first half), one in six of them a neighbour of another."""
    h = (L + 1) // 2
    tail = rng.integers(0, 4, (m - m // 6, L - h), dtype=np.uint8)
    near, _ = mutated(rng, tail[rng.integers(0, len(tail), m // 6)])
    codes = np.concatenate([tail, near])
    codes = np.concatenate([np.broadcast_to(rng.integers(0, 4, h, dtype=np.uint8), (len(codes), h)), codes], axis=1)
    return census_order(codes, rng.integers(1, 401, len(codes)))


def device_network(eng, seqs, counts, ppm=30000):
    """(pairs, kept edges, degrees, TagNet statistics, ms per kernel, wall seconds of build + fetch) through the engine."""
    data = "".join(seqs).encode("ascii")
    cnt = np.asarray(counts, dtype=np.uint64)
    t0 = time.perf_counter()
    net = eng.tagnet_build(data, cnt, len(seqs[0]), ppm)
    pairs, edges, deg = eng.tagnet_pairs(net)[0], eng.tagnet_edges(net, True)[0], eng.tagnet_degrees(net)
    wall = time.perf_counter() - t0
    stats, ms = net.stats, net.ms
    net.close()
    return pairs, edges, deg, stats, ms, wall


def fmt_ms(ms):
    return "  ".join("%s %.3f" % (k, v) for k, v in ms.items())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tags", type=int, default=1000000)
    ap.add_argument("--run", type=int, default=20000)
    ap.add_argument("--big-run", type=int, default=200000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tagpairs", "bench_mi355x.txt"))
    args = ap.parse_args(argv)
    eng = default_engine(args.device)
    rng = np.random.default_rng(20250)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("tag network, tools/tagpairs_bench.py --tags %d --run %d --big-run %d" % (args.tags, args.run, args.big_run))
    say("device ms: HIP events inside td_tagnet_build, best of %d; wall: build + fetch of pairs, kept edges, degrees" % args.repeat)
    device_network(eng, *one_run(rng, 2000))                      # warm-up: module load, first allocations

    def best_of(seqs, counts):
        runs = [device_network(eng, seqs, counts) for _ in range(args.repeat)]
        return min(runs, key=lambda r: sum(v for k, v in r[4].items() if k != "host_order"))

    def compare_with_host(label, seqs, counts):
        t0 = time.perf_counter()
        host = tf.tag_network(seqs, counts, backend="host")
        t_host = time.perf_counter() - t0
        pairs, edges, deg, stats, ms, wall = best_of(seqs, counts)
        same = ([tuple(map(int, e)) for e in pairs] == host.pairs and [tuple(map(int, e)) for e in edges] == host.edges and
                deg.tolist() == host.degree and all(stats[k] == host.stats[k] for k in host.stats if k not in ("compares", "backend")))
        if not same:
            raise SystemExit("%s: device and host results differ" % label)
        t0 = time.perf_counter()
        tf.tag_network(seqs, counts, backend="gpu")
        t_py = time.perf_counter() - t0
        say("%s: %d tags of %d bases: %s" % (label, len(seqs), len(seqs[0]), " ".join("%s=%d" % kv for kv in stats.items())))
        say("  device and host agree on pairs, kept edges, degrees and statistics")
        say("  device ms: %s" % fmt_ms(ms))
        say("  wall: device %.3f s (tag_network(backend='gpu') with its Python lists %.3f s), host backend %.3f s" % (wall, t_py, t_host))

    seqs, counts = synthetic_census(rng, args.tags, 64)
    compare_with_host("(a) census", seqs, counts)

    say()
    rate = None
    for m in (args.run, args.big_run):
        rs, rc = one_run(rng, m)
        pairs, edges, deg, stats, ms, wall = best_of(rs, rc)
        rate = stats["compares"] / (ms["compare"] * 1e-3)
        say("(b) one run of %d tags of 64 bases: compares=%d edges=%d pairs=%d" % (len(rs), stats["compares"], stats["edges"], stats["pairs"]))
        say("  device ms: %s" % fmt_ms(ms))
        say("  K4 rate: %.4g compares/s; wall %.3f s" % (rate, wall))
    say("  cap: K4 for 2 s at the rate of the longer run = 2 * %.4g = %.4g compares" % (rate, 2 * rate))

    say()
    short = {}
    for s, c in zip(seqs, counts):
        short[s[:32]] = short.get(s[:32], 0) + c
    ent = sorted(short.items(), key=lambda e: (-e[1], e[0]))
    compare_with_host("(c) the census at 32 bases", [e[0] for e in ent], [e[1] for e in ent])

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
