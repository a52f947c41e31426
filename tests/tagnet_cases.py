"""Shared by tests/test_tagnet.py and tests/test_tagnet_gpu.py: the tag network's rule stated by brute
force, and the inputs of the tests.

ref_network compares every tag with every other, base by base.  It is deliberately neither the host backend's method
(one dict lookup per tag, position and base) nor the device's (two sorts, comparing inside runs)."""
import csv
import functools
import io
import operator
import random

from census_cases import fastq

ACGT = "ACGT"
PPM = 30000                      # min_ratio = 0.03
GRID_L = (1, 2, 5, 31, 32, 33, 63, 64)
GRID_RATIO = (0, 0.03, 1)
STATS = ("tags", "edges", "kept", "deg0", "deg1", "hubs", "pairs")


def ref_network(seqs, counts, ppm):
    """dict(all_edges, edges (the kept ones), pairs, degree, stats) of the rule of DESIGN 4.13; O(n^2)."""
    n = len(seqs)
    all_edges, kept = [], []
    for i in range(n):
        a = seqs[i]
        for j in range(i + 1, n):
            if sum(map(operator.ne, a, seqs[j])) == 1:          # (sum(x != y for x, y in zip(a, b)), without the generator)
                all_edges.append((i, j))
                minor, major = min(counts[i], counts[j]), max(counts[i], counts[j])
                if minor * 1000000 >= ppm * major:
                    kept.append((i, j))
    degree = [0] * n
    for i, j in kept:
        degree[i] += 1
        degree[j] += 1
    pairs = [(i, j) for i, j in kept if degree[i] == 1 and degree[j] == 1]
    stats = dict(tags=n, edges=len(all_edges), kept=len(kept), deg0=sum(d == 0 for d in degree),
                 deg1=sum(d == 1 for d in degree), hubs=sum(d >= 2 for d in degree), pairs=len(pairs))
    return dict(all_edges=all_edges, edges=kept, pairs=pairs, degree=degree, stats=stats)


def rand_seq(rng, n):
    return "".join(rng.choice(ACGT) for _ in range(n))


def mutate(rng, s, k=None):
    """s with one base changed (at k, or at a random position)."""
    k = rng.randrange(len(s)) if k is None else k
    return s[:k] + rng.choice([b for b in ACGT if b != s[k]]) + s[k + 1:]


def census_order(census):
    """([seqs], [counts]) as a census lists them: count descending, then sequence."""
    ent = sorted(census.items(), key=lambda e: (-e[1], e[0]))
    return [e[0] for e in ent], [e[1] for e in ent]


def library(rng, L, nloci, err):
    """A synthetic census: nloci random loci with counts 50-400; half of them get a second allele at one random position
    (count 20-400), one in ten a third allele at that position; after each locus `err` error tags at distance 1 from a
    random existing tag, counts 1-3.  A sequence that exists already is left out (short tags run out of sequences)."""
    census = {}

    def add(s, c):
        if s not in census:
            census[s] = c

    for locus in range(nloci):
        s = rand_seq(rng, L)
        add(s, rng.randint(50, 400))
        if locus % 2 == 0:
            k = rng.randrange(L)
            add(mutate(rng, s, k), rng.randint(20, 400))
            if locus % 10 == 0:
                add(mutate(rng, s, k), rng.randint(20, 400))
        for _ in range(err):
            add(mutate(rng, rng.choice(sorted(census))), rng.randint(1, 3))
    return census_order(census)


@functools.lru_cache(maxsize=None)
def grid_case(L):
    """The input of the grid tests at tag length L (the same for every test of both files)."""
    seqs, counts = library(random.Random(7000 + L), L, 3 if L <= 2 else 60, 3)
    return tuple(seqs), tuple(counts)


@functools.lru_cache(maxsize=None)
def grid_ref(L, ppm):
    seqs, counts = grid_case(L)
    ref = ref_network(seqs, counts, ppm)
    if L >= 5 and ppm == PPM:
        assert_populated(ref)
    return ref


def assert_populated(ref):
    """Every class of the rule is there: an empty expectation must not pass by accident.  (Asked of every library()
    input at min_ratio = 0.03 from L = 5 on.  At L = 1 it cannot hold: there are four sequences, all neighbours of one
    another, and a pair takes two of them and leaves two, too few for a tag with two kept edges; the inputs at L <= 2
    are checked for edges, kept edges and cut edges instead.)"""
    st = ref["stats"]
    assert st["pairs"] > 0 and st["hubs"] > 0 and st["kept"] < st["edges"], st


@functools.lru_cache(maxsize=None)
def long_run_case(L, swapped):
    """(seqs, counts, reference at min_ratio = 0.03) of long_run, computed once for all the tests that use it."""
    seqs, counts = long_run(random.Random(99 + L + swapped), L, swapped)
    ref = ref_network(seqs, counts, PPM)
    assert len(seqs) > 1024
    assert_populated(ref)
    return seqs, counts, ref


def boundary_cases():
    """(seqs, counts, kept?) around min_ratio = 0.03: minor * 10^6 >= 30 000 * major in Python's integers."""
    big = 1 << 61
    least = -(-PPM * big // 1000000)             # ceil(0.03 * 2^61)
    assert least * 1000000 >= PPM * big > (least - 1) * 1000000
    return [(["ACGTACGTAC", "ACGTACGTAA"], [100, 3], True),
            (["ACGTACGTAC", "ACGTACGTAA"], [100, 2], False),
            (["ACGTACGTAC", "ACGTACGTAA"], [big, least], True),
            (["ACGTACGTAC", "ACGTACGTAA"], [least - 1, big], False)]


def long_run(rng, L, swapped, nrandom=1500, nplanted=300):
    """One run longer than a tile: nrandom tags that share part A = bases [0, ceil(L / 2)) with random parts B, plus
    nplanted neighbours at distance 1 inside B.  swapped: B is shared and A varies."""
    h = (L + 1) // 2
    fixed = rand_seq(rng, L - h if swapped else h)
    free = h if swapped else L - h
    parts = set()
    while len(parts) < nrandom:
        parts.add(rand_seq(rng, free))
    pool = sorted(parts)
    while len(parts) < nrandom + nplanted:
        parts.add(mutate(rng, rng.choice(pool)))
    census = {(p + fixed if swapped else fixed + p): rng.randint(1, 400) for p in sorted(parts)}
    return census_order(census)


def many_runs(rng, edge, L=16):
    """Runs of 1, 2, edge - 1, edge and edge + 1 tags (several of each) in one input: tags of a run share part A; the runs'
    parts A are neighbours of one another and the parts B come from one pool, so the (B, A) order has runs and edges
    of its own."""
    h = (L + 1) // 2
    lengths = [1, 2, edge - 1, edge, edge + 1, 1, edge + 1, 2, edge, edge - 1, 1]
    pool = set()
    while len(pool) < edge + 1:
        pool.add(rand_seq(rng, L - h))
    pool = sorted(pool)
    for _ in range(60):
        pool.append(mutate(rng, rng.choice(pool[:edge + 1])))
    pool = sorted(set(pool))
    heads = {rand_seq(rng, h)}
    while len(heads) < len(lengths):
        cand = mutate(rng, rng.choice(sorted(heads)))
        heads.add(cand)
    census = {}
    for a, m in zip(sorted(heads), lengths):
        for b in rng.sample(pool, m):
            census[a + b] = rng.randint(1, 400)
    return census_order(census)


def merged(major, minor):
    """The merged string of two tags that differ at one position: ...[X/Y]..."""
    k = next(i for i, (x, y) in enumerate(zip(major, minor)) if x != y)
    return major[:k] + "[" + major[k] + "/" + minor[k] + "]" + major[k + 1:]


def check_against(ref, got):
    assert got.pairs == ref["pairs"]
    assert got.edges == ref["edges"]
    assert list(got.degree) == ref["degree"]
    assert {k: got.stats[k] for k in STATS} == ref["stats"]


def write_census(path, seqs, counts):
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Tag sequence", "Count", "Known tags"])
        for s, c in zip(seqs, counts):
            w.writerow([s, c, ""])


def expected_file(seqs, counts, ref, prefix="Mrkr", numdig=7):
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(["Marker name", "Tag sequence", "Count 0", "Count 1"])
    for k, (i, j) in enumerate(ref["pairs"]):
        w.writerow(["%s%0*d" % (prefix, numdig, 1 + k), merged(seqs[i], seqs[j]), counts[i], counts[j]])
    return buf.getvalue().encode()


def expected_line(ref):
    return "Tags: {tags} Edges: {edges} Kept: {kept} Hubs: {hubs} Pairs: {pairs}".format(**ref["stats"])


BARCODES = ["ACGT", "TGACA"]


def library_fastq(rng, seqs, counts, barcodes=BARCODES, site="TGCAG"):
    """FASTQ bytes whose census under `barcodes` is {site + s: c}: every tag c times, spread over the barcodes, with a
    random tail behind it; plus some reads without a barcode."""
    reads = []
    for s, c in zip(seqs, counts):
        for _ in range(c):
            reads.append(rng.choice(barcodes) + site + s + rand_seq(rng, rng.randint(0, 20)))
    reads += [rand_seq(rng, 60) for _ in range(40)]
    rng.shuffle(reads)
    return fastq(reads)
