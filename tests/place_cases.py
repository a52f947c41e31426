"""Tag placement stated by brute force, and the cases tests/test_place.py and tests/test_place_gpu.py share.

The restatement uses plain loops over every position, both strands and every tag x locus pair: no parts, no sorting,
no dicts of windows, so it shares nothing with tagdigger_fun._place_host or csrc/place.hip."""
import functools
import random

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
NONE, NO_LOCUS = 255, 0xFFFFFFFFFFFFFFFF
SCAN_TILE, SCAN_HALO = 4096, 64       # csrc/place.hip: tile t of the site scan covers x in [4096 t - 64, 4096 t + 4032)
CHUNK = 1024                          # csrc/place.hip: PL_CHUNK, the windows of a run that one wave compares


def rc(s):
    return "".join(COMP.get(c, c) for c in reversed(s))


def parse_fasta(text):
    """(G, names, rec_start) by the genome rule: headers start records, every other line is strip().upper()."""
    G, names, starts = [], [], []
    n = 0
    for line in text.splitlines():
        if line.startswith(">"):
            names.append((line[1:].split() or [""])[0])
            starts.append(n)
        else:
            s = line.strip().upper()
            G.append(s)
            n += len(s)
    return "".join(G), names, starts + [n]


def fasta(records, width=60):
    out = []
    for name, seq in records:
        out.append(">" + name)
        out.extend(seq[i:i + width] for i in range(0, len(seq), width))
    return "\n".join(out) + "\n"


def record_of(rec_start, v):
    for r in range(len(rec_start) - 1):
        if rec_start[r] <= v < rec_start[r + 1]:
            return r
    raise AssertionError("no record holds offset %d" % v)


def ref_sites(G, rec_start, remnants, L):
    """The loci in id order and the statistics, position by position."""
    loci = []
    stats = dict(loci=0, forward=0, reverse=0, distinct=0, dropped_bounds=0, dropped_alphabet=0, records=len(rec_start) - 1)

    def decide(x, r, strand):
        if x < rec_start[r] or x + L > rec_start[r + 1]:
            stats["dropped_bounds"] += 1
            return
        w = G[x:x + L]
        if any(c not in "ACGT" for c in w):
            stats["dropped_alphabet"] += 1
            return
        loci.append((x, strand, r, rc(w) if strand else w))

    for x in range(len(G)):
        if any(G[x:x + len(c)] == c for c in remnants):
            decide(x, record_of(rec_start, x), 0)
    for z in range(1, len(G) + 1):                    # the window's end on the forward strand
        if any(z >= len(c) and G[z - len(c):z] == rc(c) for c in remnants):
            decide(z - L, record_of(rec_start, z - 1), 1)
    loci.sort(key=lambda e: (e[0], e[1]))
    stats["loci"] = len(loci)
    stats["forward"] = sum(1 for e in loci if e[1] == 0)
    stats["reverse"] = sum(1 for e in loci if e[1] == 1)
    stats["distinct"] = len({e[3] for e in loci})
    return dict(x=[e[0] for e in loci], strand=[e[1] for e in loci], rec=[e[2] for e in loci], windows=[e[3] for e in loci],
                pos1=[e[0] - rec_start[e[2]] + 1 for e in loci],
                cutpos=[e[0] - rec_start[e[2]] + 1 + (L - 1) * e[1] for e in loci], stats=stats)


def ref_place(tags, windows, L, k):
    """n_at, dist, locus, status and compares of every tag against every locus."""
    n_at, dist, locus, status = [], [], [], []
    for t in tags:
        row, first = [0, 0, 0, 0], [NO_LOCUS] * 4
        for i, w in enumerate(windows):
            d = 0
            for a, b in zip(t, w):
                d += a != b
            if d <= k:
                row[d] += 1
                first[d] = min(first[d], i)
        best = [d for d in range(k + 1) if row[d]]
        n_at.append(row)
        dist.append(best[0] if best else NONE)
        locus.append(first[best[0]] if best else NO_LOCUS)
        status.append("none" if not best else "unique" if row[best[0]] == 1 else "multi")
    compares = 0
    uniq = sorted(set(windows))
    for p in range(k + 1):
        lo, hi = p * L // (k + 1), (p + 1) * L // (k + 1)
        for t in tags:
            for w in uniq:
                compares += t[lo:hi] == w[lo:hi]
    return dict(n_at=n_at, dist=dist, locus=locus, status=status, compares=compares)


# ------------------------------------------------------------------ site-scan cases: (id, fasta text, cut site, L)
def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def plant(seq, at, what):
    assert 0 <= at and at + len(what) <= len(seq)
    return seq[:at] + what + seq[at + len(what):]


def edge_case(off):
    """TGCAG and its reverse complement `off` bases from a scan-tile edge and from a 16-byte load edge, each both as the
    remnant's own position and as the position of the window it gives on the reverse strand."""
    rng = random.Random(100 + off)
    L = 20
    g = rand_seq(rng, 3 * SCAN_TILE)
    edge1, edge2, edge16 = SCAN_TILE - SCAN_HALO, 2 * SCAN_TILE - SCAN_HALO, 16 * 125
    g = plant(g, edge1 + off, "TGCAG")                       # forward, x at the edge
    g = plant(g, edge2 + off, "CTGCA")                       # reverse, the remnant at the edge
    g = plant(g, edge2 + 300 + off + L - 5, "CTGCA")         # reverse, x = edge2 + 300 + off ...
    g = plant(g, edge1 + 1000 + off, "CTGCA")
    g = plant(g, edge16 + off, "TGCAG")
    g = plant(g, edge16 + 160 + off + L - 5, "CTGCA")        # reverse, x at a 16-byte edge
    return ("edge%+d" % off, fasta([("chrA", g)]), "TGCAG", L)


def bounds_case():
    rng = random.Random(7)
    L = 16
    body = lambda n: rand_seq(rng, n, "AC")                  # (no G, no T: no remnant by chance on either strand)
    recs = [("q", "CTGCA" + body(20)),                       # reverse: the window would start before the genome
            ("r0", "TGCAG" + body(30)),                      # a window that starts at s_r
            ("r1", body(20) + "TGCAG" + body(11)),           # ends exactly at e_r
            ("r2", body(20) + "TGCAG" + body(10)),           # one base past e_r: dropped
            ("r3", body(20) + "TGCAG" + body(3)),            # spans two records
            ("r4", body(40)),
            ("r5", body(11) + "CTGCA" + body(20)),           # reverse: starts exactly at s_r
            ("r6", body(10) + "CTGCA" + body(20)),           # reverse: one base before s_r: dropped
            ("r7", "CTGCA" + body(20)),                      # reverse: reaches into the record before
            ("r8", body(20) + "TGCAG"),                      # the last record's window leaves the genome
            ("empty", ""),
            ("r9", "TGC"), ("r10", "AG" + body(30))]         # a remnant across two records is no site
    return ("bounds", fasta(recs, width=25), "TGCAG", L)


def alphabet_case():
    rng = random.Random(8)
    L = 12
    recs = []
    for i in range(L):
        for ch in ("N", "r"):
            w = plant("TGCAG" + rand_seq(rng, L - 5, "AC"), i, ch)
            recs.append(("f%d%s" % (i, ch), rand_seq(rng, 9, "AC") + w + rand_seq(rng, 9, "AC")))
            recs.append(("b%d%s" % (i, ch), rand_seq(rng, 9, "AC") + rc(w) + rand_seq(rng, 9, "AC")))
    recs.append(("clean", rand_seq(rng, 9, "AC") + "TGCAG" + rand_seq(rng, 20, "AC")))
    return ("alphabet", fasta(recs), "TGCAG", L)


def overlap_case():
    return ("overlap", fasta([("c", "AATGCAGTGCAGTGCAGAACCAACCAACTGCACTGCACTGCAAA")]), "TGCAG", 8)


def palindrome_case():
    return ("palindrome", fasta([("c", "AACCGATCGATCAACCAAGATCAACC"), ("d", "GATCAAAAGATCGATC")]), "GATC", 8)


def cwgc_case():
    rng = random.Random(9)
    return ("cwgc", fasta([("one", rand_seq(rng, 1500)), ("two", rand_seq(rng, 1700))]), "CWGC", 10)


def many_records_case():
    rng = random.Random(10)
    recs = []
    for r in range(1000):
        s = rand_seq(rng, 70)
        if r % 3 == 0:
            s = plant(s, rng.choice([0, 3, 6, 7]), "TGCAG")
        if r % 5 == 0:
            s = plant(s, rng.choice([58, 61, 64, 65]), "CTGCA")
        recs.append(("s%04d" % r, s))
    return ("records1000", fasta(recs, width=70), "TGCAG", 64)


def short_case():
    return ("shorter_than_L", fasta([("c", "TGCAGACCTGCA")]), "TGCAG", 20)


def empty_cases():
    return [("header_only", ">c\n", "TGCAG", 20), ("empty_file", "", "TGCAG", 20)]


def whole_tag_site_case():
    rng = random.Random(11)
    site = "TGCAG" + rand_seq(rng, 59)
    g = rand_seq(rng, 100) + site + rand_seq(rng, 37) + rc(site) + rand_seq(rng, 50) + site[:63]
    return ("site_of_64", fasta([("c", g)]), site, 64)


@functools.lru_cache(maxsize=None)
def site_cases():
    return tuple([edge_case(off) for off in range(-5, 6)] +
                 [bounds_case(), alphabet_case(), overlap_case(), palindrome_case(), cwgc_case(), many_records_case(), short_case()] +
                 empty_cases() + [whole_tag_site_case()])


def remnants_of(cutsite):
    out = [cutsite]
    for code, bases in (("W", "AT"), ("S", "CG"), ("N", "ACGT")):
        while code in out[0]:
            out = [x.replace(code, b, 1) for b in bases for x in out]
    return out


@functools.lru_cache(maxsize=None)
def site_ref(case_id):
    _, text, cutsite, L = next(c for c in site_cases() if c[0] == case_id)
    G, names, rec_start = parse_fasta(text)
    ref = ref_sites(G, rec_start, remnants_of(cutsite), L)
    ref["names"], ref["rec_start"] = names, rec_start
    return ref


# ------------------------------------------------------------------ join cases: (fasta text, cut site, L, k, tags)
GRID_L = (5, 16, 31, 32, 33, 63, 64)
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def mutate(s, positions):
    for i in positions:
        s = s[:i] + OTHER[s[i]] + s[i + 1:]
    return s


def site_for(L):
    return "TGCAG"[:max(1, min(5, L // 2))]


def parts_of(L, k):
    return [(p * L // (k + 1), (p + 1) * L // (k + 1)) for p in range(k + 1)]


def windows_genome(windows, reverse=()):
    """One record per window (its forward locus starts the record); the windows of `reverse` lie reverse-complemented."""
    recs = [("w%d" % i, w) for i, w in enumerate(windows)]
    recs += [("v%d" % i, rc(w)) for i, w in enumerate(reverse)]
    return fasta(recs, width=64)


@functools.lru_cache(maxsize=None)
def join_case(L, k):
    """Windows behind the site and tags around three of them: every single mismatch, mismatches that leave each part in
    turn as the lowest one that agrees, k + 1 mismatches spread over the parts and packed into one, equal tags."""
    rng = random.Random(1000 * L + k)
    site = site_for(L)
    windows = []
    while len(windows) < min(10, 4 ** (L - len(site))):
        w = site + rand_seq(rng, L - len(site))
        if w not in windows:
            windows.append(w)
    parts = parts_of(L, k)
    tags = []
    for w in windows[:3]:
        tags.append(w)
        tags.extend(mutate(w, [i]) for i in range(L))
        for q in range(k + 1):                                # part q is the lowest that agrees; the parts above it too
            below = [lo for lo, hi in parts[:q]]
            tags.append(mutate(w, below))
            others = [hi - 1 for p, (lo, hi) in enumerate(parts) if p != q]       # ... and no other part agrees
            tags.append(mutate(w, others))
        tags.append(mutate(w, [lo for lo, hi in parts]))      # k + 1 mismatches, one in every part
        lo, hi = max(parts, key=lambda p: p[1] - p[0])
        if hi - lo >= k + 1:
            tags.append(mutate(w, range(lo, lo + k + 1)))     # k + 1 mismatches inside one part
    tags.append(tags[1])                                      # equal tags
    tags.append(tags[0])
    tags.append(rand_seq(rng, L))
    return windows_genome(windows, reverse=windows[3:5]), site, L, k, tuple(tags)


@functools.lru_cache(maxsize=None)
def multiplicity_case():
    """A window present 1, 2 and 300 times, and one that lies on both strands."""
    rng = random.Random(77)
    L, k = 24, 2
    a, b, c, d = ("TGCAG" + rand_seq(rng, L - 5) for _ in range(4))
    windows = [c] * 150 + [a] + [b] + [c] * 100 + [b] + [c] * 50 + [d]
    tags = [a, b, c, d, mutate(a, [7]), mutate(b, [5, 20]), mutate(c, [23]), mutate(c, [0, 11]), mutate(d, [9]), mutate(d, [1, 2, 3])]
    return windows_genome(windows, reverse=[d]), "TGCAG", L, k, tuple(tags)


@functools.lru_cache(maxsize=None)
def long_run_case(m, k):
    """m distinct windows of 64 bases that share part 0 of k + 1 (and the tag's other parts differ from most of them)."""
    rng = random.Random(5000 + m + k)
    L = 64
    lo, hi = parts_of(L, k)[0]
    head = "TGCAG" + rand_seq(rng, hi - 5)
    windows = set()
    while len(windows) < m:
        windows.add(head + rand_seq(rng, L - hi))
    windows = sorted(windows)
    rng.shuffle(windows)
    picks = [windows[0], windows[m // 2], windows[-1]]
    tags = [mutate(w, [L - 1 - j for j in range(d)]) for w in picks for d in range(k + 2)]
    tags.append(head + rand_seq(rng, L - hi))
    return windows_genome(windows), "TGCAG", L, k, tuple(tags)


LONG_RUNS = (63, 64, 65, 255, 256, 257, 600, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 52)


@functools.lru_cache(maxsize=None)
def join_ref(kind, *args):
    text, site, L, k, tags = {"grid": join_case, "mult": multiplicity_case, "run": long_run_case}[kind](*args)
    G, names, rec_start = parse_fasta(text)
    sites = ref_sites(G, rec_start, remnants_of(site), L)
    ref = ref_place(tags, sites["windows"], L, k)
    ref["sites"] = sites
    ref["names"] = names
    return ref


def check_sites(ref, got):
    """A CutSites against ref_sites' answer."""
    assert {k: got.stats[k] for k in ref["stats"]} == ref["stats"]
    assert got.x.tolist() == ref["x"] and got.rec.tolist() == ref["rec"] and got.strand.tolist() == ref["strand"]
    assert got.pos1.tolist() == ref["pos1"] and got.cutpos.tolist() == ref["cutpos"]
    assert list(got.windows()) == ref["windows"]
    assert got.names == ref["names"] and got.rec_start == ref["rec_start"]


def check_placed(ref, got):
    """A PlacementResult against ref_place's answer."""
    assert got.n_at == ref["n_at"]
    assert got.dist == ref["dist"] and got.locus == ref["locus"] and got.status == ref["status"]
    sites = ref["sites"]
    for t, i in enumerate(ref["locus"]):
        if i == NO_LOCUS:
            assert got.chrom[t] is None and got.pos[t] is None and got.cutpos[t] is None and got.strand[t] is None
        else:
            assert got.chrom[t] == ref["names"][sites["rec"][i]] and got.pos[t] == sites["pos1"][i]
            assert got.cutpos[t] == sites["cutpos"][i] and got.strand[t] == ("bot" if sites["strand"][i] else "top")
    assert got.stats["compares"] == ref["compares"]
    for s in ("unique", "multi", "none"):
        assert got.stats[s] == ref["status"].count(s)


# ------------------------------------------------------------------ the chain: a genome, a library cut from it, planted SNPs
BARCODES = ["ACGT", "TGCAA", "GATTCA"]


@functools.lru_cache(maxsize=None)
def chain_case():
    """Three chromosomes without G or T but for what is planted: at every 450 bases a PstI site with a window behind it,
    alternately on the forward and on the reverse strand, and a CTGCAG that closes its fragment.  Each site is a marker
    with two alleles, the genome's and one substitution.  -> (fasta text, L, {(chrom, cut position, strand): [tags]},
    {tag: expected fragment size with CTGCAG as the only cut site}, {(barcode, tag): reads}, FASTQ bytes)."""
    rng = random.Random(2026)
    L = 40
    chroms, planted, frag = [], {}, {}
    for c in range(3):
        name = "chr%d" % (c + 1)
        g = rand_seq(rng, 3000, "AC")
        for s in range(6):
            at = 300 + 450 * s
            w = "TGCAG" + rand_seq(rng, L - 5, "AC")
            alt = mutate(w, [8 + 5 * s])
            if s % 2 == 0:
                g = plant(g, at, w)
                g = plant(g, at + 120 + 10 * s, "CTGCAG")
                key, size = (name, at + 1, "top"), 126 + 10 * s
            else:
                g = plant(g, at, rc(w))
                g = plant(g, at - 100 - 10 * s, "CTGCAG")
                key, size = (name, at + L, "bot"), L + 100 + 10 * s
            planted[key] = sorted([w, alt])
            frag[w] = frag[alt] = size
        chroms.append((name, g))
    # exp_frag_size searches a record when the next header arrives (the reference's header loop, kept as it is), so the
    # tags of a genome's last record get NA: a last record without sites stands behind the three that carry them
    chroms.append(("scaffold_end", rand_seq(rng, 90, "AC")))
    reads, counts = [], {}
    for tags in planted.values():
        for t in tags:
            for b in BARCODES:
                counts[(b, t)] = rng.randint(2, 5)
                reads += [b + t + rand_seq(rng, rng.randint(0, 15), "AC") for _ in range(counts[(b, t)])]
    rng.shuffle(reads)
    fq = "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads)).encode("ascii")
    return fasta(chroms), L, planted, frag, counts, fq
