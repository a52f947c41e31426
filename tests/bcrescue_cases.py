"""Shared by tests/test_bcrescue.py and tests/test_bcrescue_gpu.py: the barcode-rescue rule restated by brute force --
every surviving entry against every read, Python strings, no index -- with the oracle's tree for which entries survive
and its line splitting; builders of the inputs, each asserting the property it is named for.  An input is a Case: FASTQ
bytes with the lists td_bcrescue_begin takes."""
import collections
import math
import random

import rescue_cases as rc
from oracle import tagdigger_oracle as orc

ACGT = "ACGT"
CLASSES = ("reads", "exact", "rescued1", "rescued2", "ambiguous", "none")
STATS = CLASSES + ("tagged", "min_entry_distance")
NPOS = 32
NO_PAIR = 64
TILE = 16384
BARCODES_MIXED = rc.BARCODES_MIXED                                   # lengths 4..9, prefix-free
LDS_INDEX = 40 * 1024                                                # the module's share of a workgroup's LDS (include/tagdig.h)
SKIP_REASONS = ("weights", "long_tag", "tags_overlap", "short_entry")

Case = collections.namedtuple("Case", "data barcut barnum tagoff stored")
Limit = rc.Limit
rand_seq, other, sub, fastq, free_tags = rc.rand_seq, rc.other, rc.sub, rc.fastq, rc.free_tags


# ------------------------------------------------------------------------------------------------------------ the rule
def entries_of(barcut, barnum):
    """The entries the index build leaves, in list order, as (sequence, row): the leaves of the oracle's tree."""
    tree = orc.build_sequence_tree(barcut, barnum)
    found = []

    def walk(node, path):
        if node is None:
            return
        if node[0] == "leaf":
            found.append((path, node[1]))
            return
        for c, child in zip(ACGT, node[1]):
            walk(child, path + c)
    walk(tree, "")
    if barnum == 1 and list(barcut) == [""]:
        return sorted(set(found))
    return sorted(found, key=lambda e: list(barcut).index(e[0]))


def distance(read, entry):
    """positions of the entry that differ from the read (the read is at least as long)"""
    return [i for i in range(len(entry)) if read[i] != entry[i]]


def min_entry_distance(entries):
    best = NO_PAIR
    for i, (a, ra) in enumerate(entries):
        for b, rb in entries[i + 1:]:
            if ra != rb:
                n = min(len(a), len(b))
                best = min(best, len(distance(a[:n], b[:n])))
    return best


def check_begin(barcut, barnum, stored, K):
    """the begin checks in td_bcrescue_begin's order -> the entries"""
    entries = entries_of(barcut, barnum)
    rc.check_tags(stored)
    for seq, _ in entries:
        if len(seq) <= 2 * K:
            raise Limit("barcode rescue: entry")
    return entries


def classify(read, entries, K):
    """(class, entry, mismatching positions) of a stripped, upper-cased read line"""
    if any(read.startswith(e) for e, _ in entries):
        return "exact", -1, ()
    cand = [(len(distance(read, e)), k) for k, (e, _) in enumerate(entries) if len(e) <= len(read)]
    if not cand:
        return "none", -1, ()
    m = min(d for d, _ in cand)
    assert m >= 1
    if m > K:
        return "none", -1, ()
    hits = [k for d, k in cand if d == m]
    if len({entries[k][1] for k in hits}) > 1:
        return "ambiguous", -1, ()
    return "rescued%d" % m, hits[0], tuple(distance(read, entries[hits[0]][0]))


def ref_lists(data, barcut, barnum, tagoff, stored, K, maxreads=5e9, first_line=0, min_distance=True):
    """(matrix, statistics, row_rescued, positions) of FASTQ bytes whose first line has index first_line.  (min_distance
    False leaves min_entry_distance out: all pairs of a few thousand entries take Python too long.)"""
    entries = check_begin(barcut, barnum, stored, K)
    bound = max(1, math.ceil(maxreads))             # (the reference tests readscount >= maxreads after a read)
    matrix = [[0] * len(stored) for _ in range(barnum)]
    rows = [[0, 0] for _ in range(barnum)]
    positions = [0] * NPOS
    st = dict.fromkeys(CLASSES + ("tagged",), 0)
    memo = {}
    for k, raw in enumerate(orc.iter_lines(data), first_line):
        if k % 4 != 1:
            continue
        if k > 4 * (bound - 1) + 1:
            break
        st["reads"] += 1
        read = orc.clean_read(raw)
        if read not in memo:
            memo[read] = classify(read, entries, K)
        kind, e, where = memo[read]
        st[kind] += 1
        if e < 0:
            continue
        b = entries[e][1]
        rows[b][len(where) - 1] += 1
        for i in where:
            positions[i] += 1
        w = read[tagoff[b]:]
        hits = [t for t, tag in enumerate(stored) if w.startswith(tag)]
        assert len(hits) <= 1
        if hits:
            matrix[b][hits[0]] += 1
            st["tagged"] += 1
    assert st["reads"] == st["exact"] + st["rescued1"] + st["rescued2"] + st["ambiguous"] + st["none"]
    assert st["tagged"] == sum(map(sum, matrix)) and st["rescued1"] == sum(r[0] for r in rows) and st["rescued2"] == sum(r[1] for r in rows)
    if min_distance:
        st["min_entry_distance"] = min_entry_distance(entries)
    return matrix, st, rows, positions


def ref_case(case, K, maxreads=5e9, min_distance=True):
    return ref_lists(case.data, case.barcut, case.barnum, case.tagoff, case.stored, K, maxreads, min_distance=min_distance)


def oracle_barcut_reads(data, barcut, barnum, maxreads=5e9):
    """the reads with barcode + cut site that the oracle's own lookup finds"""
    tree = orc.build_sequence_tree(barcut, barnum)
    bound = max(1, math.ceil(maxreads))
    n = 0
    for k, raw in enumerate(orc.iter_lines(data)):
        if k % 4 == 1 and k <= 4 * (bound - 1) + 1:
            n += orc.sequence_index_lookup(orc.clean_read(raw), tree) != -1
    return n


def lists(barcodes, tags, cutsite="TGCAG"):
    barcut, barnum, stored, tagoff = orc.prepare_lists(barcodes, tags, cutsite)
    return barcut, barnum, tagoff, stored


def make(reads, barcodes, tags, cutsite="TGCAG", **kw):
    return Case(fastq(reads, **kw), *lists(barcodes, tags, cutsite))


def golden_plan(case, directory, K):
    """What a recorded hot-path payload asks of the barcode rescue at K -> (what, value, path): 'skip' with one of
    SKIP_REASONS, 'raises' with the exception the set-up or the missing file raises, or 'run' with the FASTQ bytes."""
    import os
    from conftest import write_case_file
    kw = case["kwargs"]
    write_case_file(case, directory)
    path = os.path.join(str(directory), case.get("filename_override") or case["filename"])
    if kw.get("tassel_tagcount"):
        return "skip", "weights", path
    try:
        barcut, barnum, stored, _ = orc.prepare_lists(case["barcodes"], case["tags"], kw.get("cutsite", "TGCAG"))
    except AssertionError as exc:
        return "raises", exc, path
    try:
        entries = entries_of(barcut, barnum)
    except (AssertionError, IndexError) as exc:
        return "raises", exc, path
    try:
        rc.check_tags(stored)
    except Limit:
        return "skip", "long_tag", path
    except AssertionError:
        return "skip", "tags_overlap", path
    except IndexError as exc:
        return "raises", exc, path
    if any(len(e) <= 2 * K for e, _ in entries):
        return "skip", "short_entry", path
    if not os.path.exists(path):
        return "raises", FileNotFoundError(), path
    return "run", orc.read_fastq_bytes(path), path


# payloads skipped by reason at K, from the host rule alone (tests/test_bcrescue.py holds the host rule to them)
GOLDEN_SKIPS = {1: {"weights": 3, "long_tag": 0, "tags_overlap": 3, "short_entry": 2},
                2: {"weights": 3, "long_tag": 0, "tags_overlap": 3, "short_entry": 11}}


def check(got, want):
    """(matrix, statistics with row_rescued and positions) as rescue_barcodes_fastq returns them, against ref_lists"""
    matrix, st = got
    assert {k: st[k] for k in want[1]} == want[1]
    assert matrix == want[0]
    assert st["row_rescued"] == want[2]
    assert st["positions"] == want[3]


def golden_payloads(tmp_path, cases, K, run):
    """Every payload at K through run(path, (barcodes, tags, cutsite), maxreads) -> (payloads that ran, skips by reason).
    A payload that is skipped for its tags or its entries is one that `run` itself refuses."""
    import pytest
    from tagdigger_amd import NonAsciiSequence, TagdigError
    refusal = {"long_tag": TagdigError, "tags_overlap": AssertionError, "short_entry": ValueError}
    ran, skips = 0, dict.fromkeys(SKIP_REASONS, 0)
    for k, case in enumerate(cases):
        kw = case["kwargs"]
        d = tmp_path / ("g%d_%d" % (K, k))
        d.mkdir()
        what, value, path = golden_plan(case, d, K)
        args = (case["barcodes"], case["tags"], kw.get("cutsite", "TGCAG"))
        maxreads = kw.get("maxreads", 5e9)
        if what == "skip":
            skips[value] += 1
            if value in refusal:
                with pytest.raises(refusal[value]):
                    run(path, args, maxreads)
            continue
        ran += 1
        if what == "raises":
            with pytest.raises(type(value)):
                run(path, args, maxreads)
            continue
        begin = lists(*args)
        try:
            want = ref_lists(value, *begin, K, maxreads)
        except orc.NonAsciiSequence:
            with pytest.raises(NonAsciiSequence):
                run(path, args, maxreads)
            continue
        # step 1 is the counter's lookup: the reads with barcode + cut site that the oracle finds
        assert want[1]["exact"] == oracle_barcut_reads(value, begin[0], begin[1], maxreads), case["name"]
        check(run(path, args, maxreads), want)
    return ran, skips


def lds_bytes(n):
    """what an index of n distinct entries of 5 bases or more takes of the module's LDS share (include/tagdig.h)"""
    return (8 * n + (4 * n + 7) // 8 * 8 + 2048 + 15) // 16 * 16 + 2 * n


def largest_index():
    n = 1
    while lds_bytes(n + 1) <= LDS_INDEX:
        n += 1
    return n


# ------------------------------------------------------------------------------------------------------------ inputs
def some_tags(rnd, n=6, length=40):
    bodies = free_tags(rnd, [length] * n)
    return bodies, ["TGCAG" + b for b in bodies]


def geometry_case(K, seed=41):
    """Barcodes of every length 4..9 before a 5-base site.  Per entry: one substitution and one N at every position (the
    first and the last base named), two substitutions both in the barcode, both in the site and one in each, and K + 1
    substitutions."""
    rnd = random.Random(seed + K)
    bodies, tags = some_tags(rnd)
    reads = []
    for b in BARCODES_MIXED:
        e = b + "TGCAG"
        n, nb = len(e), len(b)
        first, last = sub(e, 0), sub(e, n - 1)
        assert distance(first, e) == [0] and distance(last, e) == [n - 1]
        heads = [first, last] + [sub(e, i) for i in range(n)] + [sub(e, i, to="N") for i in range(n)]
        heads += [sub(e, 0, nb - 1), sub(e, nb, n - 1), sub(e, 1, nb + 1), sub(e, 0, to="N")[:nb] + sub(e[nb:], 2)]
        heads += [sub(e, *range(0, 2 * (K + 1), 2))]
        assert len(distance(heads[-1], e)) == K + 1
        reads += [h + rnd.choice(bodies) + rand_seq(rnd, 7) for h in heads]
    rnd.shuffle(reads)
    return make(reads, BARCODES_MIXED, tags)


def long_entries_case(K, seed=42):
    """entries of 31 and of 32 bases: one substitution and one N at every position, two at the ends"""
    rnd = random.Random(seed)
    a, b = rand_seq(rnd, 31), rand_seq(rnd, 32)
    stored = free_tags(rnd, [30] * 4)
    reads = []
    for e in (a, b):
        n = len(e)
        heads = [e] + [sub(e, i) for i in range(n)] + [sub(e, i, to="N") for i in range(n)] + [sub(e, 0, n - 1), sub(e, n - 2, n - 1), sub(e, 0, 15, n - 1)]
        reads += [h + rnd.choice(stored) + "AC" for h in heads] + [sub(e, n - 1), sub(e, n - 1)[:n - 1]]
    return Case(fastq(reads), [a, b], 2, [31, 32], stored)


def near_and_far_case(seed=43):
    """a read at distance 1 from one row and 2 from another goes to the nearer; at 1 from both it is ambiguous"""
    rnd = random.Random(seed)
    bodies, tags = some_tags(rnd)
    bars = ["AAAAA", "AACCC", "GGTGT"]
    first, second, other_way = "AACAA" + "TGCAG", "AAACA" + "TGCAG", "AAACC" + "TGCAG"
    e0, e1 = "AAAAATGCAG", "AACCCTGCAG"
    assert (len(distance(first, e0)), len(distance(first, e1))) == (1, 2)
    assert (len(distance(second, e0)), len(distance(second, e1))) == (1, 2)
    assert (len(distance(other_way, e0)), len(distance(other_way, e1))) == (2, 1)
    reads = [h + bodies[k % 6] + "GATC" for k, h in enumerate([first, second, other_way, "AACACTGCAG", "AAACCTGCAN", "AACAATGCNG"])]
    return make(reads, bars, tags)


def read_length_case(seed=44):
    """one base shorter than the entry (no candidate), exactly the entry (no tag window), the entry and a tag cut one base short"""
    rnd = random.Random(seed)
    bodies, tags = some_tags(rnd)
    e = "GATTAC" + "TGCAG"
    h = sub(e, 2)
    reads = [h[:-1], h, h + bodies[0][:-1], h + bodies[0], h + "  ", h[:-1] + " ", h + bodies[1] + "\t", "  " + h + bodies[2], h[:4]]
    return make(reads, ["GATTAC"], tags)


def two_rows_tie_case(seed=45):
    rnd = random.Random(seed)
    bodies, tags = some_tags(rnd)
    head = "AAAAC" + "TGCAG"
    assert len(distance(head, "AAAAATGCAG")) == 1 == len(distance(head, "AAACCTGCAG"))
    return make([head + bodies[0], head, "AAAAG" + "TGCAG" + bodies[1]], ["AAAAA", "AAACC"], tags)


def variants_tie_case(seed=46):
    """Two entries of ONE row at the same distance, mismatching at different positions, the later one first in the
    directory's order: rescued, with the earlier entry's position."""
    rnd = random.Random(seed)
    stored = free_tags(rnd, [30] * 3)
    barcut = ["TCGTCCGG", "TCGTAAGG"]                    # one row: k % 1
    head = "TCGTACGG"
    assert distance(head, barcut[0]) == [4] and distance(head, barcut[1]) == [5]
    reads = [head + stored[0] + "A", head + stored[1], "TCGTCAGG" + stored[2]]
    return Case(fastq(reads), barcut, 1, [8], stored)


def degenerate_site_case(K, seed=47):
    """a degenerate cut site: a substitution on the degenerate base ties the two variants of one row"""
    rnd = random.Random(seed)
    bodies = free_tags(rnd, [36] * 5)
    tags = [rnd.choice(("CAGC", "CTGC")) + b for b in bodies]
    reads = []
    for b in BARCODES_MIXED:
        for site in ("CGGC", "CCGC", "CAGC", "CTGG", "NTGC"):
            reads.append(b + site + rnd.choice(bodies))
        reads.append(sub(b, 1) + rnd.choice(tags))
    return make(reads, BARCODES_MIXED, tags, "CWGC")


def length_trap_case(seed=48):
    """ACGT + site and ACGTT + site, two rows, both at distance 1 from one read"""
    rnd = random.Random(seed)
    bodies = free_tags(rnd, [30] * 3)
    tags = ["TTAA" + b for b in bodies]
    head = "ACGTTTCAA"
    assert distance(head, "ACGT" + "TTAA") == [6] and distance(head, "ACGTT" + "TTAA") == [6]
    return make([head + bodies[0], "ACGTTTAAC" + bodies[1], "ACGTATTAA" + bodies[2]], ["ACGT", "ACGTT"], tags, "TTAA")


def shadow_case(seed=49):
    """a duplicate and an extension of the first entry under other rows: neither survives, neither creates a tie"""
    rnd = random.Random(seed)
    stored = free_tags(rnd, [30] * 3)
    e0, e1 = "ACGTTGCAG", "GGATCTGCAG"
    barcut = [e0, e1, e0, e0 + "AC"]
    assert [e for e, _ in entries_of(barcut, 4)] == [e0, e1]
    reads = [sub(e0, 3) + stored[0], sub(e0, 3) + "AC" + stored[1], sub(e1, 0) + stored[2], e0 + stored[0]]
    return Case(fastq(reads), barcut, 4, [9, 10, 9, 11], stored)


def dirt_case(K, seed=50):
    """leading and trailing blanks, lower case, blanks inside the head"""
    rnd = random.Random(seed)
    bodies, tags = some_tags(rnd)
    e = "TGACA" + "TGCAG"
    reads = ["  \t " + sub(e, 1) + bodies[0] + "  ", (sub(e, 2) + bodies[1]).lower(), "\x0b" + sub(e, 7) + bodies[2] + "\x1c\x1f",
             sub(e, 4, to=" ") + bodies[3], sub(e, 9, to="n") + bodies[4], e.lower() + bodies[5], " " + sub(e, 0) + "   ", "   "]
    return make(reads, BARCODES_MIXED, tags)


def tag_lengths_case(with_one, seed=51):
    """tags of 1 (with_one), 32, 33, 64, 65 and 128 bases behind rescued barcodes"""
    rnd = random.Random(seed)
    while True:
        stored = (["A"] if with_one else []) + ["CGT"[k % 3] + rand_seq(rnd, n - 1) for k, n in enumerate((32, 33, 64, 65, 128, 128))]
        try:
            rc.check_tags(stored)
            break
        except AssertionError:
            continue
    reads = []
    for t in stored:
        for b in BARCODES_MIXED[:3]:
            reads += [sub(b + "TGCAG", 2) + t + "G", sub(b + "TGCAG", 5) + t, sub(b + "TGCAG", 0) + t[:-1], sub(b + "TGCAG", 1) + sub(t, len(t) - 1)]
            reads.append(sub(b + "TGCAG", 3) + sub(t, len(t) // 2, to="N") + "AC")
    barcut, barnum, _, tagoff = orc.prepare_lists(BARCODES_MIXED, ["TGCAG" + t for t in stored], "TGCAG")
    return Case(fastq(reads), barcut, barnum, tagoff, stored)


def library(rnd, entries_by_row, bodies, n, p_exact=0.6):
    """reads: an entry of some row, exact or with 1..3 substitutions or an N, then a tag body with 0..1 substitutions"""
    reads = []
    for _ in range(n):
        e = rnd.choice(entries_by_row)
        roll = rnd.random()
        if roll >= p_exact:
            k = 1 if roll < p_exact + 0.25 else 2 if roll < p_exact + 0.35 else 3
            e = sub(e, *rnd.sample(range(len(e)), k))
            if rnd.random() < 0.1:
                e = sub(e, rnd.randrange(len(e)), to="N")
        t = rnd.choice(bodies)
        if rnd.random() < 0.1:
            t = sub(t, rnd.randrange(len(t)))
        reads.append(e + t + rand_seq(rnd, rnd.randrange(0, 12)))
    return reads


def wide_index_case(seed=52):
    """384 rows x 2 cut-site variants"""
    rnd = random.Random(seed)
    bars = set()
    while len(bars) < 384:
        bars.add(rand_seq(rnd, 8))
    bars = sorted(bars)
    rnd.shuffle(bars)
    bodies = free_tags(rnd, [34] * 8)
    tags = [rnd.choice(("CAGC", "CTGC")) + b for b in bodies]
    reads = library(rnd, [b + s for b in bars for s in ("CAGC", "CTGC")], bodies, 500)
    case = make(reads, bars, tags, "CWGC")
    assert len(entries_of(case.barcut, case.barnum)) == 768
    return case


def full_index_case(extra, seed=53):
    """the largest entry count that fits the module's LDS share, plus `extra`"""
    rnd = random.Random(seed)
    n = largest_index() + extra
    ents = set()
    while len(ents) < n:
        ents.add(rand_seq(rnd, 12))
    ents = sorted(ents)
    rnd.shuffle(ents)
    stored = free_tags(rnd, [30] * 3)
    reads = library(rnd, ents, stored, 60, p_exact=0.3)
    return Case(fastq(reads), ents, n, [12] * n, stored)


def few_entries_case(n, seed=54):
    rnd = random.Random(seed + n)
    ents = ["ACGTTGCAG", "TTGACATGCAG"][:n]
    stored = free_tags(rnd, [30] * 3)
    reads = library(rnd, ents, stored, 40, p_exact=0.3) + [rand_seq(rnd, 50)]
    return Case(fastq(reads), ents, n, [len(e) for e in ents], stored)


def offsets_case(stripped, seed=55):
    """tagoff = barcode + site length (one site, the tags carry it and are stripped) or = barcode length (a degenerate
    site, the tags keep it)"""
    rnd = random.Random(seed)
    bodies = free_tags(rnd, [rnd.randint(24, 60) for _ in range(12)])
    if stripped:
        case = make(library(rnd, [b + "TGCAG" for b in BARCODES_MIXED], bodies, 300), BARCODES_MIXED, ["TGCAG" + b for b in bodies])
        assert case.tagoff == [len(b) + 5 for b in BARCODES_MIXED]
    else:
        tags = [rnd.choice(("CAGC", "CTGC")) + b for b in bodies]
        case = make(library(rnd, [b + s for b in BARCODES_MIXED for s in ("CAGC", "CTGC")], bodies, 300), BARCODES_MIXED, tags, "CWGC")
        assert case.tagoff == [len(b) for b in BARCODES_MIXED]
    return case


# tile composition: records of "@\n" + read + "\n+\nI\n"
def short_records(reads):
    return b"".join(b"@\n" + r.encode() + b"\n+\nI\n" for r in reads)


def tile_case(kind, seed=56):
    """`kind`: 'exact' -- three tiles whose reads all begin with an entry; 'nohit' -- three tiles of short records none of
    which does, so that the no-hit list is full round after round; 63, 64, 65 -- one tile with that many no-hit reads
    among exact ones"""
    rnd = random.Random(seed)
    bodies, tags = some_tags(rnd, 4, 30)
    ents = [b + "TGCAG" for b in BARCODES_MIXED]
    if kind == "exact":
        reads = [rnd.choice(ents) + rnd.choice(bodies) + rand_seq(rnd, 40) for _ in range(500)]
    elif kind == "nohit":
        reads = [sub(rnd.choice(ents), rnd.randrange(9), *([rnd.randrange(9)] if rnd.random() < 0.3 else [])) for _ in range(2800)]
        reads = [r if rnd.random() < 0.9 else r + rnd.choice(bodies) for r in reads]
    else:
        reads = [rnd.choice(ents) + rnd.choice(bodies) for _ in range(150)]
        for k in rnd.sample(range(150), kind):
            e = rnd.choice(ents)
            reads[k] = sub(e, rnd.randrange(len(e))) + rnd.choice(bodies)
    data = short_records(reads)
    case = Case(data, *lists(BARCODES_MIXED, tags))
    entries = entries_of(case.barcut, case.barnum)
    nohit = sum(1 for r in reads if classify(r, entries, 1)[0] != "exact")
    if kind == "exact":
        assert nohit == 0 and len(data) > 2 * TILE
    elif kind == "nohit":
        assert nohit == len(reads) and len(data) > 2 * TILE
        assert data[:TILE].count(b"\n+\n") > 2 * 256                                      # three rounds of 256 reads in a tile, two of them full
    else:
        assert nohit == kind and len(data) < TILE
    return case


def seam_buffer(rnd, offset, read):
    """FASTQ bytes in which `read` (barcode ACGT, site TGCAG) starts `offset` bytes before the first tile's end"""
    data = rc.straddle_buffer(rnd, TILE - offset + 9, "ACGTTGCAG" + read[9:])
    start = TILE - offset
    assert data[start - 1:start] == b"\n" and data[start + len(read):start + len(read) + 1] == b"\n"
    return data[:start] + read.encode() + data[start + len(read):]


def big_case(seed=57):
    """seven tiles and more, CRLF"""
    rnd = random.Random(seed)
    bodies = free_tags(rnd, [rnd.randint(30, 110) for _ in range(40)])
    reads = library(rnd, [b + "TGCAG" for b in BARCODES_MIXED] + ["TTTTTTTTT"], bodies, 700)
    case = make(reads, BARCODES_MIXED, ["TGCAG" + b for b in bodies], nl="\r\n")
    assert len(case.data) > 6 * TILE
    return case


NAMED = {
    "geometry": geometry_case,
    "long_entries": long_entries_case,
    "near_and_far": lambda K: near_and_far_case(),
    "read_length": lambda K: read_length_case(),
    "two_rows_tie": lambda K: two_rows_tie_case(),
    "variants_tie": lambda K: variants_tie_case(),
    "degenerate_site": degenerate_site_case,
    "length_trap": lambda K: length_trap_case(),
    "shadow": lambda K: shadow_case(),
    "dirt": dirt_case,
    "tags_with_one_base": lambda K: tag_lengths_case(True),
    "tags_32_to_128": lambda K: tag_lengths_case(False),
    "one_entry": lambda K: few_entries_case(1),
    "two_entries": lambda K: few_entries_case(2),
    "offset_behind_site": lambda K: offsets_case(True),
    "offset_behind_barcode": lambda K: offsets_case(False),
}
