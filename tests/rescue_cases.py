"""Shared by tests/test_rescue.py and tests/test_rescue_gpu.py: the rescue rule restated by brute force -- every tag
against every read, Python strings, no parts -- with the oracle's tree for the barcode + cut site lookup and its line
splitting; the begin checks the slow and obvious way; builders of the inputs, each asserting the property it is named
for."""
import math
import random

from oracle import tagdigger_oracle as orc

ACGT = "ACGT"
MAXLEN = 128
CLASSES = ("reads", "barcut", "exact", "rescued1", "rescued2", "ambiguous", "none")
BARCODES_MIXED = ["ACGT", "TGACA", "GATTAC", "CCTAGGA", "TTGGCCAA", "AGAGTCTCA"]       # lengths 4..9, prefix-free
TILE = 16384


class Limit(Exception):
    """what TD_E_LIMIT stands for in the restatement"""


def check_tags(stored):
    """The begin checks of the stored tags: IndexError (no tag, an empty tag), Limit (longer than 128), AssertionError
    naming the later tag of the first pair -- by that later tag's position -- in which one tag equals or begins the other."""
    if not stored:
        raise IndexError("list index out of range")
    for t in stored:
        if not t:
            raise IndexError("list index out of range")
        if len(t) > MAXLEN:
            raise Limit("tag longer than 128 bases")
    for j in range(len(stored)):
        for i in range(j):
            if stored[i].startswith(stored[j]) or stored[j].startswith(stored[i]):
                raise AssertionError("Problematic sequence: {}.  Likely due to overlapping tags.".format(j))


def distance(w, t):
    return sum(1 for a, b in zip(w, t) if a != b)


def classify(w, stored, K):
    """(class, tag, mismatching positions) of the window w: every candidate's distance, the smallest decides"""
    cand = [(distance(w, t), k) for k, t in enumerate(stored) if len(t) <= len(w)]
    if any(d == 0 for d, _ in cand):
        hits = [k for d, k in cand if d == 0]
        assert len(hits) == 1
        return "exact", hits[0], ()
    if not cand:
        return "none", -1, ()
    m = min(d for d, _ in cand)
    if m > K:
        return "none", -1, ()
    hits = [k for d, k in cand if d == m]
    if len(hits) > 1:
        return "ambiguous", -1, ()
    t = stored[hits[0]]
    return "rescued%d" % m, hits[0], tuple(i for i in range(len(t)) if w[i] != t[i])


def ref_rescue_lists(data, barcut, barnum, tagoff, stored, K, maxreads=5e9, first_line=0):
    """(rescued, statistics, positions, exact) of FASTQ bytes whose first line has index first_line."""
    check_tags(stored)
    tree = orc.build_sequence_tree(barcut, barnum)
    bound = max(1, math.ceil(maxreads))             # (the reference tests readscount >= maxreads after a read)
    rescued = [[0] * len(stored) for _ in range(barnum)]
    exact = [[0] * len(stored) for _ in range(barnum)]
    positions = [0] * MAXLEN
    st = dict.fromkeys(CLASSES, 0)
    memo = {}
    for k, raw in enumerate(orc.iter_lines(data), first_line):
        if k % 4 != 1:
            continue
        if k > 4 * (bound - 1) + 1:
            break
        st["reads"] += 1
        line1 = orc.clean_read(raw)
        b = orc.sequence_index_lookup(line1, tree)
        if b == -1:
            continue
        st["barcut"] += 1
        w = line1[tagoff[b]:]
        if w not in memo:
            memo[w] = classify(w, stored, K)
        kind, t, where = memo[w]
        st[kind] += 1
        if kind == "exact":
            exact[b][t] += 1
        elif t >= 0:
            rescued[b][t] += 1
            for i in where:
                positions[i] += 1
    assert st["barcut"] == st["exact"] + st["rescued1"] + st["rescued2"] + st["ambiguous"] + st["none"]
    return rescued, st, positions, exact


def ref_rescue(data, barcodes, tags, cutsite="TGCAG", K=1, maxreads=5e9):
    barcut, barnum, stored, tagoff = orc.prepare_lists(barcodes, tags, cutsite)
    return ref_rescue_lists(data, barcut, barnum, tagoff, stored, K, maxreads)


def golden_plan(case, directory):
    """What a recorded hot-path payload asks of the rescue -> (what, value, path to call with):
    'skip' (weights; stored tags beyond 128 bases or not prefix-free), 'raises' with the exception the set-up or the
    missing file raises, or 'run' with the FASTQ bytes."""
    import os
    from conftest import write_case_file
    kw = case["kwargs"]
    write_case_file(case, directory)
    path = os.path.join(str(directory), case.get("filename_override") or case["filename"])
    if kw.get("tassel_tagcount"):
        return "skip", None, path
    try:
        barcut, barnum, stored, _ = orc.prepare_lists(case["barcodes"], case["tags"], kw.get("cutsite", "TGCAG"))
    except AssertionError as exc:
        return "raises", exc, path
    try:
        check_tags(stored)
    except (AssertionError, Limit):
        return "skip", None, path
    except IndexError as exc:
        return "raises", exc, path
    try:
        orc.build_sequence_tree(barcut, barnum)
    except (AssertionError, IndexError) as exc:
        return "raises", exc, path
    if not os.path.exists(path):
        return "raises", FileNotFoundError(), path
    return "run", orc.read_fastq_bytes(path), path


def part_bases(stored, K):
    return min(32, min(len(t) for t in stored) // (K + 1))


def longest_run(stored, K):
    """tags that share one of the K + 1 parts, at most; None when the shortest tag leaves no part"""
    P = part_bases(stored, K)
    if P < 1:
        return None
    best = 0
    for p in range(K + 1):
        keys = [t[p * P:(p + 1) * P] for t in stored]
        best = max(best, max(keys.count(k) for k in set(keys)))
    return best


# ------------------------------------------------------------------------------------------------------------ inputs
def rand_seq(rnd, n):
    return "".join(rnd.choice(ACGT) for _ in range(n))


def other(base, step=1):
    return ACGT[(ACGT.index(base) + step) % 4]


def sub(s, *where, to=None):
    """s with another base (or `to`) at every position of `where`"""
    s = list(s)
    for i in where:
        s[i] = to if to is not None else other(s[i])
    return "".join(s)


def fastq(reads, nl="\n", quality=True, last_nl=True):
    out = []
    for i, r in enumerate(reads):
        out.append("@r%d%s%s%s+%s%s%s" % (i, nl, r, nl, nl, "I" * len(r) if quality else "I", nl))
    text = "".join(out)
    if not last_nl:
        text = text[:-len(nl)]
    return text.encode("latin-1")


def free_tags(rnd, lengths):
    """random tags of these lengths, none equal to or beginning another"""
    while True:
        tags = [rand_seq(rnd, n) for n in lengths]
        try:
            check_tags(tags)
            return tags
        except AssertionError:
            continue


def seam_positions(n, K):
    """the first and the last base, both sides of every part seam and of every 32-base word seam"""
    P = min(32, n // (K + 1))
    pos = {0, n - 1}
    for p in range(1, K + 2):
        pos |= {p * P - 1, p * P}
    for s in (32, 64, 96):
        pos |= {s - 1, s}
    return sorted(i for i in pos if 0 <= i < n), P


def length_case(n, K, seed=0):
    """Tags of n bases (one of them the target) and reads behind ACGT + TGCAG that carry the target with one mismatch at
    every seam position and with two mismatches in one part, in two parts and behind the parts.  Returns (reads, tags)."""
    rnd = random.Random(1000 * n + K + seed)
    ntags = min(12, 4 ** n // 2) if n < 3 else 12
    if n < 3:
        alls = [a + b for a in ACGT for b in (ACGT if n == 2 else [""])]
        tags = rnd.sample(alls, max(2, ntags))
    else:
        tags = free_tags(rnd, [n] * ntags)
    target = tags[0]
    pos, P = seam_positions(n, K)
    windows = [target] + [sub(target, i) for i in pos]
    pairs = []
    if n >= 2:
        pairs.append((0, n - 1))
        if P >= 2:
            pairs.append((0, P - 1))                       # one part
        if P >= 1 and P < n:
            pairs.append((0, P))                           # two parts
        if n - 2 >= (K + 1) * P:
            pairs.append((n - 2, n - 1))                   # behind every part
        if 2 * P < n:
            pairs.append((P, 2 * P))
    windows += [sub(target, i, j) for i, j in pairs if i != j]
    tails = [rand_seq(rnd, 20), ""]                        # the line goes on, or ends exactly at the tag's end
    reads = ["ACGTTGCAG" + w + tails[k % 2] for k, w in enumerate(windows)]
    reads += ["ACGTTGCAG" + rand_seq(rnd, n + 5) for _ in range(6)]
    # the property: every single substitution lies at distance 1 from the target, every pair at 2
    for i in pos:
        assert distance(sub(target, i), target) == 1
    for i, j in pairs:
        assert i == j or distance(sub(target, i, j), target) == 2
    return reads, ["TGCAG" + t for t in tags]


def mixed_case(K, seed=3):
    """one index with tags of many lengths; reads one and two mismatches from each"""
    rnd = random.Random(seed)
    lengths = [20, 21, 33, 40, 64, 65, 100, 127, 128] * 2
    tags = free_tags(rnd, lengths)
    reads = []
    for t in tags:
        n = len(t)
        for w in (t, sub(t, 0), sub(t, n - 1), sub(t, n // 2), sub(t, 1, n - 2), sub(t, n // 3, to="N")):
            reads.append(rnd.choice(BARCODES_MIXED) + "TGCAG" + w + rand_seq(rnd, rnd.randrange(0, 30)))
    rnd.shuffle(reads)
    assert len({len(t) for t in tags}) == 9
    return reads, ["TGCAG" + t for t in tags]


def tie_case_equal(n=40, seed=5):
    """two tags of equal length one substitution apart: a read equal to neither at that position lies at 1 from both"""
    rnd = random.Random(seed)
    a = rand_seq(rnd, n)
    b = sub(a, n // 2)
    w = a[:n // 2] + other(a[n // 2], 2) + a[n // 2 + 1:]
    assert w != a and w != b and distance(w, a) == distance(w, b) == 1
    return ["ACGTTGCAG" + w + "ACGT", "ACGTTGCAG" + sub(a, 3) + "AC"], ["TGCAG" + a, "TGCAG" + b, "TGCAG" + rand_seq(rnd, n)]


def tie_case_lengths(seed=6):
    """a shorter and a longer tag that differ inside the shorter one's length; a read at distance 1 from both"""
    rnd = random.Random(seed)
    long_ = rand_seq(rnd, 50)
    short = sub(long_[:30], 10)
    w = sub(long_, 10, to=other(long_[10], 2))
    assert w[10] not in (long_[10], short[10]) and distance(w, long_) == 1 and distance(w[:30], short) == 1
    return ["ACGTTGCAG" + w, "ACGTTGCAG" + w[:40]], ["TGCAG" + short, "TGCAG" + long_]


def two_parts_case(K, n=64, seed=7):
    """a read one mismatch from its tag with K of the K + 1 parts intact: the tag is reached K times and counted once"""
    rnd = random.Random(seed)
    tags = free_tags(rnd, [n] * 5)
    P = min(32, n // (K + 1))
    w = sub(tags[0], n - 1) if (K + 1) * P < n else sub(tags[0], P // 2)
    intact = sum(1 for p in range(K + 1) if w[p * P:(p + 1) * P] == tags[0][p * P:(p + 1) * P])
    assert intact >= 2 or K == 1 and intact >= 1
    return ["ACGTTGCAG" + w + "A"] * 3, ["TGCAG" + t for t in tags]


def second_part_tie_case(seed=8):
    """K = 1, two parts of 20: the read's first part is tag a's, its second part tag b's, and it lies at 1 from both --
    the second tag comes through the other part"""
    rnd = random.Random(seed)
    a = rand_seq(rnd, 40)
    b = sub(a, 5, 30)                      # differs from a in both parts
    w = sub(a, 30, to=b[30])               # part 0 as a's, part 1 as b's
    assert w[:20] == a[:20] and w[:20] != b[:20] and w[20:] == b[20:] and w[20:] != a[20:]
    assert distance(w, a) == 1 and distance(w, b) == 1
    return ["ACGTTGCAG" + w + "ACGT"] * 2, ["TGCAG" + a, "TGCAG" + b]


def last_part_case(K, seed=9):
    """reads whose only intact part is the last one"""
    rnd = random.Random(seed)
    n = 30 * (K + 1)
    tags = free_tags(rnd, [n] * 6)
    w = sub(tags[2], *[p * 30 + 7 for p in range(K)])
    P = 30
    assert [w[p * P:(p + 1) * P] == tags[2][p * P:(p + 1) * P] for p in range(K + 1)] == [False] * K + [True]
    return ["ACGTTGCAG" + w + "TT"] * 2, ["TGCAG" + t for t in tags]


def n_case(K, seed=10):
    """one N inside each part in turn, an N as the only mismatch, two Ns; dirt: lower case, leading blanks"""
    rnd = random.Random(seed)
    n = 20 * (K + 1) + 6
    tags = free_tags(rnd, [n] * 6)
    t = tags[1]
    windows = [sub(t, p * 20 + 9, to="N") for p in range(K + 1)]
    windows += [sub(t, n - 1, to="N"), sub(t, 3, 50 if n > 50 else 25, to="N"), sub(sub(t, 2), 30, to="N"), sub(t, 0, to="n")]
    for p in range(K + 1):
        assert "N" in windows[p][p * 20:(p + 1) * 20] and distance(windows[p], t) == 1
    reads = ["ACGTTGCAG" + w + "GG" for w in windows]
    reads += [("ACGTTGCAG" + sub(t, 11) + "CC").lower(), "  \t ACGTTGCAG" + sub(t, 12) + "  ", "\x0bACGTTGCAG" + t + "\x1c\x1f"]
    return reads, ["TGCAG" + x for x in tags]


def line_end_case(seed=11):
    """the line ends exactly at the tag's end, one base short of it, inside the barcode, and right behind the cut site"""
    rnd = random.Random(seed)
    tags = free_tags(rnd, [30] * 4 + [12])
    t = tags[0]
    reads = ["ACGTTGCAG" + sub(t, 4), "ACGTTGCAG" + sub(t, 4)[:29], "ACG", "ACGTTGCAG", "ACGTTGCAG" + sub(t, 4) + "   ",
             "ACGTTGCAG" + sub(t, 29)[:29] + " ", "ACGTTGCAG" + sub(tags[4], 11), "ACGTTGCAG" + tags[4][:11] + " \t"]
    assert len(reads[1]) == 9 + 29 and reads[3][9:] == ""
    return reads, ["TGCAG" + x for x in tags]


def shadow_case(seed=12):
    """an exact tag beside a tag at distance 1: the read is the counter's"""
    rnd = random.Random(seed)
    a = rand_seq(rnd, 36)
    b = sub(a, 20)
    assert distance(a, b) == 1
    return ["ACGTTGCAG" + a + "AC", "ACGTTGCAG" + b, "ACGTTGCAG" + sub(a, 1) + "T"], ["TGCAG" + a, "TGCAG" + b]


def run_case(nrun, K=1, seed=13):
    """nrun tags share their first part (20 bases) and differ behind it; reads one mismatch from some of them, the
    mismatch in the second part, so that the whole run is walked"""
    rnd = random.Random(seed + nrun)
    head = rand_seq(rnd, 20)
    tails = set()
    while len(tails) < nrun:
        tails.add(rand_seq(rnd, 20 * K))                  # 20 (K + 1) bases: parts of 20
    tags = [head + t for t in sorted(tails)]
    rnd.shuffle(tags)
    tags += free_tags(rnd, [len(tags[0])] * 3)
    reads = []
    for k in range(0, nrun, max(1, nrun // 7)):
        reads += ["ACGTTGCAG" + sub(tags[k], 25) + "A", "ACGTTGCAG" + tags[k], "ACGTTGCAG" + sub(tags[k], 22, 39 + 20 * (K - 1))]
    assert longest_run(tags, K) == nrun
    return reads, ["TGCAG" + t for t in tags]


def straddle_buffer(rnd, window_at, read, nfill=100):
    """FASTQ bytes in which `read` (barcode ACGT, site TGCAG) has its window start at byte `window_at`"""
    line_at = window_at - 9
    filler = fastq(["TTTT" + rand_seq(rnd, 120) for _ in range(nfill)], quality=False)
    pad = line_at - 3 - len(filler) - 8                     # one more record: "@f\n" + A * pad + "\n+\nI\n"
    assert pad >= 0
    data = filler + b"@f\n" + b"A" * pad + b"\n+\nI\n" + b"@r\n" + read.encode() + b"\n+\nI\n" + fastq(["ACGTTGCAGAC"], quality=False)
    assert data[window_at - 9:window_at] == b"ACGTTGCAG" and data[window_at - 10:window_at - 9] == b"\n"
    return data
