"""Inputs that reach the structural edges of the tag hash table (td_set_index in csrc/tagdig.hip, the probe
match_stream / match_finish in csrc/kernels.hpp): chains of displaced keys, the ring wrap, every packed width, the
hashed prefix below 32 bases and the short list, the staging budget at its extreme, every piece count of k_fast2 /
k_fast4.

Plain Python; the product is not imported here.  tests/test_index_edges.py holds every case on the CPU against three
references that share nothing -- the C oracle's trie, the Python oracle's trie, and brute_counts below (str.startswith)
-- and tests/test_index_edges_gpu.py holds the kernels against the C oracle on identical bytes.

What the table stores.  With the single cut site TGCAG and tags that all begin with it, find_tags_fastq strips the
site from the tags (the barcode entry has checked it): the table holds the bases BEHIND the site.  Every length, stem
and width below is stated for that stored tag; the tags handed to the engine and the oracles are CUT + stored.

    W      64-bit words of a packed tag: the smallest of 1, 2, 3, 4, 6, 10 with 32 W >= the longest stored tag
    spb    slots per bucket: 5, 3, 2, 3, 2, 1
    m      hashed leading bases: 32, or the 17th shortest stored length where there are more than 16 tags and that is
           less; stored tags shorter than m lie on the linear short list
Stored tags that share their first m bases share a home bucket: more than spb of them make a chain.
"""
import bisect
import collections
import functools
import random

import weighted_cases as wc
from oracle import c_oracle
from oracle import tagdigger_oracle as orc

CUT = "TGCAG"
WIDTHS = (1, 2, 3, 4, 6, 10)
SPB = {1: 5, 2: 3, 3: 2, 4: 3, 6: 2, 10: 1}
MAX_SHORT = 16
NQ = {1: (3, 4, 6), 2: (5, 6, 8), 3: (7, 8, 10)}
SEAM = 96 * 1024            # a multiple of every tile the kernels use (16, 24, 32 KiB): a tile boundary for all of them;
                            # the GPU test asserts, mode by mode, that the mode's tile divides it

# reads: (kind, sequence).  "hit" must count a tag, MISS_KINDS must count the barcode only, the rest is whatever the
# references say.  extra_off: bases between barcode + site and the tag that nothing looks at (the C-ABI's tagoff may lie
# behind the barcode entry; the Python front-end never asks for it, and only that reaches the largest piece counts).
# expect: what td_index_info must report for the case to have reached its regime ("min_*": at least).
Case = collections.namedtuple("Case", "name barcodes tags cutsite reads data load extra_off expect")
MISS_KINDS = ("last", "short", "stem")


# ---------------------------------------------------------------------------------------------------- table shape
def width_of(maxlen, off=0):
    """The narrowest width that holds the longest stored tag and stages it: 16 (2 W + 3) bytes from the 16-byte chunk the
    read starts in must reach the tag's last base, off + maxlen bases behind a read that starts at the chunk's byte 15.
    (off: barcode + site + extra_off, at most 32 without extra_off -- then the first condition implies the second.)"""
    return next(w for w in WIDTHS if 32 * w >= maxlen and 16 * (2 * w + 3) >= 15 + off + maxlen)


def stored_tags(case):
    assert all(t.startswith(CUT) for t in case.tags)
    return [t[len(CUT):] for t in case.tags]


def expected_shape(stored, off=0):
    """td_set_index's rules restated: {W, spb, m_bases, nshort}."""
    lens = sorted(len(t) for t in stored)
    m = 32
    if len(lens) > MAX_SHORT:
        m = min(32, lens[MAX_SHORT])
    W = width_of(lens[-1], off)
    return {"W": W, "spb": SPB[W], "m_bases": m, "nshort": sum(1 for x in lens if x < m)}


def is_prefix_free(seqs):
    s = sorted(seqs)
    return all(not b.startswith(a) for a, b in zip(s, s[1:]))


# ---------------------------------------------------------------------------------------------------- references
class Brute:
    """The rule by str.startswith.  Among prefix-free tags the only one that can be a prefix of r is r's predecessor in
    sorted order (a tag between a prefix of r and r would itself start with that prefix)."""

    def __init__(self, case):
        self.barcut = [b + case.cutsite for b in case.barcodes]
        stored = stored_tags(case)
        self.order = sorted(range(len(stored)), key=lambda i: stored[i])
        self.sorted = [stored[i] for i in self.order]
        self.extra = case.extra_off

    def find_tag(self, rest):
        k = bisect.bisect_right(self.sorted, rest) - 1
        if k >= 0 and rest.startswith(self.sorted[k]):
            return self.order[k]
        return -1

    def lookup(self, read):
        """(barcode or -1, tag or -1) of one sequence line."""
        for bi, bc in enumerate(self.barcut):
            if read.startswith(bc):
                return bi, self.find_tag(read[len(bc) + self.extra:])
        return -1, -1


def brute_counts(case, weighted=False):
    """(matrix as lists of ints, {"reads", "barcut", "tag"})."""
    br = Brute(case)
    m = [[0] * len(case.tags) for _ in case.barcodes]
    st = {"reads": 0, "barcut": 0, "tag": 0}
    weight = 1
    for i, raw in enumerate(case.data.splitlines()):
        if i & 3 == 0 and weighted:
            text = raw.decode("latin-1")
            weight = int(text[text.find("count=") + 6:].strip())
        if i & 3 != 1:
            continue
        st["reads"] += 1
        b, t = br.lookup(raw.decode("latin-1").strip().upper())
        if b >= 0:
            st["barcut"] += 1
            if t >= 0:
                st["tag"] += 1
                m[b][t] += weight
    return m, st


def COracle(case):
    """The C oracle with the tag search `extra_off` bases further into the read."""
    return c_oracle.COracle(case.barcodes, case.tags, case.cutsite, extra_off=case.extra_off)


def c_reference(case, weighted=False):
    st = {}
    m = COracle(case).count_bytes(case.data, tassel_tagcount=weighted, stats=st)
    return m.astype("int64").tolist(), {k: st[k] for k in ("reads", "barcut", "tag")}


def py_reference(case, weighted=False):
    barcuttree, tagtree, barcutlen, barnum, ntags = orc.prepare_index(case.barcodes, case.tags, case.cutsite)
    index = (barcuttree, tagtree, [x + case.extra_off for x in barcutlen], barnum, ntags)
    st = {}
    m = orc.count_bytes(case.data, case.barcodes, case.tags, case.cutsite, tassel_tagcount=weighted, stats=st, index=index)
    return m, st


# ---------------------------------------------------------------------------------------------------- generators
def bases(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def make_barcodes(rnd, n, length):
    """n barcodes of `length` bases (an int or a (lo, hi) range), prefix-free together with the site."""
    out = []
    while len(out) < n:
        b = bases(rnd, length if isinstance(length, int) else rnd.randint(*length))
        if is_prefix_free([x + CUT for x in out + [b]]):
            out.append(b)
    return out


def distinct_tails(rnd, n, length):
    """n different sequences of `length` bases (an int or a (lo, hi) range), none a prefix of another."""
    if isinstance(length, int):
        assert 4 ** length >= n
    while True:
        out, seen = [], set()
        while len(out) < n:
            t = bases(rnd, length if isinstance(length, int) else rnd.randint(*length))
            if t not in seen:
                seen.add(t)
                out.append(t)
        if is_prefix_free(out):                     # (mixed lengths: else again from the generator's next state)
            return out


def random_tags(rnd, n, length):
    """n prefix-free stored tags of `length` bases (an int or a (lo, hi) range)."""
    return distinct_tails(rnd, n, length)


def make_reads(rnd, barcodes, stored, extra_off=0, sample=None, stem_len=32, nrandom=2000, random_len=(33, 70)):
    """The reads of a case: for each sampled tag a hit (barcode + site + tag + 0-4 further bases) and the three near
    misses -- last base changed, one base short, the tag's first stem_len bases with a foreign tail of the tag's length
    (it hashes to the tag's home bucket and must walk the whole chain) --, then nrandom reads with a barcode and no
    tag on purpose, and a few without a barcode.  A near miss that happens to hit another tag is not made."""
    probe = Brute(Case("", barcodes, [CUT + t for t in stored], CUT, None, None, 25, extra_off, None))
    idx = list(range(len(stored)))
    if sample is not None and sample < len(idx):
        idx = sorted(rnd.sample(idx, sample))
    reads = []

    def full(rest):
        return rnd.choice(barcodes) + CUT + bases(rnd, extra_off) + rest

    def add_miss(kind, rest):
        if probe.find_tag(rest) < 0:
            reads.append((kind, full(rest)))
    for i in idx:
        t = stored[i]
        reads.append(("hit", full(t + bases(rnd, rnd.randint(0, 4)))))
        add_miss("last", t[:-1] + rnd.choice([c for c in "ACGT" if c != t[-1]]) + bases(rnd, rnd.randint(0, 4)))
        add_miss("short", t[:-1])
        if len(t) > stem_len:
            add_miss("stem", t[:stem_len] + bases(rnd, len(t) - stem_len + rnd.randint(0, 4)))
    for _ in range(nrandom):
        reads.append(("random", full(bases(rnd, rnd.randint(*random_len)))))
    for _ in range(20):
        s = bases(rnd, rnd.randint(0, 60))
        if probe.lookup(s)[0] < 0:
            reads.append(("nobar", s))
    rnd.shuffle(reads)
    return reads


def fastq(rnd, reads, nl="\n"):
    """Four-line records; every header carries a count= field in weighted_cases' grammar, the quality line is short."""
    out = []
    for k, (_, seq) in enumerate(reads):
        out.append("@r%d count=%s%s%s%s+%s%s%s" % (k, wc.weight_text(rnd), nl, seq, nl, nl, "I" * (1 + k % 5), nl))
    return "".join(out).encode("latin-1")


def make_case(name, rnd, barcodes, stored, expect, load=25, extra_off=0, **read_args):
    assert is_prefix_free(stored) and len(set(stored)) == len(stored), name
    reads = make_reads(rnd, barcodes, stored, extra_off=extra_off, **read_args)
    shape = expected_shape(stored, max(len(b) for b in barcodes) + len(CUT) + extra_off)
    shape.update(expect)
    return Case(name, barcodes, [CUT + t for t in stored], CUT, reads, fastq(rnd, reads), load, extra_off, shape)


def w1_family(rnd, n):
    """A chain at W = 1, where a tag has no room behind a 32-base stem: 16 stored tags of 19 bases (the short list) and
    one of 20 make m = 20, and n tags of 32 bases share their first 20."""
    while True:
        shorts = random_tags(rnd, MAX_SHORT, 19)
        stem = bases(rnd, 20)
        stored = shorts + [bases(rnd, 20)] + [stem + t for t in distinct_tails(rnd, n, 12)]
        if is_prefix_free(stored):
            return stored


# ---------------------------------------------------------------------------------------------------- families
FAMILY_L = (32, 33, 64, 65, 96, 97, 128, 129, 192, 193, 320)
FAMILY_N = 45


def family_size(L):
    """Tags of L bases that can share a 32-base stem: 45, but one at L = 32 and four at L = 33."""
    return min(FAMILY_N, 4 ** (L - 32))


def chain_depth(n, spb):
    """n keys of one home bucket: the farthest lies at least this many buckets on."""
    return -(-n // spb) - 1


@functools.lru_cache(maxsize=None)
def family_case(L):
    """Stems of 32 bases with family_size(L) tags of L bases each, 45 tags or a few more in all (L = 32 is the degenerate
    family of one: 45 stems and no promise of a chain).  L = "w1": the chain at W = 1 (w1_family).  L = ("mixed", W):
    one stem, 45 tags of lengths between the next narrower width's 32 W' + 1 (at least 35) and 32 W."""
    rnd = random.Random("family %r" % (L,))
    barcodes = make_barcodes(rnd, 4, (4, 9))
    if L == "w1":
        stored = w1_family(rnd, FAMILY_N)
        expect = {"W": 1, "m_bases": 20, "nshort": 16, "min_displaced": 1, "min_longest": chain_depth(FAMILY_N, SPB[1])}
        return make_case("family W=1, m=20", rnd, barcodes, stored, expect, stem_len=20)
    if isinstance(L, tuple):
        W = L[1]
        lo = 32 * WIDTHS[WIDTHS.index(W) - 1] + 1
        stem = bases(rnd, 32)
        tails = distinct_tails(rnd, FAMILY_N - 1, (max(lo - 32, 3), 32 * W - 32))
        stored = [stem + t for t in tails] + [stem + _foreign_tail(rnd, tails, 32 * W - 32)]
        expect = {"W": W, "min_displaced": 1, "min_longest": chain_depth(FAMILY_N, SPB[W])}
        return make_case("family mixed lengths W=%d" % W, rnd, barcodes, stored, expect)
    n = family_size(L)
    stems = distinct_tails(rnd, -(-FAMILY_N // n), 32)
    stored = [s + t for s in stems for t in (distinct_tails(rnd, n, L - 32) if L > 32 else [""])]
    W = width_of(L)
    expect = {"W": W, "min_longest": chain_depth(n, SPB[W])}
    if n > SPB[W]:
        expect["min_displaced"] = 1
    return make_case("family L=%d" % L, rnd, barcodes, stored, expect)


def _foreign_tail(rnd, tails, length):
    """One more tail, of exactly `length` bases (the family's longest: it fixes W), prefix-free with the others."""
    while True:
        t = bases(rnd, length)
        if is_prefix_free(tails + [t]):
            return t


FAMILY_KEYS = FAMILY_L + ("w1",) + tuple(("mixed", W) for W in WIDTHS[1:])


# ---------------------------------------------------------------------------------------------------- dense ring
RING_STEMS = 4


def ring_family_size(W):
    return int(16 * SPB[W] * 0.95)


@functools.lru_cache(maxsize=None)
def ring_case(W, k):
    """table_load_pct = 95 and one family of floor(16 spb 0.95) tags: 16 buckets, and the chain covers nearly the whole
    ring.  Stem number k of RING_STEMS; even k: tags of exactly 32 W bases, odd k: mixed lengths.  (W = 1: w1_family with two
    tags less -- its 20-base tag takes a slot too, and 76 of 76.0 would leave the 16 buckets to the rounding of 16 * 5 * 0.95.)"""
    rnd = random.Random("ring %d %d" % (W, k))
    barcodes = make_barcodes(rnd, 3, (4, 9))
    n = ring_family_size(W)
    if W == 1:
        n -= 2
        stored = w1_family(rnd, n)
        expect = {"W": 1, "m_bases": 20, "nshort": 16}
        stem_len = 20
    else:
        stem = bases(rnd, 32)
        lo = 32 * WIDTHS[WIDTHS.index(W) - 1] + 1
        if k % 2 == 0:
            tails = distinct_tails(rnd, n, 32 * W - 32)
        else:
            tails = distinct_tails(rnd, n - 1, (max(lo - 32, 3), 32 * W - 32))
            tails.append(_foreign_tail(rnd, tails, 32 * W - 32))
        stored = [stem + t for t in tails]
        expect = {"W": W}
        stem_len = 32
    expect.update({"buckets": 16, "min_displaced": n - SPB[W], "min_longest": chain_depth(n, SPB[W])})
    return make_case("ring W=%d stem %d" % (W, k), rnd, barcodes, stored, expect, load=95, stem_len=stem_len)


DENSE_BUCKETS = {1: 512, 2: 512, 3: 1024, 4: 512, 6: 1024, 10: 2048}


@functools.lru_cache(maxsize=None)
def dense_random_case(W):
    """About 2 000 random tags at 95 % load -- one less than 95 % of the slots of a power of two of buckets, the table's
    size: many interleaved chains, filter bits of foreign keys in every full bucket."""
    rnd = random.Random("dense %d" % W)
    barcodes = make_barcodes(rnd, 3, (4, 9))
    n = int(DENSE_BUCKETS[W] * SPB[W] * 0.95) - 1
    lo = 32 if W == 1 else 32 * WIDTHS[WIDTHS.index(W) - 1] + 1
    while True:
        stored = random_tags(rnd, n - 1, (lo, 32 * W)) + [bases(rnd, 32 * W)]
        if is_prefix_free(stored):
            break
    expect = {"W": W, "m_bases": 32, "nshort": 0, "buckets": DENSE_BUCKETS[W], "min_displaced": n // 10, "min_longest": 3}
    return make_case("2000 random tags at 95 %% load, W=%d" % W, rnd, barcodes, stored, expect, load=95, sample=300)


# ---------------------------------------------------------------------------------------------------- multi-allelic markers
@functools.lru_cache(maxsize=None)
def allelic_case(L, nmarkers=3000):
    """Markers of 4-6 alleles of L bases that differ at two sites behind base 32: every marker's alleles share a home
    bucket and do not fit it (spb = 3 at 64 bases, 2 at 96).  Default load."""
    rnd = random.Random("alleles %d" % L)
    barcodes = make_barcodes(rnd, 6, (4, 9))
    stored, seen, most = [], set(), 0
    while len(stored) < 1 or len(seen) < nmarkers:
        base = bases(rnd, L)
        if base[:32] in seen:
            continue
        seen.add(base[:32])
        p, q = sorted(rnd.sample(range(32, L), 2))
        k = rnd.randint(4, 6)
        most = max(most, k)
        for x, y in rnd.sample([(x, y) for x in "ACGT" for y in "ACGT"], k):
            stored.append(base[:p] + x + base[p + 1:q] + y + base[q + 1:])
    W = width_of(L)
    expect = {"W": W, "m_bases": 32, "nshort": 0, "min_displaced": nmarkers * (4 - SPB[W]), "min_longest": chain_depth(most, SPB[W])}
    return make_case("%d markers of 4-6 alleles, %d bases" % (nmarkers, L), rnd, barcodes, stored, expect, sample=600, nrandom=1000)


# ---------------------------------------------------------------------------------------------------- m_bases, short list
SHORT_COUNTS = (15, 16, 17, 40, "all")


@functools.lru_cache(maxsize=None)
def short_case(nshort):
    """`nshort` stored tags below 32 bases beside 30 of 40-64 bases ("all": 40 short ones and no other).  Reads: the
    usual ones, and for every tag and some random sequences a read cut to exactly m - 1, m and m + 1 bases behind the
    offset -- below m only the short list may answer, from m on the probe runs."""
    rnd = random.Random("short %r" % (nshort,))
    barcodes = make_barcodes(rnd, 3, (4, 9))
    while True:
        k = 40 if nshort == "all" else nshort
        stored = [bases(rnd, rnd.randint(6, 31)) for _ in range(k)]
        if nshort != "all":
            stored += [bases(rnd, rnd.randint(40, 64)) for _ in range(30)]
        if is_prefix_free(stored) and len(set(stored)) == len(stored):
            break
    shape = expected_shape(stored)
    m = shape["m_bases"]
    reads = make_reads(rnd, barcodes, stored, stem_len=m, nrandom=500, random_len=(1, 70))
    for t in stored + [bases(rnd, 40) for _ in range(40)]:
        for n in (m - 1, m, m + 1):
            reads.append(("edge", rnd.choice(barcodes) + CUT + (t + bases(rnd, 40))[:n]))
    rnd.shuffle(reads)
    return Case("%s tags below 32 bases" % (nshort,), barcodes, [CUT + t for t in stored], CUT, reads, fastq(rnd, reads), 25, 0, shape)


# ---------------------------------------------------------------------------------------------------- piece counts
# (W, pieces) -> (barcode bases, longest stored tag, extra_off): barcode + site + extra_off + tag = the bases the matcher
# may look at, 16 to a piece, rounded up to the next instantiated count
# (the largest count of a width is reached at one total only, 65 / 97 / 129 bases, and only with extra_off: one base more
# and the k_count / k_fast staging of that width would end before the tag does, so the table takes the next width)
NQ_SHAPES = {(1, 3): (5, 30, 0), (1, 4): (27, 32, 0), (1, 6): (27, 25, 8),
             (2, 5): (5, 64, 0), (2, 6): (27, 64, 0), (2, 8): (27, 57, 8),
             (3, 7): (5, 96, 0), (3, 8): (27, 96, 0), (3, 10): (27, 89, 8)}


@functools.lru_cache(maxsize=None)
def nq_case(W, nq):
    blen, maxlen, extra = NQ_SHAPES[(W, nq)]
    rnd = random.Random("nq %d %d" % (W, nq))
    barcodes = make_barcodes(rnd, 3, blen)
    need = -(-(blen + len(CUT) + extra + maxlen) // 16)
    assert min(x for x in NQ[W] if x >= need) == nq
    lo = max(20, 32 * (W - 1) + 1)
    stored = random_tags(rnd, 39, (lo, maxlen)) + [bases(rnd, maxlen)]
    while not is_prefix_free(stored):
        stored[-1] = bases(rnd, maxlen)
    return make_case("W=%d, %d pieces" % (W, nq), rnd, barcodes, stored, {"W": W, "nch2": nq}, extra_off=extra, nrandom=500,
                     random_len=(20, maxlen + 8))


@functools.lru_cache(maxsize=None)
def wide_offset_case(maxlen):
    """The tag search starts 8 bases behind a barcode + site of 32, and the longest stored tag fills its width (32, 64, ...
    bases): a read that starts at byte 15 of a chunk needs 15 + 40 + maxlen staged bytes, more than the 16 (2 W + 3) of
    the tag's own width -- the table must take the next width (found by this module: td_set_index chose W from the tag
    length alone, and k_count / k_fast did not see such a tag's last bases)."""
    rnd = random.Random("wide offset %d" % maxlen)
    barcodes = make_barcodes(rnd, 3, 27)
    stored = random_tags(rnd, 20, maxlen)
    W = width_of(maxlen, 40)
    assert W > width_of(maxlen)
    return make_case("offset 40, tags of %d bases" % maxlen, rnd, barcodes, stored, {"W": W}, extra_off=8, nrandom=300,
                     random_len=(20, maxlen + 8))


WIDE_OFFSET_LENS = (32, 64, 96, 128, 192)


# ---------------------------------------------------------------------------------------------------- exact lengths, staging
@functools.lru_cache(maxsize=None)
def staging_index(W):
    """Barcode + site of exactly 32 bases (27 + TGCAG), stored tags of exactly 32 W: 15 + 32 + 32 W staged bytes when the
    read starts at byte 15 of a chunk, one less than the 16 (2 W + 3) there are.  Two tags differ in their last base
    only, two in the first base of their last word, two in base 32 of 32 W: (barcodes, tags, a stored sequence that
    misses by its last base)."""
    rnd = random.Random("staging %d" % W)
    barcodes = make_barcodes(rnd, 3, 27)
    L = 32 * W
    a, b, c = bases(rnd, L), bases(rnd, L), bases(rnd, L)
    flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
    stored = [a[:-1] + "A", a[:-1] + "C", b, b[:L - 32] + flip[b[L - 32]] + b[L - 31:], c, c[:31] + flip[c[31]] + c[32:]]
    stored = list(dict.fromkeys(stored))
    assert is_prefix_free(stored)
    return barcodes, [CUT + t for t in stored], a[:-1] + "G"


def _staging_seqs(W):
    barcodes, tags, miss = staging_index(W)
    return [barcodes[k % 3] + t for k, t in enumerate(tags + [CUT + miss])]


def _aligned_header(at, a, k, nl):
    """A header for a record that begins at byte `at`, padded so that the sequence line starts at a byte = a (mod 16)."""
    tail = " count=%d" % (3 + k)
    pad = (a - (at + len("@a%d" % k) + len(tail) + len(nl))) % 16
    return "@a%d%s%s%s" % (k, "x" * pad, tail, nl)


@functools.lru_cache(maxsize=None)
def staging_aligned(W, nl):
    """Every read ends at its tag's last base, then `nl`; every tag (and the miss) with its sequence line at every
    alignment 0..15."""
    out, k = "", 0
    for a in range(16):
        for seq in _staging_seqs(W):
            out += _aligned_header(len(out), a, k, nl) + seq + nl + "+" + nl + "II" + nl
            k += 1
            assert (out.rindex(seq) & 15) == a
    return out.encode()


@functools.lru_cache(maxsize=None)
def staging_tail(W, a):
    """The buffer ends at the tag's last base: the last line has no terminator and starts at alignment a."""
    seqs = _staging_seqs(W)
    out = "@f count=2\n%s\n+\nII\n" % seqs[(a + 1) % 6]
    out += _aligned_header(len(out), a, a, "\n") + seqs[a % 6]
    return out.encode()


def filler(n, seq="GGGG"):
    """Records that match nothing, exactly n bytes in all, none longer than 4 KiB."""
    out = []
    while n > 0:
        k = n if n <= 4096 else 4096 if n >= 4096 + 32 else n - 32
        head = "@p count=5\n%s\n+\n" % seq
        assert k > len(head) + 1
        out.append(head + "I" * (k - len(head) - 1) + "\n")
        n -= k
    return "".join(out)


def staging_slide_offsets(W):
    """Where the sequence line starts, relative to the tile boundary: in the tile's last 18 bytes and the next one's first
    three (every alignment, the halo in full use), and where the line's end, its \\r and its \\n meet the boundary."""
    n = 32 + 32 * W
    return sorted(set(list(range(-18, 3)) + [-n + j for j in range(-2, 3)] + [-(n // 2)]))


@functools.lru_cache(maxsize=None)
def staging_slide(W, d):
    """The sequence line of a \\r\\n record starts d bytes behind SEAM (before it: d < 0), a second record follows, 40 KiB of
    other records lie behind."""
    seqs = _staging_seqs(W)
    head = "@h count=7\r\n"
    out = filler(SEAM + d - len(head)) + head + seqs[d % 6] + "\r\n+\r\nII\r\n"
    out += "@h count=9\r\n" + seqs[(d + 1) % 6] + "\r\n+\r\nII\r\n" + filler(40 * 1024) + "@h count=4\n" + seqs[6] + "\n+\nII\n"
    assert out.index(seqs[d % 6]) == SEAM + d
    return out.encode()


def staging_case(W, data):
    barcodes, tags, _ = staging_index(W)
    return Case("staging W=%d" % W, barcodes, tags, CUT, None, data, 25, 0, None)


# ---------------------------------------------------------------------------------------------------- limits
@functools.lru_cache(maxsize=None)
def limit_case(L):
    """Three stored tags of L bases and two shorter: 320 is the longest the table takes."""
    rnd = random.Random("limit %d" % L)
    barcodes = make_barcodes(rnd, 2, 6)
    stored = random_tags(rnd, 3, L) + random_tags(rnd, 2, (40, 60))
    assert is_prefix_free(stored)
    return make_case("limit %d" % L, rnd, barcodes, stored, {}, nrandom=100)


def case_keys():
    """(builder, arguments) of every case of reads (the staging buffers apart); nothing is built here."""
    out = [("family_case", (L,)) for L in FAMILY_KEYS]
    out += [("ring_case", (W, k)) for W in WIDTHS for k in range(RING_STEMS)]
    out += [("dense_random_case", (W,)) for W in WIDTHS]
    out += [("allelic_case", (64,)), ("allelic_case", (96,))]
    out += [("short_case", (n,)) for n in SHORT_COUNTS]
    out += [("nq_case", (W, nq)) for W in (1, 2, 3) for nq in NQ[W]]
    out += [("wide_offset_case", (n,)) for n in WIDE_OFFSET_LENS]
    out += [("limit_case", (320,))]
    return out


def get_case(key):
    return globals()[key[0]](*key[1])


def all_cases():
    return [get_case(k) for k in case_keys()]
