"""Inputs and references for the weighted count (find_tags_fastq's tassel_tagcount=True, reference
tagdigger_fun.py:251-253 and :264-267): a header's `count=N` is added to the cell instead of 1.

Plain Python; the product is not imported here.  tests/test_weighted.py checks on the CPU that the two references
agree on every case below -- the literal rule with Python integers (oracle.tagdigger_oracle.count_bytes) and its
C restatement (oracle.c_oracle) -- and tests/test_weighted_gpu.py holds the kernel against them.

The rule reads EVERY line of phase 0 as a header: a blank line there, or a '+' line that a phase shift has moved
there, is a ValueError.  The generator therefore keeps blank lines out of phase 0, and where it shifts the phase
for good every line of a record carries a count= field of its own, so that a weight taken from the wrong line
changes a cell instead of raising."""
import collections
import functools
import hashlib
import random

from helpers import small_index
from oracle import c_oracle
from oracle import tagdigger_oracle as orc

Case = collections.namedtuple("Case", "name barcodes tags cutsite data maxreads first_line")
Case.__new__.__defaults__ = (5e9, 0)

TILE = 16 * 1024            # the weighted kernel's tile
HALO = 128


# ---------------------------------------------------------------------------------------------------- references
def _py_prefix(first_line):
    """`first_line` lines in front of a buffer that the rule reads without effect: a header of weight 0 in
    phase 0, blank lines elsewhere.  Returns (bytes, reads among them)."""
    text = b"".join(b"@ count=0\n" if (i & 3) == 0 else b"\n" for i in range(first_line))
    return text, (first_line + 2) // 4


def py_reference(case):
    """("ok", matrix as lists of Python ints, {"reads", "barcut", "tag"}) or ("raises", exception type), by the
    literal rule.  first_line is stated through lines in front of the buffer."""
    prefix, extra = _py_prefix(case.first_line)
    st = {}
    try:
        m = orc.count_bytes(prefix + case.data, case.barcodes, case.tags, case.cutsite,
                            maxreads=case.maxreads + extra, tassel_tagcount=True, stats=st)
    except (ValueError, AssertionError, IndexError, TypeError) as e:
        return ("raises", type(e))
    st["reads"] -= extra
    return ("ok", m, st)


def c_reference(case):
    """The same from the C oracle; its stats also hold "lines"."""
    st = {}
    try:
        m = c_oracle.COracle(case.barcodes, case.tags, case.cutsite).count_bytes(
            case.data, maxreads=case.maxreads, tassel_tagcount=True, first_line=case.first_line, stats=st)
    except (ValueError, AssertionError, IndexError, TypeError) as e:
        return ("raises", type(e))
    return ("ok", m.astype("int64").tolist(), st)


def line_count(data):
    return data.count(b"\n") + data.count(b"\r") - data.count(b"\r\n")


# ---------------------------------------------------------------------------------------------------- generator
def weight_text(rnd):
    """A value int() accepts: 0, 1, small, negative, up to 2^40; signs, leading zeros, underscores, blanks."""
    u = rnd.random()
    w = (0 if u < 0.05 else 1 if u < 0.25 else rnd.randint(2, 40) if u < 0.6 else -rnd.randint(1, 1000) if u < 0.75
         else rnd.randint(41, 1 << 40))
    f = rnd.random()
    if f < 0.1 and w >= 0:
        s = "+" + str(w)
    elif f < 0.2:
        s = ("-" if w < 0 else "") + "00" + str(abs(w))
    elif f < 0.3:
        s = format(w, "_")
    else:
        s = str(w)
    if rnd.random() < 0.2:
        s = rnd.choice([" ", "\t", " \x0b", "\x1c"]) + s + rnd.choice(["", " ", "\t\x0c", "\x1f "])
    return s


def weighted_fastq(rnd, barcodes, tags, cutsites, nrec, nl_choices=("\n",), long_lines=False, permanent_shifts=False,
                   all_lines=None, fillers=True):
    """helpers.dirty_fastq with count= headers: blank lines, N, lower case, every terminator style, long lines,
    phase shifts, reads that match nothing.  all_lines (default: permanent_shifts): every line of a record
    carries a weight of its own.  fillers=False: no lines between the records."""
    if all_lines is None:
        all_lines = permanent_shifts
    out = []
    state = {"line": 0, "nl": ""}

    def emit(text, nl):
        if text == "" and nl[0] == "\n" and state["nl"][-1:] == "\r":
            nl = "\r" + nl                       # (a blank line behind a bare \r: its \n must not complete a \r\n)
        out.append(text + nl)
        state["line"] += 1
        state["nl"] = nl

    def field(text):
        return text + rnd.choice([" ", "", ";", "\t"]) + "count=" + weight_text(rnd)

    def filler(n):          # n lines between two records: junk with a weight in phase 0, blank elsewhere
        for _ in range(n):
            nl = rnd.choice(["\n", "\r\n", "\r"])
            emit(field("#") if (state["line"] & 3) == 0 else "", nl)

    for ri in range(nrec):
        u = rnd.random()
        b = rnd.choice(barcodes)
        cs = rnd.choice(cutsites)
        t = rnd.choice(tags)
        carries = len(cs) > 0 and t[:len(cs)] in cutsites
        if u < 0.55:
            seq = b + (t if carries else cs + t) + "".join(rnd.choice("ACGT") for _ in range(rnd.randint(0, 30)))
        elif u < 0.7:
            seq = b + cs + "".join(rnd.choice("ACGT") for _ in range(rnd.randint(0, 80)))
        elif u < 0.85:
            seq = "".join(rnd.choice("ACGTN") for _ in range(rnd.randint(0, 120)))
        else:
            seq = b + (t if carries else cs + t)
            if seq:
                p = rnd.randrange(len(seq))
                seq = seq[:p] + rnd.choice("Nn.-*RYX\x00~`[{@") + seq[p + 1:]
        if rnd.random() < 0.2:
            seq = seq.lower()
        if rnd.random() < 0.08:
            seq = rnd.choice([" ", "\t", "  ", "\x0b\x0c", "\x1c\x1d\x1e\x1f "]) + seq + rnd.choice(["", " ", "\t "])
        if long_lines and rnd.random() < 0.02:
            seq = " " * rnd.randint(100, 700) + seq
        if rnd.random() < 0.05:
            seq = seq[:rnd.randint(0, len(seq))]
        if rnd.random() < 0.1:
            hdr = "@r%03d" % (ri % 1000) + weight_text(rnd)       # no count=: the slice [5:]
        else:
            hdr = "@r%d" % ri + ("" if rnd.random() < 0.8 else " " + "x" * rnd.randint(0, 40))
            if long_lines and rnd.random() < 0.02:
                hdr += " " + "y" * rnd.randint(100, 700)
            hdr = field(hdr)
        plus, qual = "+", "I" * (len(seq) if rnd.random() < 0.9 else rnd.randint(0, 5))
        if all_lines:
            seq, plus, qual = field(seq), field(plus), field(qual)
        nl = rnd.choice(nl_choices)
        if rnd.random() < 0.03:
            nl = rnd.choice(["\n", "\r\n", "\r"])
        for text in (hdr, seq, plus, qual):
            emit(text, nl)
        r = rnd.random() if fillers else 1.0
        if r < 0.01:
            filler(4)                                                   # four lines: phase kept
        elif r < 0.012:
            k = rnd.randint(1, 3)                                       # phase lost ...
            filler(k)
            if not (permanent_shifts and rnd.random() < 0.3):
                filler(4 - k)                                           # ... and usually restored
    return "".join(out).encode("latin-1")


# ---------------------------------------------------------------------------------------------------- header grammar
G_BAR, G_TAG = ["AACG"], ["TGCAGAAAC"]
G_BODY = "\nAACGTGCAGAAACTT\n+\nIIII\n"
LONG_HEADER = "@" + "x" * (TILE + HALO + 50) + " count=77"
# (header, does int() take it?)
HEADERS = [
    ("@r count=12", True), ("@r count= 12 ", True), ("@r count=\t12\x0b", True), ("@r count=007", True),
    ("@r count=12\x1c\x1f", True), ("@r count=0", True), ("@r count=-0", True), ("@r count=1099511627776", True),
    ("@r count=+7", True), ("@r count=-3", True), ("@r count=- 3", False), ("@r count=+ 7", False),
    ("@r count=++7", False), ("@r count=+", False),
    ("@r count=12 count=13", False),
    ("@r count=", False), ("@r count=   ", False), ("@r count=1.0", False), ("@r count=1e3", False), ("@r count=0x10", False),
    ("@abcd42", True), ("@ab", False), ("@abcd", False), ("@abcd 4 2", False),
    (LONG_HEADER, True),
    ("@r count=1_0", True), ("@r count=+1_0", True), ("@r count=-1_000_000", True), ("@r count=0_0", True),
    ("@r count=1__0", False), ("@r count=_1", False), ("@r count=1_", False), ("@r count=-_1", False), ("@r count=1_ 0", False),
]


def literal_rule(header):
    """The reference's own expression (:252) on one header line."""
    line = header + "\n"
    return int(line[line.find("count=") + 6:].strip())


def grammar_cases():
    return [Case("header %d %r" % (i, h[:40]), G_BAR, G_TAG, "TGCAG", (h + G_BODY).encode("latin-1"))
            for i, (h, ok) in enumerate(HEADERS)]


def maxreads_header_cases():
    """A bad header on read 2: beyond maxreads = 1 it is never read, at maxreads = 2 it raises."""
    data = ("@a count=3" + G_BODY + "@b count=x" + G_BODY).encode()
    return [Case("bad header behind maxreads", G_BAR, G_TAG, "TGCAG", data, 1),
            Case("bad header on read maxreads", G_BAR, G_TAG, "TGCAG", data, 2)]


def buffer_end_cases():
    rec = "@a count=3" + G_BODY
    texts = [
        ("header last, terminated", rec + "@b count=5\n"),
        ("header last, CRLF", rec + "@b count=5\r\n"),
        ("header last, unterminated", rec + "@b count=5"),
        ("bad header last, terminated", rec + "@b count=zz\n"),
        ("bad header last, unterminated", rec + "@b count=zz"),
        ("sequence line unterminated", rec + "@b count=5\nAACGTGCAGAAAC"),
        ("sequence line ends in a bare CR", rec + "@b count=5\rAACGTGCAGAAAC\r"),
        ("empty header line first", "\nAACGTGCAGAAAC\n+\nII\n"),
        ("empty header line later", rec + "\nAACGTGCAGAAAC\n+\nII\n"),
        ("partial record: no quality line", rec + "@b count=9\nAACGTGCAGAAACTT\n+"),
        ("partial record: sequence cut short", rec + "@b count=9\nAACGTG"),
        ("header only", "@b count=9"),
        ("header only, terminated", "@b count=9\n"),
    ]
    return [Case(name, G_BAR, G_TAG, "TGCAG", t.encode()) for name, t in texts]


# ---------------------------------------------------------------------------------------------------- tile seams
SWEEP_BAR, SWEEP_TAGS = ["AACG", "TTGACC"], ["TGCAGAAAC", "TGCAGGGGT", "TGCAGCCTA"]
SWEEP_PADS = list(range(TILE - 40, TILE + 8))


def tile_sweep_case(pad):
    """Four tiles; a \\r\\n record slides across the boundary between the second and the third, from its '@' to the
    first bases of its sequence line.  Six records, each with a cell and a weight of its own."""
    cells = [(b, t) for b in SWEEP_BAR for t in SWEEP_TAGS]

    def padded(n, k):          # record k, exactly n bytes long
        b, t = cells[k]
        head = ("@p count=%d\n%s%s\n+\n" % (1000 + 7 * k, b, t)).encode()
        return head + b"I" * (n - len(head) - 1) + b"\n"

    def rec(k):
        b, t = cells[k]
        return ("@h count=%d\r\n%s%sTT\r\n+\r\nIIII\r\n" % (12345 + 1000 * k, b, t)).encode()
    data = padded(TILE, 0) + padded(pad, 1) + rec(2) + rec(3) + padded(TILE, 4) + padded(TILE // 2, 5)
    return Case("tile seam pad %d" % pad, SWEEP_BAR, SWEEP_TAGS, "TGCAG", data)


# ---------------------------------------------------------------------------------------------------- fuzz
FUZZ_SHAPES = [("TGCAG", ("\n",)), ("CWGC", ("\n",)), ("TGCAG", ("\r\n",)), ("TGCAT", ("\r",)),
               ("", ("\n", "\r\n", "\r")), ("RCATGY", ("\n", "\r\n"))]


@functools.lru_cache(maxsize=None)
def fuzz_case(cutsite, nl, seed):
    rnd = random.Random(7000 * seed + len(cutsite) + len(nl))
    barcodes, tags, cutsites = small_index(rnd, cutsite)
    data = weighted_fastq(rnd, barcodes, tags, cutsites, nrec=1500, nl_choices=nl, long_lines=(seed == 2),
                          permanent_shifts=(seed == 2))
    return Case("fuzz %r %r seed %d" % (cutsite, nl, seed), barcodes, tags, cutsite, data)


WIDTH_MAXLENS = (20, 60, 90, 125, 190, 300)        # tag lengths across the packed widths W = 1, 2, 3, 4, 6, 10 words


@functools.lru_cache(maxsize=None)
def width_case(maxlen):
    rnd = random.Random(300 + maxlen)
    barcodes = ["ACGTAC", "TTGA", "GGGTCCAATC"]
    tags = []
    while len(tags) < 30:
        t = "TGCAG" + "".join(rnd.choice("ACGT") for _ in range(rnd.randint(max(1, maxlen - 40), maxlen)))
        if not any(t.startswith(o) or o.startswith(t) for o in tags):
            tags.append(t)
    data = weighted_fastq(rnd, barcodes, tags, ["TGCAG"], nrec=400)
    return Case("tags up to %d bases" % maxlen, barcodes, tags, "TGCAG", data)


# ---------------------------------------------------------------------------------------------------- maxreads, first_line
@functools.lru_cache(maxsize=None)
def limits_base():
    """300 records, every line with a weight of its own (any first_line leaves a parsable line in phase 0)."""
    rnd = random.Random(41)
    barcodes, tags, cutsites = small_index(rnd, "TGCAG")
    data = weighted_fastq(rnd, barcodes, tags, cutsites, nrec=300, nl_choices=("\n", "\r\n"), all_lines=True, fillers=False)
    return Case("limits", barcodes, tags, "TGCAG", data)


def maxreads_cases():
    base = limits_base()
    n = py_reference(base)[2]["reads"]
    return [base._replace(name="maxreads %d of %d" % (m, n), maxreads=m) for m in (1, 77, n - 1, n, n + 1)]


def first_line_cases():
    """first_line = 1 (mod 4) opens the buffer with a sequence line that has no header: the reference has no
    answer for it (its weight is unbound), so it is not a case."""
    base = limits_base()
    return [base._replace(name="first_line %d" % f, first_line=f) for f in (0, 4, 8, 2, 3)]


# ---------------------------------------------------------------------------------------------------- 64-bit cells
def wide_cases():
    def recs(ws):
        return "".join("@r count=%d%s" % (w, G_BODY) for w in ws).encode()
    return [Case("cell sum beyond 2^32", G_BAR, G_TAG, "TGCAG", recs([2 ** 32 - 1, 5, 2 ** 33, 2 ** 40])),
            Case("negative cell sum", G_BAR, G_TAG, "TGCAG", recs([-10, 3, -(2 ** 35)]))]


# ---------------------------------------------------------------------------------------------------- piece seams
SEAM_R = 128                 # bytes per record
SEAM_PIECE = 64 * 1024       # the smallest staged piece and 64 BGZF members of 1 KiB
SEAM_NREC = 3 * SEAM_PIECE // SEAM_R + 40       # a little over three pieces
SEAM_LEADS = list(range(SEAM_R))


def _kmers(rnd, n, k):
    seen = []
    while len(seen) < n:
        s = "".join(rnd.choice("ACGT") for _ in range(k))
        if s not in seen:
            seen.append(s)
    return seen


@functools.lru_cache(maxsize=None)
def seam_index():
    rnd = random.Random(11)
    return _kmers(rnd, 40, 6), ["TGCAG" + s for s in _kmers(rnd, 40, 20)]


def _fixed_record(header, seq, nl, length):
    """A four-line record of exactly `length` bytes: the header is padded in front of its count= field (padding and
    quality are hex digits of a hash of the header, so that gzip does not shrink the file to a single piece)."""
    noise = hashlib.sha256(header.encode()).hexdigest() * (1 + length // 64)
    body = nl + seq + nl + "+" + nl + noise[-len(seq):] + nl
    name, _, cnt = header.partition(" ")
    pad = length - len(header) - len(body)
    assert pad >= 0, (length, header)
    return name + noise[:pad] + " " + cnt + body


@functools.lru_cache(maxsize=None)
def seam_case(lead, nl, nrec=SEAM_NREC):
    """`nrec` records of SEAM_R bytes, record k with weight 1000 + 7 k in cell (k // 40 % 40, k % 40) -- a cell of its
    own up to 1 600 records -- behind a lead-in record of `lead` bytes that matches nothing (lead + SEAM_R where
    `lead` is shorter than a record can be: the piece boundaries fall on the same bytes of the records behind it)."""
    barcodes, tags = seam_index()
    shortest = len("@l count=999983" + nl + "N" + nl + "+" + nl + "I" + nl)
    parts = []
    if lead:
        parts.append(_fixed_record("@l count=999983", "N", nl, lead if lead >= shortest else lead + SEAM_R))
    for k in range(nrec):
        parts.append(_fixed_record("@s%04d count=%d" % (k, 1000 + 7 * k), barcodes[k // 40 % 40] + tags[k % 40], nl, SEAM_R))
    return Case("piece seam lead %d %r" % (lead, nl), barcodes, tags, "TGCAG", "".join(parts).encode())


def seam_expected(case):
    """What a seam case counts, from its construction (tests/test_weighted.py holds it against both oracles):
    (matrix, stats)."""
    nrec = len(case.data) // SEAM_R if case.data.startswith(b"@s") else (len(case.data) - case.data.index(b"@s0000")) // SEAM_R
    m = [[0] * 40 for _ in range(40)]
    for k in range(nrec):
        m[k // 40 % 40][k % 40] += 1000 + 7 * k
    lead = 0 if case.data.startswith(b"@s") else 1
    return m, {"reads": nrec + lead, "barcut": nrec, "tag": nrec, "lines": 4 * (nrec + lead)}


def small_cases():
    """Every case of one buffer that the GPU module runs, apart from the sweeps and the piece seams."""
    return (grammar_cases() + maxreads_header_cases() + buffer_end_cases() + wide_cases() + maxreads_cases()
            + first_line_cases())
