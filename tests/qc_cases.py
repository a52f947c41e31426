"""Shared by tests/test_qc.py and tests/test_qc_gpu.py: the library QC rule restated over bytes, with the
oracle's line splitting, strip set, clean_read and tree for the barcode + cut site lookup; inputs for the tests."""
import random

import numpy as np

from oracle import tagdigger_oracle as orc

ACGT = "ACGT"
STATS = ("reads", "barcut", "qual_lines", "bases", "qual_bases", "qual_invalid", "empty_qual")
TABLES = ("barcodes", "base_cycle", "qual_cycle", "lengths", "meanq")
BASE_CLASS = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
BARCODES = ["ACGT", "TGACA", "GATTAC", "CCTAGGA", "TTGGCCAA", "AGAGTCTCA"]       # lengths 4..9, prefix-free


def ref_qc(data, barcodes, cutsite="TGCAG", C=160, maxreads=5e9):
    """{stats, barcodes, base_cycle, qual_cycle, lengths, meanq} of FASTQ bytes: record r is lines 4r .. 4r + 3, the
    records below max(1, ceil(maxreads)) are looked at, every line on its own."""
    barcut, barnum, _, _ = orc.prepare_lists(barcodes, ["A"], cutsite)
    tree = orc.build_sequence_tree(barcut, barnum)
    R = max(1, -int(-maxreads // 1))
    B = len(barcodes)
    bar = [[0, 0, 0] for _ in range(B + 1)]
    base = [[0] * 6 for _ in range(C + 1)]
    qual = [[0] * 95 for _ in range(C + 1)]
    lengths = [0] * (C + 1)
    meanq = [0] * 94
    st = dict.fromkeys(STATS, 0)
    for k, raw in enumerate(orc.iter_lines(data)):
        if k // 4 >= R:
            break
        if k % 4 == 1:
            line1 = orc.clean_read(raw)
            b = orc.sequence_index_lookup(line1, tree)
            if b == -1:
                b = B
            n = len(line1)
            st["reads"] += 1
            st["barcut"] += b < B
            st["bases"] += n
            bar[b][0] += 1
            bar[b][1] += n
            bar[b][2] += any(ch not in ACGT for ch in line1)
            lengths[min(n, C)] += 1
            for i, ch in enumerate(line1):
                base[min(i, C)][BASE_CLASS.get(ch, 5)] += 1
        elif k % 4 == 3:
            q = raw.strip(orc.STRIP_BYTES)
            qsum = nvalid = 0
            for i, v in enumerate(q):
                if 33 <= v <= 126:
                    qual[min(i, C)][v - 33] += 1
                    qsum += v - 33
                    nvalid += 1
                else:
                    qual[min(i, C)][94] += 1
            st["qual_lines"] += 1
            st["qual_bases"] += nvalid
            st["qual_invalid"] += len(q) - nvalid
            if nvalid == 0:
                st["empty_qual"] += 1
            else:
                meanq[qsum // nvalid] += 1
    u = lambda x: np.array(x, dtype=np.uint64)
    return dict(stats=st, barcodes=u(bar), base_cycle=u(base), qual_cycle=u(qual), lengths=u(lengths), meanq=u(meanq))


def times(ref, k):
    """The QC of k copies of an input made of whole records: every line is decided on its own, so everything scales."""
    out = {name: ref[name] * np.uint64(k) for name in TABLES}
    out["stats"] = {name: v * k for name, v in ref["stats"].items()}
    return out


def plus(a, b):
    out = {name: a[name] + b[name] for name in TABLES}
    out["stats"] = {name: a["stats"][name] + b["stats"][name] for name in STATS}
    return out


def same(got, want):
    """Exact equality of every total and every table; `got` is a QCResult or a dict like ref_qc's."""
    if not isinstance(got, dict):
        got = dict(stats=got.stats, barcodes=got.barcodes, base_cycle=got.base_cycle, qual_cycle=got.qual_cycle, lengths=got.lengths,
                   meanq=got.meanq)
    assert {k: int(got["stats"][k]) for k in STATS} == want["stats"]
    for name in TABLES:
        g, w = np.asarray(got[name]), want[name]
        assert g.shape == w.shape and g.dtype == np.uint64, name
        if not (g == w).all():
            at = np.argwhere(g != w)[:5]
            raise AssertionError("%s differs at %s: got %s, want %s" % (name, at.tolist(), [int(g[tuple(i)]) for i in at], [int(w[tuple(i)]) for i in at]))
    return True


def check_invariants(res):
    st = res["stats"] if isinstance(res, dict) else res.stats
    get = (lambda n: res[n]) if isinstance(res, dict) else (lambda n: getattr(res, n))
    assert int(get("lengths").sum()) == int(get("barcodes")[:, 0].sum()) == st["reads"]
    assert int(get("base_cycle").sum()) == st["bases"] == int(get("barcodes")[:, 1].sum())
    assert int(get("meanq").sum()) + st["empty_qual"] == st["qual_lines"]
    assert int(get("qual_cycle").sum()) == st["qual_bases"] + st["qual_invalid"]
    assert int(get("qual_cycle")[:, 94].sum()) == st["qual_invalid"]
    assert int(get("barcodes")[:-1, 0].sum()) == st["barcut"]


def rand_seq(rnd, n, alphabet=ACGT):
    return "".join(rnd.choice(alphabet) for _ in range(n))


def rand_qual(rnd, n):
    return "".join(chr(33 + min(93, max(0, int(rnd.gauss(34, 8))))) for _ in range(n))


def records(pairs, nl=b"\n", last_nl=True):
    """FASTQ bytes of (sequence line, quality line) pairs given as bytes."""
    out = bytearray()
    for i, (s, q) in enumerate(pairs):
        out += b"@r%d" % i + nl + s + nl + b"+" + nl + q + nl
    if not last_nl and out:
        del out[len(out) - len(nl):]
    return bytes(out)


def library(rnd, nreads, barcodes=BARCODES, lo=30, hi=160):
    """(sequence, quality) pairs: barcode + site + random tail, some without a barcode, with N, in lower case, with other
    letters; qualities of the same length, or another one now and then (every line is decided on its own)."""
    pairs = []
    for _ in range(nreads):
        n = rnd.randint(lo, hi)
        roll = rnd.random()
        if roll < 0.08:
            s = rand_seq(rnd, n)
        else:
            s = (rnd.choice(barcodes) + "TGCAG" + rand_seq(rnd, hi))[:n]
            if roll < 0.14:
                k = rnd.randrange(len(s))
                s = s[:k] + rnd.choice("NnRX.-") + s[k + 1:]
            elif roll < 0.18:
                s = s.lower()
        q = rand_qual(rnd, n if rnd.random() < 0.9 else rnd.randint(0, hi))
        pairs.append((s.encode(), q.encode()))
    return pairs


# ------------------------------------------------------------------------------------------------------------------ inputs
TILE = 16384                                   # the kernel's tile
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257)


def length_input(C, seed=21):
    """Sequence and quality lines of the lengths at which the kernel's 16-byte chunks, 256-byte steps and the table
    rows change, C - 1, C and C + 1 among them, and one of 40 000 bytes (more than two tiles; the overflow row)."""
    rnd = random.Random(seed)
    pairs = []
    for n in list(LENGTHS) + [C - 1, C, C + 1, 40000]:
        s = (rnd.choice(BARCODES) + "TGCAG" + rand_seq(rnd, n))[:n]
        pairs.append((s.encode(), rand_qual(rnd, n).encode()))
        pairs.append((rand_seq(rnd, 40, "ACGTN").encode(), rand_qual(rnd, 33).encode()))
    return records(pairs)


def byte_values_input(seed=22):
    """Quality lines holding every byte value except the two terminators in their interior, at varying cycles; the same
    bytes below 0x80 in sequence lines."""
    rnd = random.Random(seed)
    interior = [v for v in range(256) if v not in (10, 13)]
    pairs = []
    for k in range(6):
        rnd.shuffle(interior)
        q = b"I" * k + bytes(interior) + b"#"
        s = b"ACGTTGCAG" + bytes(v for v in interior if v < 0x80) + b"A"
        pairs.append((s, q))
    pairs.append((b"ACGTTGCAGAC", bytes([0x80, 0xFF, 0x01])))          # no valid byte at all
    pairs.append((b"", b""))
    return records(pairs)


def strip_input():
    """Every strip byte at both ends of both lines, blank-only lines, blanks kept in the interior."""
    blanks = [bytes([b]) for b in orc.STRIP_BYTES if b not in (10, 13)]
    pairs = []
    for k, sb in enumerate(blanks):
        pairs.append((sb * (k + 1) + b"ACGTTGCAGAACC" + sb * 2, sb * 2 + b"IIIIFFFF##" + sb * (k + 1)))
        pairs.append((sb + b"acgtTGCAG" + sb + b"AC" + sb, b"II" + sb + b"II"))
        pairs.append((sb * 3, sb * 20))
    pairs.append((b"".join(blanks) * 40 + b"TGACATGCAGTT" + b"".join(blanks), b"".join(blanks) * 40 + b"5" + b"".join(blanks) * 3))
    return records(pairs)


def seam_input(nl, delta, which, seed=23):
    """More than three tiles with terminator `nl`; the sequence (which = 1) or quality (which = 3) line of one record
    starts at byte TILE + delta (tile 1) resp. 2 * TILE + delta."""
    rnd = random.Random(seed + 7 * delta + which)
    target = (1 if which == 1 else 2) * TILE + delta
    out = bytearray()
    pairs = library(rnd, 700, lo=20, hi=150)
    placed = False
    for i, (s, q) in enumerate(pairs):
        head = b"@r%d" % i
        if not placed:
            before = len(s) + len(nl) + 1 + len(nl) if which == 3 else 0      # bytes between the header's end and the line
            room = target - len(out) - len(head) - len(nl) - before
            if 0 <= room < 400:
                head += b"x" * room
                placed = True
        start = len(out)
        out += head + nl + s + nl + b"+" + nl + q + nl
        if placed and room is not None:
            at = start + len(head) + len(nl) + (len(s) + len(nl) + 1 + len(nl) if which == 3 else 0)
            assert at == target, (at, target)
            room = None
    assert placed and len(out) > 3 * TILE + 100
    return bytes(out)


def tail_inputs(seed=24):
    """Files whose last record lacks its quality line, its terminator, or ends in a bare CR."""
    rnd = random.Random(seed)
    body = records(library(rnd, 30))
    return {
        "no_quality": body + b"@last\nACGTTGCAGACGT\n+\n",
        "no_quality_no_plus": body + b"@last\nACGTTGCAGACGT",
        "no_terminator": body + b"@last\nACGTTGCAGACGT\n+\nIIIIIIIIIIIII",
        "ends_in_cr": body.replace(b"\n", b"\r") + b"@last\rACGTTGCAGACGT\r+\rIIIIIIIIIIIII\r",
        "ends_in_crlf_cut": body + b"@last\nACGTTGCAGACGT\n+\nIIIII\r",
    }


_REF = {}


def ref_cached(name, data, barcodes, cutsite, C, maxreads=5e9):
    """ref_qc, computed once per named input and never changed by a test."""
    key = (name, C, maxreads)
    if key not in _REF:
        _REF[key] = ref_qc(data, barcodes, cutsite, C, maxreads)
    return _REF[key]


_INPUTS = {}


def named_inputs():
    """name -> (bytes, C): the edge-case inputs both test files run."""
    if not _INPUTS:
        _INPUTS["lengths_c160"] = (length_input(160), 160)
        _INPUTS["lengths_c20"] = (length_input(20, seed=31), 20)
        _INPUTS["byte_values"] = (byte_values_input(), 50)
        _INPUTS["strip"] = (strip_input(), 160)
        for nl in (b"\n", b"\r\n", b"\r"):
            for delta in (-1, 0, 1, 2):
                tag = {b"\n": "lf", b"\r\n": "crlf", b"\r": "cr"}[nl]
                _INPUTS["seam_%s_%d_seq" % (tag, delta)] = (seam_input(nl, delta, 1), 160)
            _INPUTS["seam_%s_0_qual" % tag] = (seam_input(nl, 0, 3), 160)
            _INPUTS["seam_%s_1_qual" % tag] = (seam_input(nl, 1, 3), 160)
        for name, data in tail_inputs().items():
            _INPUTS["tail_" + name] = (data, 160)
    return _INPUTS
