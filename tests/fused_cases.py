"""Inputs for td_count_and_split_device, the call that counts and takes the splitter's decisions over one resident buffer.
Where the count pass was a free-running one with 24 KiB tiles and the splitter's kernel is k_split2, the splitter's line
index of every tile comes from the count kernel's own per-tile terminator records (prefix source 2); everywhere else the
terminators are counted from the bytes again (source 1).  A record that is off by one changes the line phase behind it,
one that is off by four changes nothing but the slot every later decision is written to.

Nothing is generated here that another module generates already:

  * every buffer of tests/splitter_edge_cases.py that ends without an error, with a count index beside its splitter set:
    the set's barcodes and cut site, and tags taken from the windows behind barcode + cut site that the buffer's own
    reads carry (at most MAX_TAGS of them, at most TAG_BASES bases: two or three 32-base words);
  * the count kernels' ring inputs of tests/ring_cases.py with a splitter beside their index: their barcodes, their cut
    site and the PstI-MspI-Hall adapter.

Plain Python; the product is not imported.  Expected decisions are the Python oracle's barcodeSplitter restatement,
expected matrices and counters the C oracle's; both are cached per case.  tests/test_fused.py shows from the bytes and
the oracles alone that each input can catch a wrong line index (shift_model); tests/test_fused_gpu.py and
tests/test_line_prefix_gpu.py run them.
"""
import bisect
import collections
import functools

import numpy as np

import ring_cases as rc
import splitter_edge_cases as ec
from oracle import c_oracle
from oracle import tagdigger_oracle as po

TILE2, TILE1 = 24576, 16384            # k_split2's tile (and k_fast4's, and k_fast2's at tile_kb2 = 24); k_split's
TILES = (TILE2, TILE1)
SENTINEL = 0x5A5A5A5A
SLACK = 8
MAX_TAGS, TAG_BASES = 200, 64
NO_BARCODE = (-1, 999)

# name, splitter set (an ec.Set), tags of the count index, bytes, labels per sequence line (or None), origin
Case = collections.namedtuple("Case", "name set tags data labels origin")


# ---------------------------------------------------------------------------------------------------- lines and decisions
def twin(data):
    return ec.ascii_twin(data)


@functools.lru_cache(maxsize=None)
def _trees(st):
    barcut = po.combine_barcode_and_cutsite(st.barcodes, st.cutsite)
    return po.build_sequence_tree(barcut, len(barcut)), po.build_adapter_tree(st.adapter, st.barcodes), ec.sites_of(st)


def _key(st):
    return ec.Set(tuple(st.adapter), tuple(st.barcodes), st.cutsite, st.compact)


def decide(st, raw):
    """(barcode index, findAdapterSeq value) as the kernels report them, for ONE line's raw bytes (any line: a line index
    that is wrong makes the splitter take a header or a quality line for a read)."""
    tree, trees, (s0, s1) = _trees(_key(st))
    s = twin(raw).strip(po.STRIP_BYTES).decode("ascii").upper()
    bar = po.sequence_index_lookup(s, tree)
    if bar < 0:
        return NO_BARCODE
    return bar, po.find_adapter_seq(s, trees[bar], s0, s1, len(st.barcodes[bar]) + len(st.cutsite))


def sequence_lines_are_ascii(data, first_line=0):
    return all(line.isascii() for k, line in enumerate(ec.lines_of(data)) if (first_line + k) & 3 == 1)


_decisions = {}


def expected_decisions(case, data=None, first_line=0):
    """int32 [sequence lines, 2]: splitter_edge_cases.expected_for -- the oracle's barcodeSplitter loop -- over the bytes
    (bytes >= 0x80 outside sequence lines replaced by a letter: the oracle decodes every line), cached.  first_line: 0 or 4, or 1 for bytes that begin with a
    sequence line (a header line is put in front for the oracle)."""
    data = case.data if data is None else data
    key = (case.name, len(data), first_line & 3)
    if key not in _decisions:
        assert first_line & 3 in (0, 1) and sequence_lines_are_ascii(data, first_line), case.name
        whole = (b"@\n" if first_line & 3 else b"") + twin(data)
        assert ec.seq_line_count(whole, 0) == ec.seq_line_count(data, first_line)
        arr = np.array(ec.expected_for(case.set, whole), dtype=np.int32).reshape(-1, 2)
        arr.setflags(write=False)
        _decisions[key] = arr
    return _decisions[key]


_counts = {}


def expected_counts(case, data=None, **kw):
    """(matrix, {"reads", "barcut", "tag", "lines"}) of the C oracle, cached; kw: first_line, maxreads."""
    data = case.data if data is None else data
    key = (case.name, len(data), tuple(sorted(kw.items())))
    if key not in _counts:
        if case.origin == "ring":
            m, st = rc.expected(rc.Case(case.name, list(case.set.barcodes), list(case.tags), case.set.cutsite, data), **kw)
        else:
            st = {}
            m = c_oracle.COracle(list(case.set.barcodes), list(case.tags), case.set.cutsite).count_bytes(data, stats=st, **kw)
        m.setflags(write=False)
        _counts[key] = (m, st)
    return _counts[key]


def n_terminators(data):
    return len(rc.terminator_ends(data))


def counted_read_offsets(case):
    """Start offsets of the sequence lines that the count index counts (barcode + cut site + tag), by the Python oracle's
    two lookups."""
    barcuttree, tagtree, barcutlen, _, _ = po.prepare_index(case.set.barcodes, case.tags, case.set.cutsite)
    starts = [0] + rc.terminator_ends(case.data)
    out = []
    for k, line in enumerate(ec.lines_of(case.data)):
        if k & 3 == 1:
            read = po.clean_read(line)
            bar = po.sequence_index_lookup(read, barcuttree)
            if bar > -1 and po.sequence_index_lookup(read[barcutlen[bar]:], tagtree) > -1:
                out.append(starts[k])
    return out


# ---------------------------------------------------------------------------------------------------- splitter edge cases
def _windows(st, data, bases=TAG_BASES):
    """(offset of the sequence line, window of up to `bases` bases behind barcode + cut site) for every sequence line
    that begins with a barcode and the cut site and goes on in ACGT."""
    tree = _trees(_key(st))[0]
    starts = [0] + rc.terminator_ends(data)
    out = []
    for k, line in enumerate(ec.lines_of(data)):
        if k & 3 != 1 or not line.isascii():
            continue
        s = line.strip(po.STRIP_BYTES).decode("ascii").upper()
        bar = po.sequence_index_lookup(s, tree)
        if bar < 0:
            continue
        w = s[len(st.barcodes[bar]) + len(st.cutsite):][:bases]
        n = next((i for i, ch in enumerate(w) if ch not in "ACGT"), len(w))
        if n >= 4:
            out.append((starts[k], w[:n]))
    return out


DEFAULT_WINDOWS = ("ATATATATATATATATATAT", "ATATATATCCGG", "ATATATATATATCCGCTC", "ATATATCTGCAGA", "ATATCC")


def choose_tags(st, data, bases=TAG_BASES):
    """Cut site + window: the windows of the last 24 KiB tile's reads first (the last tile goes its own way in every count
    kernel), then the others as they come; a window that is the beginning of a chosen one, or begins with one, is
    skipped (td_set_index takes the reference's rules: such tags shadow each other).  A buffer too short to carry a
    window gets the filler reads' windows."""
    wins = _windows(st, data, bases)
    last = (len(data) - 1) // TILE2
    order = [w for off, w in wins if off // TILE2 == last] + [w for _, w in wins] + list(DEFAULT_WINDOWS)
    tags = []
    for w in order:
        if len(tags) == MAX_TAGS:
            break
        if not any(w.startswith(t) or t.startswith(w) for t in tags):
            tags.append(w)
    return tuple(st.cutsite + t for t in tags)


@functools.lru_cache(maxsize=None)
def edge_cases():
    out = collections.OrderedDict()
    for name, c in ec.cases().items():
        if c.error is None:
            st = ec.SETS[c.set]
            out["edge:" + name] = Case("edge:" + name, _key(st), choose_tags(st, c.data), c.data, c.labels, "edge")
    return out


# ---------------------------------------------------------------------------------------------------- ring cases
@functools.lru_cache(maxsize=None)
def ring_set(barcodes, cutsite):
    st = ec.Set(tuple(ec.HALL), tuple(barcodes), cutsite, None)
    return st._replace(compact=ec.compact_form(st, ec.entries_from_oracle(st)))


def _ring_sources():
    yield "dirty", rc.g_dirty()
    yield "qual", rc.g_qual()
    yield "sparse", rc.g_sparse()
    yield "short", rc.g_short()
    yield "cr-quarter-ends", rc.g_cr_at_quarter_ends(False)
    yield "cr-quarter-ends-lone", rc.g_cr_at_quarter_ends(True)
    yield "qual-high-byte-in-halo", rc.g_qual_high_byte_in_halo()
    for boundary in sorted(rc.CRLF_BOUNDARIES):
        # the step that puts the header's \r on the boundary's last byte: its \n is the boundary's first
        case, target = rc.crlf_case(boundary, rc.CRLF_STEPS // 2, False)
        assert (target + 1 - rc.SWEEP_TILE * rc.TILE) == rc.CRLF_BOUNDARIES[boundary]
        yield "crlf-" + boundary.replace(" ", "-"), case
    for which, off in (("first", rc.HI_SPAN[0]), ("last", rc.HI_SPAN[1])):
        yield "high-byte-header-" + which, rc.hi_case(False, off)


def with_a_tail(c):
    """G_dirty's last copies of its block begin at line phases under which no read of the last tile is counted.  A few
    bytes behind the generator's own: empty lines up to a record's start, then two records -- barcode + tag, and the same
    with the common cutter's site behind it.  The generator's bytes stay as they are in front of them, so what
    tests/test_ring.py asserts of its tiles holds as it did (tests/test_fused.py: same tiles, same classes)."""
    data = c.data if c.data[-1:] in (b"\n", b"\r") else c.data + b"\n"
    data += b"\n" * (-rc.line_count(data) % 4)
    read = c.barcodes[0] + c.tags[0]
    for k, seq in enumerate((read + "ACGTAC", read + "AT" + ec.sites_of(ring_set(tuple(c.barcodes), c.cutsite))[0] + "AT")):
        data += ("@tail%d\n%s\n+\n%s\n" % (k, seq, "I" * len(seq))).encode()
    assert rc.ntiles(data) == rc.ntiles(c.data)
    return c._replace(data=data)


TAILED = ("dirty",)


@functools.lru_cache(maxsize=None)
def ring_cases():
    out = collections.OrderedDict()
    for name, c in _ring_sources():
        if name in TAILED:
            c = with_a_tail(c)
        out["ring:" + name] = Case("ring:" + name, ring_set(tuple(c.barcodes), c.cutsite), tuple(c.tags), c.data, None, "ring")
    return out


SHORT_READS = ("AACGTGCAGATCCGGA", "TTGACCTGCAGGTTC", "GGGG", "CGTTGCAGATCC", "CCACTGCAGACGC")
SHORT_TILES = 5


@functools.lru_cache(maxsize=None)
def short_records():
    """Records of some 18 bytes, four lines each ("@", a read of 4 to 16 bases, "+", "I"): a line is 4.6 bytes on average.
    This is the one input here on which a maxreads bound can stop the count inside the buffer and still leave the count
    pass free-running: launch_count takes that path only where the bound's line, 4 (maxreads - 1) + 1, is at least
    nbytes / 16, and every other input's lines are 18 bytes and longer.  Every quarter of every tile holds more
    terminators than a list of line starts (384): the count kernels record such tiles with TI_SKIP, k_split2 walks them in
    global memory."""
    st = ec.SETS["hall"]
    recs = [("@\n%s\n+\nI\n" % r).encode() for r in SHORT_READS]
    data, k = bytearray(), 0
    while len(data) < SHORT_TILES * TILE2 - 100:
        data += recs[k % len(recs)]
        k += 1
    data = bytes(data)
    return Case("extra:short-records", _key(st), choose_tags(st, data), data, None, "extra")


def bound_is_far(nbytes, maxreads, first_line=0):
    """launch_count's limit_far restated: the bound's line lies at least nbytes / 16 lines behind the buffer's first."""
    limit_line = 4 * (maxreads - 1) + 1
    return limit_line - min(limit_line, first_line) >= nbytes // 16


@functools.lru_cache(maxsize=None)
def cases():
    out = collections.OrderedDict(edge_cases())
    out.update(ring_cases())
    c = short_records()
    out[c.name] = c
    return out


# ---------------------------------------------------------------------------------------------------- the shift model
SHIFTS = (1, -1, 4, -4)


class LineTable:
    """Every line of a case with the decision the splitter would take if it read that line as a read."""

    def __init__(self, case):
        self.case = case
        lines = ec.lines_of(case.data)
        self.nlines = len(lines)
        self.ends = rc.terminator_ends(case.data)
        # quality lines (phase 3) are never read as reads under a shift of 1, -1, 4 or -4
        self.dec = np.array([decide(case.set, line) if k & 3 != 3 else NO_BARCODE for k, line in enumerate(lines)],
                            dtype=np.int64).reshape(-1, 2)
        self.nseq = ec.seq_line_count(case.data, 0)

    def first_line_behind(self, boundary):
        """Index of the first line that starts at or behind the offset: the lines a tile's line index is used for."""
        return bisect.bisect_left(self.ends, boundary) + 1

    def slots(self, first_shifted=None, shift=0):
        """The output as the kernels write it -- slot = sequence-line ordinal = line >> 2 for lines of index 1 mod 4,
        decision = that line's -- with `shift` added to the index of every line from first_shifted on.  One slot more
        than SLACK is kept behind the last, so that a write past the end shows; a slot that is never written keeps the
        sentinel."""
        out = np.full((self.nseq + SLACK + 1, 2), SENTINEL, dtype=np.int64)
        k = np.arange(self.nlines)
        idx = k + (np.where(k >= first_shifted, shift, 0) if shift else 0)
        ok = (idx >= 0) & ((idx & 3) == 1)
        out[np.minimum(idx[ok] >> 2, len(out) - 1)] = self.dec[k[ok]]
        return out


@functools.lru_cache(maxsize=None)
def line_table(name):
    return LineTable(cases()[name])


def boundaries(data, tile):
    return range(tile, len(data), tile)


# ---------------------------------------------------------------------------------------------------- more than 8 192 tiles
SCAN_ROUND = 8192                       # tiles k_scan_tiles takes per round of its loop: behind them `carry` crosses it
BIG_FILLER_TILES = SCAN_ROUND + 1


@functools.lru_cache(maxsize=None)
def big_block():
    """Three records of 101 to 135 bytes whose reads begin with no barcode of the set "hall": every decision is (-1, 999) and
    nothing is counted.  353 bytes: the copies lie at every alignment, and the terminators in front of tile SCAN_ROUND are no
    multiple of 4 at either tile size (tests/test_fused.py)."""
    recs = []
    for k, (pad, n) in enumerate(((44, 20), (55, 31), (38, 24))):
        seq = "GGGG" + ec.expand(ec.at(n))
        recs.append("@filler%d %s\n%s\n+\n%s\n" % (k, "x" * pad, seq, "I" * len(seq)))
    block = "".join(recs).encode()
    assert len(block) % 16 != 0 and len(block) % 4 != 0
    return block


def big_filler(tile):
    """BIG_FILLER_TILES tiles exactly, so that the case behind it keeps its seams at tile ends: whole blocks, then whole
    records, then one record whose header line takes up the rest."""
    block = big_block()
    total = BIG_FILLER_TILES * tile
    reps = (total - 400) // len(block)
    rest = total - reps * len(block)
    seq = b"GGGGATATATAT"
    last = b"@" + b"x" * (rest - 2 * len(seq) - 6) + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"
    data = block * reps + last
    assert len(data) == total
    return data, 3 * reps + 1


def big_case(tile):
    """(bytes, sequence lines of the filler, the geometry case of that tile size): more than SCAN_ROUND tiles in front of a
    case whose every decision is known."""
    case = cases()["edge:geometry-%d" % tile]
    filler, nseq = big_filler(tile)
    return filler + case.data, nseq, case


def big_terminators_in_first_round(tile):
    """Terminators of the filler whose last byte lies in the first SCAN_ROUND tiles, from the block's own."""
    block = big_block()
    ends = rc.terminator_ends(block)
    limit = SCAN_ROUND * tile
    whole = limit // len(block)
    assert whole < (BIG_FILLER_TILES * tile - 400) // len(block)         # (the boundary lies inside the repeated blocks)
    return whole * len(ends) + bisect.bisect_right(ends, limit - whole * len(block))


# ---------------------------------------------------------------------------------------------------- one-off inputs
def adhoc(name, data, tags=None, setname="hall"):
    """A buffer for the set `setname` with tags of its own windows (or the tags given)."""
    st = ec.SETS[setname]
    return Case(name, _key(st), tuple(tags) if tags is not None else choose_tags(st, data), data, None, "extra")


@functools.lru_cache(maxsize=None)
def wide_case():
    """The read case "hall-A" with tags of up to 100 bases: four 32-base words, a width that only k_fast counts."""
    base = cases()["edge:hall-A"]
    tags = []
    for _, w in sorted(_windows(base.set, base.data, 100), key=lambda x: -len(x[1])):       # (the longest first: nothing shadows them)
        if len(tags) < MAX_TAGS and not any(w.startswith(t) or t.startswith(w) for t in tags):
            tags.append(w)
    tags = tuple(base.set.cutsite + t for t in tags)
    assert max(len(t) for t in tags) - len(base.set.cutsite) == 100
    return base._replace(name="extra:wide-tags", tags=tags, origin="extra")


@functools.lru_cache(maxsize=None)
def rotated_case():
    """geometry-24576 with its first record moved to the end: as many tiles, other terminator counts in them."""
    base = cases()["edge:geometry-24576"]
    cut = rc.terminator_ends(base.data)[3]
    data = base.data[cut:] + b"\n" + base.data[:cut]
    return base._replace(name="extra:geometry-rotated", data=data[:len(base.data)], labels=None, origin="extra")
