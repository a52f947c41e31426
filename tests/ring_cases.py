"""Inputs that take k_fast4's ring of five LDS slots deep (csrc/kernel_fast4.hpp): with td_set_option "max_grid" = 1 one
workgroup takes every tile of a buffer of 40 tiles and more, so that every slot is used eight times and more, and "run"
decides where the line phase is carried and where it is voted.  The generators put into that regime what the clean
synthetic stream never holds: every terminator style and lines of any length (G_dirty), quality lines that read as
barcode + cut site + tag so that a vote picks them and the fix-up pass has counts to take back (G_qual), tiles with no
terminator, with more line starts than a quarter's list holds, with a high byte, with fewer wanted lines than a pass
needs (G_sparse), reads of a dozen bases (G_short), and a clean stream whose hits go to two cells of one hot-cache slot
(G_hotslot); then single bytes aimed at tile 17, whose slot has been used three times before: a high byte swept over the
tile's end and its halo, \\r\\n and \\r slid across a quarter's, a lane span's and a chunk's end, a \\r at every quarter's end.

Plain Python; the product is not imported here.  tests/test_ring.py asserts, from the bytes and the C oracle alone,
that every generator reaches its regime; tests/test_ring_gpu.py holds the kernels against the C oracle on these bytes.

Sizes.  A tile is 24 576 bytes; the buffers are 40 to 64 tiles -- G_short apart: its 60 000 reads (a progress window
ends at read 50 000) at a mean line of 17 to 20 bytes are some 180 tiles.
"""
import bisect
import collections
import functools
import random
import re

import helpers
from oracle import c_oracle

TILE = 24576
QUARTER = TILE // 4                 # a producer's job; its list holds LIST_CAP line starts
LIST_CAP = 384
HALO_MAX = 192
CUT = "TGCAG"
WINDOW = 50000                      # reads per progress window

Case = collections.namedtuple("Case", "name barcodes tags cutsite data")


def ntiles(data):
    return -(-len(data) // TILE)


def oracle(case):
    return c_oracle.COracle(case.barcodes, case.tags, case.cutsite)


def expected(case, data=None, **kw):
    """(matrix, {"reads", "barcut", "tag", "lines"}) of the C oracle."""
    st = {}
    m = oracle(case).count_bytes(case.data if data is None else data, stats=st, **kw)
    return m, st


def bases(rnd, n):
    return "".join(rnd.choices("ACGT", k=n))


def repeat_block(block, tiles):
    """`block` (bytes, not a multiple of 16 long: its copies lie at every alignment) repeated to at least `tiles` tiles."""
    assert len(block) % 16 != 0
    return block * -(-tiles * TILE // len(block))


# ---------------------------------------------------------------------------------------------------- tiles by their bytes
_TERMINATOR = re.compile(rb"\r\n|\n|\r")


def terminator_ends(data):
    """Offsets behind every line terminator (\\n, \\r\\n, lone \\r), ascending."""
    return [m.end() for m in _TERMINATOR.finditer(data)]


def line_count(data):
    return data.count(b"\n") + data.count(b"\r") - data.count(b"\r\n")


def tile_classes(data):
    """Per tile, from the bytes alone: {"hi": holds a byte >= 0x80, "over": a quarter with more than LIST_CAP terminators,
    "noterm": no terminator, "nstarts": terminators in it (the lines that start behind them)}.  A terminator belongs to the
    tile (and quarter) of its own last byte; the kernel's masks mark the \\r of a \\r\\n pair that is split across a boundary,
    one byte earlier: at the sizes asserted here the difference of one is immaterial, and the asserts keep a margin."""
    nt = ntiles(data)
    per_q = [0] * (4 * nt)
    for e in terminator_ends(data):
        per_q[(e - 1) // QUARTER] += 1
    out = []
    for t in range(nt):
        chunk = data[t * TILE:(t + 1) * TILE]
        q = per_q[4 * t:4 * t + 4]
        out.append({"hi": not chunk.isascii(),
                    "over": max(q) > LIST_CAP, "noterm": sum(q) == 0, "nstarts": sum(q)})
    return out


def interior(nt):
    """Not tile 0 and not the last two (the first and the tiles whose window crosses the buffer's end go other ways)."""
    return range(1, nt - 2)


# ---------------------------------------------------------------------------------------------------- G_dirty
@functools.lru_cache(maxsize=None)
def g_dirty(seed=1):
    """helpers.dirty_fastq with all three terminator styles, long lines and phase shifts that stay: a block of some 2 000
    records repeated to 44 tiles."""
    rnd = random.Random("ring dirty %d" % seed)
    barcodes, tags, cutsites = helpers.small_index(rnd, CUT)
    block = helpers.dirty_fastq(rnd, barcodes, tags, cutsites, nrec=2000, nl_choices=("\n", "\r\n", "\r"), long_lines=True,
                                permanent_shifts=True)
    if line_count(block) % 4 == 0:
        block += b"\r" if block.endswith(b"\r") else b"\n"         # (an empty line: the block's copies begin at different line phases)
    if len(block) % 16 == 0:
        block += b"@pad\nACGT\n+\nIIII\n"          # (17 bytes)
    return Case("dirty", barcodes, tags, CUT, repeat_block(block, 44))


# ---------------------------------------------------------------------------------------------------- G_qual
def qual_records(rnd, barcodes, tags, first, n):
    """@rN / blank + read / + / qread: read and qread are barcode + tag + 0 to 20 bases each, independent of each other; qread
    padded with bases or cut to the sequence line's length.  The sequence line opens with a blank (the reference strips
    it: the read counts; the kernel takes its raw-bytes route and the line has no vote), the quality line is the only one
    a vote can pick -- A C G T are Phred 32, 34, 38 and 51."""
    out = []
    for k in range(first, first + n):
        read = rnd.choice(barcodes) + rnd.choice(tags) + bases(rnd, rnd.randint(0, 20))
        qread = rnd.choice(barcodes) + rnd.choice(tags) + bases(rnd, rnd.randint(0, 20))
        line = " " + read
        qread = (qread + bases(rnd, max(0, len(line) - len(qread))))[:len(line)]
        out.append("@r%d\n%s\n+\n%s\n" % (k, line, qread))
    return out


QUAL_NREC = 7000
QUAL_SHIFT_TILE = 5


@functools.lru_cache(maxsize=None)
def g_qual(seed=1, shift=False):
    """QUAL_NREC records of qual_records (some 42 tiles).  shift: two empty lines between two records inside tile
    QUAL_SHIFT_TILE -- behind them the reference reads the quality lines as the sequences, and a phase carried from the
    buffer's start (run = 4096) that had the quality lines wanted has the blank-led lines wanted from there on."""
    rnd = random.Random("ring qual %d" % seed)
    barcodes, tags, _ = helpers.small_index(rnd, CUT)
    recs = qual_records(rnd, barcodes, tags, 0, QUAL_NREC)
    if shift:
        at, k = 0, 0
        while at < QUAL_SHIFT_TILE * TILE + TILE // 2:
            at += len(recs[k])
            k += 1
        recs.insert(k, "\n\n")
    return Case("qual shift" if shift else "qual", barcodes, tags, CUT, "".join(recs).encode())


QUAL_HEAD_TILES = 2


@functools.lru_cache(maxsize=None)
def g_qual_behind_clean_head(seed=1):
    """Two tiles and a bit of clean records (the sequence lines are the only ones a vote can pick: tile 1 votes right), then
    g_qual's records: a phase carried from tile 1 on stays right through tiles in which every vote would be wrong."""
    rnd = random.Random("ring qual head %d" % seed)
    base = g_qual(seed)
    head = "".join(clean_records(rnd, base.barcodes, base.tags, QUAL_HEAD_TILES * TILE + 1000))
    return Case("qual behind a clean head", base.barcodes, base.tags, CUT, head.encode() + base.data)


# ---------------------------------------------------------------------------------------------------- G_sparse
@functools.lru_cache(maxsize=None)
def g_sparse(seed=1):
    """Records of 2 to 6 KB (barcode + tag + filler, the quality as long) with, four times over: a line of 30 to 60 KB (a
    header, or a sequence and its quality: tiles with no terminator, nwant = 0, the slot goes straight back, and tiles
    with a handful of line starts beside them), a stretch of about 10 KB of 1- and 2-byte lines (four to a record: the
    phase holds; more than LIST_CAP terminators in a quarter), and a header with a byte >= 0x80."""
    rnd = random.Random("ring sparse %d" % seed)
    barcodes, tags, _ = helpers.small_index(rnd, CUT)
    pool = bases(rnd, 200000)
    out = []
    nrec = [0]

    def fill(n):
        o = rnd.randrange(len(pool) - n)
        return pool[o:o + n]

    def record(total=None, header=None):
        seq = rnd.choice(barcodes) + rnd.choice(tags)
        seq += fill((total if total is not None else rnd.randint(2048, 6144)) // 2 - len(seq))
        out.append("%s\n%s\n+\n%s\n" % (header or "@s%d" % nrec[0], seq, "I" * len(seq)))
        nrec[0] += 1

    def ordinary(nbytes):
        goal = sum(len(x) for x in out) + nbytes
        while sum(len(x) for x in out) < goal:
            record()

    for cycle in range(4):
        ordinary(4 * TILE)
        if cycle % 2 == 0:
            record(total=2048, header="@long " + "x" * rnd.randint(30000, 60000))
        else:
            record(total=2 * rnd.randint(30000, 60000))
        ordinary(3 * TILE)
        for _ in range(10240 // 6):             # "\nA\n\nC\n"-like records of four lines, six bytes
            out.append("\n%s\n\n%s\n" % (rnd.choice("ACGT"), rnd.choice("ACGTI")))
        ordinary(3 * TILE)
        record(header="@hi%d caf\xe9 %s" % (cycle, "y" * rnd.randint(0, 30)))
    ordinary(3 * TILE)
    return Case("sparse", barcodes, tags, CUT, "".join(out).encode("latin-1"))


# ---------------------------------------------------------------------------------------------------- G_short
SHORT_NREADS = 64000


@functools.lru_cache(maxsize=None)
def g_short(seed=1):
    """Sequence lines of 12 to 36 bytes, tags of 4 to 9 bases behind the site (tests/test_progress.py's
    test_windows_with_short_lines_and_a_bound), in stretches of 400 records that are long (30 to 36) or, one in six, short
    (12 to 20): the short ones put more line starts into a quarter than its list holds, the long ones do not."""
    rnd = random.Random("ring short %d" % seed)
    barcodes, tags, _ = helpers.small_index(rnd, CUT, nbar=6, ntag=30, taglens=(4, 9))
    recs = []
    for k in range(SHORT_NREADS):
        lo, hi = (12, 20) if (k // 400) % 6 == 5 else (30, 36)
        n = rnd.randint(lo, hi)
        if rnd.random() < 0.7:
            seq = rnd.choice(barcodes) + rnd.choice(tags)
            seq = (seq + bases(rnd, max(0, n - len(seq))))[:max(n, len(seq))]
        else:
            seq = bases(rnd, n)
        recs.append("@%d\n%s\n+\n%s\n" % (k, seq, "I" * len(seq)))
    return Case("short", barcodes, tags, CUT, "".join(recs).encode())


# ---------------------------------------------------------------------------------------------------- G_hotslot
HC_SLOTS = 128


def hc_hash(cell):
    """csrc/kernel_fast2.hpp hc_hash: v_mul_u32_u24 of the cell's low 24 bits, bits 13..19 of the product."""
    return ((((cell & 0xFFFFFF) * 0x9E3779) & 0xFFFFFFFF) >> 13) & (HC_SLOTS - 1)


def colliding_cells(nrows, ncols):
    """((r1, c1), (r2, c2), (r3, c3)): the first two cells (different rows, different columns) share a slot of the hot-cell
    cache, the third has another slot."""
    by_slot = {}
    for r in range(nrows):
        for c in range(ncols):
            by_slot.setdefault(hc_hash(r * ncols + c), []).append((r, c))
    for slot in sorted(by_slot):
        cells = by_slot[slot]
        for a in cells:
            for b in cells:
                if a[0] != b[0] and a[1] != b[1]:
                    third = next(x for s in sorted(by_slot) if s != slot for x in by_slot[s] if x[0] not in (a[0], b[0]))
                    return a, b, third
    raise AssertionError("no collision")


def hot_index(seed=1):
    """12 barcodes x 60 tags of 25 to 45 bases: records of some 110 bytes."""
    rnd = random.Random("ring hot index %d" % seed)
    barcodes, tags, _ = helpers.small_index(rnd, CUT, nbar=12, ntag=60, taglens=(20, 40))
    return barcodes, tags


def hot_block(rnd, barcodes, tags, nrec, hot):
    """A clean stream (four lines, \\n, every read a hit).  hot: of every five reads three go to the two colliding cells
    in turn (A B A | B A B | ...), one to the third cell, one anywhere; else every read goes anywhere."""
    a, b, third = colliding_cells(len(barcodes), len(tags))
    out, turn = [], 0
    for k in range(nrec):
        if hot and k % 5 < 3:
            r, c = (a, b)[turn]
            turn ^= 1
        elif hot and k % 5 == 3:
            r, c = third
        else:
            r, c = rnd.randrange(len(barcodes)), rnd.randrange(len(tags))
        seq = barcodes[r] + tags[c] + bases(rnd, rnd.randint(0, 30))
        out.append("@h%d\n%s\n+\n%s\n" % (k, seq, "I" * len(seq)))
    block = "".join(out)
    if len(block) % 16 == 0:
        block += "@h\n%s\n+\nI\n" % (barcodes[third[0]] + tags[third[1]] + "A" * (len(tags[third[1]]) % 2))    # (an odd number of bytes)
    return block.encode()


@functools.lru_cache(maxsize=None)
def g_hotslot(seed=1):
    """A block of 2 000 hot records repeated to 42 tiles."""
    barcodes, tags = hot_index(seed)
    rnd = random.Random("ring hot %d" % seed)
    return Case("hotslot", barcodes, tags, CUT, repeat_block(hot_block(rnd, barcodes, tags, 2000, True), 42))


HOT_LONG_PARTS = (26, 8, 6)         # MB: uniform, hot, uniform
HC_AGE_PASSES, HC_REST, PASS_LINES = 64, 15, 64             # csrc/kernel_fast2.hpp, kernel_fast4.hpp
HC_OFF_BELOW = HC_AGE_PASSES * 45 // 32                     # a period with fewer cache hits than this switches the cache off (90)
HOT_LONG_UNIFORM_READS = 12000


def ageing_periods(nreads, consumers=3):
    """Ageing periods every consumer lives through while the workgroup matches nreads lines, evenly shared."""
    return nreads / float(consumers * PASS_LINES * HC_AGE_PASSES)


def cells_of(case, data):
    """The matrix cell (row * columns + column) of every read of a clean stream in which every read hits, in read order."""
    by_len = {}
    for r, b in enumerate(case.barcodes):
        by_len.setdefault(len(b), {})[b] = r
    tag_len = {}
    for c, t in enumerate(case.tags):
        tag_len.setdefault(len(t), {})[t] = c
    out = []
    for seq in data.decode().split("\n")[1::4]:
        # (the barcodes are prefix-free together with the site the tags begin with)
        r, n = next((d[seq[:n]], n) for n, d in by_len.items() if seq[:n] in d and seq[n:n + len(CUT)] == CUT)
        c = next(d[seq[n:n + m]] for m, d in tag_len.items() if seq[n:n + m] in d)
        out.append(r * len(case.tags) + c)
    return out


def hc_model(cells, consumers=3, on=True):
    """hc_commit, the hit count beside it and the ageing step of k_fast4's consumers (csrc/kernel_fast2.hpp,
    kernel_fast4.hpp) restated: the reads go to the consumers in passes of 64 lines, in turn; every lane of a pass sees the
    slots as the pass found them, the lanes whose cell is cached count there (a hit), of the others that find a slot
    with a count of at most 1 one takes it (the last lane here; which one is the hardware's choice), the rest count with
    plain atomics; after 64 passes the cache is written out and cleared.  Returns, per consumer, the cache hits of each
    full period -- what the kernel holds against HC_OFF_BELOW.  The cache is taken as on throughout (hot_cache = 2): the
    numbers say whether a period WOULD switch it off."""
    hits = [[] for _ in range(consumers)]
    slots = [dict() for _ in range(consumers)]              # slot -> [cell, count]
    cur = [0] * consumers
    aged = [0] * consumers
    for p in range(len(cells) // PASS_LINES):
        w = p % consumers
        S = slots[w]
        lanes = cells[p * PASS_LINES:(p + 1) * PASS_LINES]
        seen = {h: list(e) for h, e in S.items()}          # what every lane reads before any lane writes
        taker = {}
        for lane, cell in enumerate(lanes):
            h = hc_hash(cell)
            e = seen.get(h)
            if e is not None and e[0] == cell:
                cur[w] += 1
                S[h][1] += 1
            elif e is None or e[1] <= 1:
                taker[h] = cell
        for h, cell in taker.items():
            S[h] = [cell, 1]
        aged[w] += 1
        if aged[w] == HC_AGE_PASSES:
            hits[w].append(cur[w])
            cur[w], aged[w] = 0, 0
            S.clear()
    return hits


def hot_long_index(seed=1):
    """96 barcodes x 200 tags of 25 to 45 bases, 19 200 cells: 150 to a slot of the cache, so that a stream that goes anywhere
    hardly ever finds its cell cached (with g_hotslot's 720 cells a fifth of the commits do, and no cache ever rests)."""
    rnd = random.Random("ring hot long index %d" % seed)
    barcodes, tags, _ = helpers.small_index(rnd, CUT, nbar=96, ntag=200, taglens=(20, 40))
    return barcodes, tags


@functools.lru_cache(maxsize=None)
def hot_long_blocks(seed=1):
    barcodes, tags = hot_long_index(seed)
    rnd = random.Random("ring hot long %d" % seed)
    return hot_block(rnd, barcodes, tags, HOT_LONG_UNIFORM_READS, False), hot_block(rnd, barcodes, tags, 3000, True)


@functools.lru_cache(maxsize=None)
def g_hotslot_long(seed=1):
    """(case, reads of its three parts).  About 40 MB: a uniform block x a, the hot block x b, the uniform block x c.  With
    max_grid = 1 and thirteen producers three consumers take 64 lines a pass: an ageing period of 64 passes is 12 288 of the
    workgroup's reads.  In the first part a consumer's cache sees far fewer than HC_OFF_BELOW hits a period (hc_model;
    tests/test_ring.py): it is switched off after its first period, rests HC_REST periods and comes back; the hot part
    gives it more than a thousand hits a period, both colliding cells fighting for their slot; the last part switches it
    off again."""
    barcodes, tags = hot_long_index(seed)
    uni, hot = hot_long_blocks(seed)
    reps = [-(-mb * (1 << 20) // len(blk)) for mb, blk in zip(HOT_LONG_PARTS, (uni, hot, uni))]
    data = uni * reps[0] + hot * reps[1] + uni * reps[2]
    reads = tuple(blk.count(b"\n") // 4 * r for blk, r in zip((uni, hot, uni), reps))
    return Case("hotslot long", barcodes, tags, CUT, data), reads


# ---------------------------------------------------------------------------------------------------- byte sweeps
SWEEP_TILES = 40
SWEEP_TILE = 17                     # with max_grid = 1 its slot (17 mod 5) has been used three times before


@functools.lru_cache(maxsize=None)
def sweep_index(seed=1):
    rnd = random.Random("ring sweep %d" % seed)
    barcodes, tags, _ = helpers.small_index(rnd, CUT)
    return barcodes, tags


def clean_records(rnd, barcodes, tags, nbytes, nl="\n", tag="c"):
    """Clean four-line records (two in three a hit), at least nbytes of them."""
    out, n, k = [], 0, 0
    while n < nbytes:
        seq = rnd.choice(barcodes) + (rnd.choice(tags) if rnd.random() < 0.67 else CUT) + bases(rnd, rnd.randint(0, 30))
        out.append("@%s%d%s%s%s+%s%s%s" % (tag, k, nl, seq, nl, nl, "I" * len(seq), nl))
        n += len(out[-1])
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def sweep_base(seed=1):
    """(records in front of the swept spot -- they end some 600 to 900 bytes before tile SWEEP_TILE's end or start, see
    the callers --, the records behind): a clean stream of SWEEP_TILES tiles in all."""
    barcodes, tags = sweep_index(seed)
    rnd = random.Random("ring sweep base %d" % seed)
    return tuple(clean_records(rnd, barcodes, tags, SWEEP_TILES * TILE))


@functools.lru_cache(maxsize=None)
def _sweep_ends(seed):
    ends, n = [], 0
    for r in sweep_base(seed):
        n += len(r)
        ends.append(n)
    return ends


@functools.lru_cache(maxsize=64)
def _split_count(seed, k):
    recs = sweep_base(seed)
    return "".join(recs[:k]), "".join(recs[k:])


def _split_at(seed, nbytes):
    """(the base's whole records that fit into nbytes, the other records), both joined."""
    return _split_count(seed, bisect.bisect_right(_sweep_ends(seed), nbytes))


def _assemble(front, spot, rest):
    data = (front + spot + rest).encode("latin-1")
    return data[:SWEEP_TILES * TILE + 4321]


HI_SPAN = (TILE - 2, TILE + HALO_MAX + 8)       # offsets behind tile SWEEP_TILE's start: its last bytes, the whole halo and beyond


def hi_offsets():
    return range(HI_SPAN[0], HI_SPAN[1] + 1)


@functools.lru_cache(maxsize=None)
def _hi_frame(in_sequence, seed=1):
    """The buffer with one line -- a header, or a sequence (barcode + tag + bases) -- that covers HI_SPAN of tile SWEEP_TILE
    with 20 bytes to spare on either side: (bytes, offset of tile SWEEP_TILE's start)."""
    barcodes, tags = sweep_index(seed)
    t0 = SWEEP_TILE * TILE
    front, rest = _split_at(seed, t0 + HI_SPAN[0] - 400)
    rnd = random.Random("ring hi %d %d" % (in_sequence, seed))
    span = HI_SPAN[1] - HI_SPAN[0] + 1
    if in_sequence:
        # the line starts 20 bytes in front of the span: its barcode and tag lie across the tile's end, in the halo
        start = t0 + HI_SPAN[0] - 20
        head = "@seq\n"
        pad = start - len(head) - len(front)
        fseq = barcodes[3] + tags[3]
        filler = "@" + "p" * (pad - 2 * len(fseq) - 6) + "\n" + fseq + "\n+\n" + "I" * len(fseq) + "\n"
        seq = barcodes[0] + tags[0]
        seq += bases(rnd, t0 + HI_SPAN[1] + 20 - start - len(seq))
        spot = filler + head + seq + "\n+\n" + "I" * 10 + "\n"
        assert len(front) + len(filler) + len(head) == start
    else:
        hdr = "@" + "h" * (t0 + HI_SPAN[1] + 20 - len(front) - 1)
        seq = barcodes[1] + tags[1] + "ACGT"
        spot = hdr + "\n" + seq + "\n+\n" + "I" * len(seq) + "\n"
        start = len(front)
    assert start + 20 <= t0 + HI_SPAN[0] and span > HALO_MAX and len(hdr if not in_sequence else seq) > span + 20
    return _assemble(front, spot, rest), t0


def hi_case(in_sequence, off, seed=1):
    """0xE9 at offset `off` behind tile SWEEP_TILE's start, inside a header line or inside a sequence line."""
    data, t0 = _hi_frame(bool(in_sequence), seed)
    b = bytearray(data)
    assert b[t0 + off] in (b"h"[0],) + tuple(b"ACGT")
    b[t0 + off] = 0xE9
    barcodes, tags = sweep_index(seed)
    return Case("high byte in a %s at %d" % ("sequence" if in_sequence else "header", off), barcodes, tags, CUT, bytes(b))


# offsets inside tile SWEEP_TILE: the end of a producer's quarter; the end of a lane's 96 bytes of masks (phase B); the end
# of a 16-byte chunk that is neither
CRLF_BOUNDARIES = {"quarter": QUARTER, "lane span": 2 * QUARTER + 37 * 96, "chunk": QUARTER + 5 * 96 + 32}
CRLF_STEPS = 40


def crlf_case(boundary, step, lone_cr, seed=1):
    """A record whose lines end in \\r\\n -- or in a lone \\r, the sequence's first base behind it -- slid byte by byte (step
    0 .. CRLF_STEPS - 1) across a boundary inside tile SWEEP_TILE: the \\r that ends the header lies at boundary -
    CRLF_STEPS // 2 + step - 1, the last byte in front of the boundary at step CRLF_STEPS // 2 (the pair is split there,
    or the base behind the lone \\r is the boundary's first byte); the sequence line and the record's other terminators
    follow across it.  Returns (case, offset of that \\r)."""
    barcodes, tags = sweep_index(seed)
    assert CRLF_BOUNDARIES["quarter"] % QUARTER == 0 and CRLF_BOUNDARIES["lane span"] % 96 == 0 and CRLF_BOUNDARIES["lane span"] % QUARTER
    assert CRLF_BOUNDARIES["chunk"] % 16 == 0 and CRLF_BOUNDARIES["chunk"] % 96 != 0 and CRLF_BOUNDARIES["chunk"] % 1024 != 0
    target = SWEEP_TILE * TILE + CRLF_BOUNDARIES[boundary] - CRLF_STEPS // 2 + step - 1
    nl = "\r" if lone_cr else "\r\n"
    seq = barcodes[2] + tags[2] + "ACGTAC"
    head = "@cr"
    front, rest = _split_at(seed, target - len(head) - 300)
    pad = target - len(head) - len(front)
    # a clean record of exactly `pad` bytes in front (its header takes up the slack)
    fseq = barcodes[3] + tags[3]
    filler = "@" + "p" * (pad - 2 * len(fseq) - 6) + "\n" + fseq + "\n+\n" + "I" * len(fseq) + "\n"
    assert len(filler) == pad
    spot = filler + head + nl + seq + nl + "+" + nl + "I" * len(seq) + nl
    data = _assemble(front, spot, rest)
    assert data[target] == 0x0D and data[target - 1] == ord("r")
    assert data[target + 1] == (ord(seq[0]) if lone_cr else 0x0A)
    return Case("%s at the %s boundary, step %d" % ("\\r" if lone_cr else "\\r\\n", boundary, step), barcodes, tags, CUT, data), target


CRQ_TILES = 42


@functools.lru_cache(maxsize=None)
def g_cr_at_quarter_ends(lone_cr=False, seed=1):
    """Clean records with \\r\\n terminators (lone_cr: \\r alone) in which, in front of every quarter's end, a header is padded
    so that its \\r is the quarter's last byte: the \\n of the pair (or the read's first base) is the next quarter's first byte,
    another producer's -- or the halo's, or the next tile's.  The one-off of crlf_case at every quarter of every tile."""
    barcodes, tags = sweep_index(seed)
    rnd = random.Random("ring crq %d %d" % (lone_cr, seed))
    nl = "\r" if lone_cr else "\r\n"
    out, pos, k = [], 0, 0
    while pos < CRQ_TILES * TILE:
        end = (pos // QUARTER + 1) * QUARTER
        while end - pos > 600:
            out.append(clean_records(rnd, barcodes, tags, 1, nl=nl, tag="q%d_" % k)[0])
            pos += len(out[-1])
            k += 1
        seq = rnd.choice(barcodes) + rnd.choice(tags) + bases(rnd, rnd.randint(0, 30))
        out.append("@" + "p" * (end - 2 - pos) + nl + seq + nl + "+" + nl + "I" * len(seq) + nl)
        pos += len(out[-1])
    return Case("cr at quarter ends" + (" (lone)" if lone_cr else ""), barcodes, tags, CUT, "".join(out).encode())


HALO_BYTE_AT = 3                    # bytes behind tile SWEEP_TILE's end: inside its halo, tile SWEEP_TILE + 1's fourth byte


@functools.lru_cache(maxsize=None)
def g_qual_high_byte_in_halo(seed=1):
    """g_qual's records with one whose quality line -- barcode + a tag that ends in A -- starts in tile SWEEP_TILE's last
    bytes and has 0xE9 in place of the tag's last base, HALO_BYTE_AT bytes behind the tile's end.  Legal: only sequence
    lines must be ASCII.  Voted for (run = 1), the line is packed from the tile's halo; the forms for ASCII bytes read
    0xE9 as a base -- as A -- and would count the tag, and the take-back, which looks at the bytes exactly, would find
    nothing to subtract: a tile whose halo holds such a byte must not be matched in the main pass."""
    base = g_qual(seed)
    barcodes, tags = base.barcodes, base.tags
    rnd = random.Random("ring qual halo %d" % seed)
    recs = qual_records(rnd, barcodes, tags, 0, QUAL_NREC)
    end = (SWEEP_TILE + 1) * TILE
    pos, k = 0, 0
    while pos + len(recs[k]) <= end - 700:
        pos += len(recs[k])
        k += 1
    bar, tag = barcodes[0], next(t for t in tags if t.endswith("A"))
    qread = bar + tag[:-1] + "\xe9" + bases(rnd, 12)
    read = " " + rnd.choice(barcodes) + rnd.choice(tags)
    read += bases(rnd, max(0, len(qread) - len(read)))
    qread += bases(rnd, len(read) - len(qread))
    start = end + HALO_BYTE_AT - (len(bar) + len(tag) - 1)              # where the quality line begins
    hdr = "@r" + "x" * (start - pos - (len(read) + 4) - 2)
    spot = "%s\n%s\n+\n%s\n" % (hdr, read, qread)
    data = ("".join(recs[:k]) + spot + "".join(recs[k:])).encode("latin-1")
    assert data[end + HALO_BYTE_AT] == 0xE9 and data[start - 1] == 0x0A and data[start:start + len(bar)] == bar.encode() and start < end
    return Case("qual, high byte in a halo", barcodes, tags, CUT, data)
