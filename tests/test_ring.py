"""The generators of tests/ring_cases.py without a GPU: from the bytes and the C oracle alone, each reaches the regime
tests/test_ring_gpu.py runs it for -- the sizes, the quality lines that read as reads, the classes of tiles, the
overflowing and the ordinary quarters, the colliding cells and their shares, where the swept bytes lie."""
import numpy as np
import pytest

import ring_cases as rc
from oracle import tagdigger_oracle as orc

TILE = rc.TILE


line_count = rc.line_count


def test_generators_are_seeded():
    for fn in (rc.g_dirty, rc.g_qual, rc.g_sparse, rc.g_short, rc.g_hotslot, rc.sweep_base):
        assert fn.__wrapped__() == fn()
    assert rc.g_qual.__wrapped__(1, True) == rc.g_qual(1, True) and rc.g_qual(1, True) != rc.g_qual()
    assert rc.g_dirty(2).data != rc.g_dirty().data


@pytest.mark.parametrize("gen", [rc.g_dirty, rc.g_qual, rc.g_sparse, rc.g_hotslot], ids=lambda g: g.__name__)
def test_forty_to_sixty_four_tiles(gen):
    case = gen()
    assert 40 <= rc.ntiles(case.data) <= 64
    m, st = rc.expected(case)
    assert st["lines"] == line_count(case.data) and st["reads"] >= st["barcut"] >= st["tag"] == m.sum() > 200


def test_terminator_ends():
    data = b"a\nb\r\nc\rd\r\r\n\n\re"
    assert rc.terminator_ends(data) == [2, 5, 7, 9, 11, 12, 13] and line_count(data) == 7
    assert rc.terminator_ends(b"abc") == [] and rc.terminator_ends(b"\r") == [1]


def test_dirty():
    case = rc.g_dirty()
    d = case.data
    assert d.count(b"\r\n") > 1000 and d.count(b"\n") - d.count(b"\r\n") > 1000 and d.count(b"\r") - d.count(b"\r\n") > 1000
    assert max(len(x) for x in d.splitlines()) > 500                        # long_lines
    block = d[:d.index(b"@r0", 1)]
    assert len(block) % 16 != 0 and d == block * (len(d) // len(block)) and len(d) // len(block) >= 4
    # the shifts that stay: the block's copies do not all begin at the same line phase
    assert line_count(block) % 4 != 0
    # every tile of the interior is an ordinary tile or one of the kinds the producers flag
    cl = rc.tile_classes(d)
    assert sum(1 for t in rc.interior(len(cl)) if cl[t]["nstarts"] >= 64) >= 30


def test_qual():
    """want.sum() == nrec; read under first_line = 2 (the quality lines as the sequences) more than half of the records
    hit, and that matrix differs from the true one in more than 100 cells: a take-back that went to the wrong cell, or
    missed lines, cannot cancel out."""
    case = rc.g_qual()
    want, st = rc.expected(case)
    assert want.sum() == rc.QUAL_NREC == st["reads"] == st["tag"]
    wrong, wst = rc.expected(case, first_line=2)
    assert wrong.sum() > 0.5 * rc.QUAL_NREC
    assert (wrong != want).sum() > 100
    lines = case.data.split(b"\n")
    assert lines[-1] == b"" and len(lines) == 4 * rc.QUAL_NREC + 1
    for k in range(0, 4 * rc.QUAL_NREC, 4):
        assert lines[k].startswith(b"@r") and lines[k + 1][:1] == b" " and lines[k + 2] == b"+"
        assert len(lines[k + 3]) == len(lines[k + 1]) and set(lines[k + 3]) <= set(b"ACGT") and set(lines[k + 1][1:]) <= set(b"ACGT")
    # the only lines whose first eight bytes are bases are quality lines: every interior tile has them, none has another
    cl = rc.tile_classes(case.data)
    assert all(cl[t]["nstarts"] >= 256 and not cl[t]["hi"] and not cl[t]["over"] for t in rc.interior(len(cl)))


def test_qual_with_a_shift():
    plain, case = rc.g_qual(), rc.g_qual(1, True)
    at = case.data.index(b"\n\n\n")
    assert at // TILE == rc.QUAL_SHIFT_TILE and 1000 < at % TILE < TILE - 1000
    assert case.data[:at + 1] == plain.data[:at + 1] and case.data[at + 3:] == plain.data[at + 1:]
    want, st = rc.expected(case)
    head, _ = rc.expected(case, data=case.data[:at + 1])
    tail, _ = rc.expected(case, data=plain.data[at + 1:], first_line=2)
    assert (want == head + tail).all() and st["reads"] == rc.QUAL_NREC + 1      # (the quality line of the last record: no read)
    assert tail.sum() > 0.5 * (rc.QUAL_NREC - head.sum())


def test_qual_behind_a_clean_head():
    plain, case = rc.g_qual(), rc.g_qual_behind_clean_head()
    assert case.data.endswith(plain.data) and 40 <= rc.ntiles(case.data) <= 64
    head = case.data[:-len(plain.data)]
    assert rc.QUAL_HEAD_TILES * TILE < len(head) < (rc.QUAL_HEAD_TILES + 1) * TILE and rc.line_count(head) % 4 == 0 and b"\r" not in head
    lines = head.split(b"\n")
    assert all(set(lines[k]) <= set(b"ACGT") and len(lines[k]) >= 8 for k in range(1, len(lines) - 1, 4))
    assert all(not set(lines[k][:8]) <= set(b"ACGT") for k in range(len(lines) - 1) if k % 4 != 1)
    want, st = rc.expected(case)
    hwant, hst = rc.expected(case, data=head)
    assert (want == hwant + rc.expected(plain)[0]).all() and st["reads"] == hst["reads"] + rc.QUAL_NREC


def test_sparse():
    """Every tile classified from the bytes alone; at least three interior tiles of each kind, and ordinary ones between."""
    case = rc.g_sparse()
    cl = rc.tile_classes(case.data)
    inner = list(rc.interior(len(cl)))
    hi = [t for t in inner if cl[t]["hi"]]
    over = [t for t in inner if cl[t]["over"]]
    noterm = [t for t in inner if cl[t]["noterm"]]
    few = [t for t in inner if 0 < cl[t]["nstarts"] < 13 and not cl[t]["hi"]]
    assert min(len(hi), len(over), len(noterm), len(few)) >= 3, (hi, over, noterm, few)
    odd = set(hi) | set(over) | set(noterm)
    ordinary = [t for t in inner if t not in odd]
    assert len(ordinary) >= 10
    # ... between them: the irregular tiles do not lie in one heap at either end
    assert sum(1 for t in ordinary if min(odd) < t < max(odd)) >= 10
    lines = case.data.splitlines()
    assert sum(1 for x in lines if 30000 <= len(x) <= 60010) >= 3
    assert sum(1 for k, x in enumerate(lines) if k % 4 == 0 and not x.isascii()) >= 3
    assert all(x.isascii() for k, x in enumerate(lines) if k % 4 == 1)
    ordinary_records = [len(lines[k]) + len(lines[k + 1]) + len(lines[k + 2]) + len(lines[k + 3]) + 4 for k in range(0, len(lines), 4)
                        if 1000 <= len(lines[k + 1]) < 4000 and len(lines[k]) < 100]
    assert len(ordinary_records) > 200 and 2000 <= min(ordinary_records) and max(ordinary_records) <= 6200
    # a quarter's list overflows in at least three separate stretches
    assert sum(1 for a, b in zip(over, over[1:] + [10 ** 9]) if b - a > 2) >= 3
    want, st = rc.expected(case)
    assert want.sum() == st["tag"] >= len(ordinary_records)


def test_short():
    case = rc.g_short()
    d = case.data
    want, st = rc.expected(case)
    assert st["reads"] == rc.SHORT_NREADS >= 60000 and st["lines"] == 4 * rc.SHORT_NREADS == d.count(b"\n")
    assert 17.0 <= len(d) / float(st["lines"]) <= 20.0
    lines = d.split(b"\n")
    seqlens = [len(lines[k]) for k in range(1, len(lines) - 1, 4)]
    assert min(seqlens) >= 12 and max(seqlens) <= 36
    assert all(4 <= len(t) - len(rc.CUT) <= 9 for t in case.tags)
    cl = rc.tile_classes(d)
    inner = list(rc.interior(len(cl)))
    assert sum(1 for t in inner if cl[t]["over"]) >= 10 and sum(1 for t in inner if not cl[t]["over"]) >= 10
    assert not any(cl[t]["hi"] or cl[t]["noterm"] for t in inner)
    # the progress window's boundary: read 50 000's sequence line starts in an interior tile
    at = sum(len(x) + 1 for x in lines[:4 * rc.WINDOW + 1])
    assert d[at - 1:at] == b"\n" and (at // TILE) in inner
    assert st["tag"] > 0.5 * st["reads"]


def test_hotslot():
    case = rc.g_hotslot()
    nrows, ncols = len(case.barcodes), len(case.tags)
    a, b, third = rc.colliding_cells(nrows, ncols)
    cell = lambda rc_: rc_[0] * ncols + rc_[1]
    assert a != b and rc.hc_hash(cell(a)) == rc.hc_hash(cell(b)) != rc.hc_hash(cell(third))
    # the hash restated once more, in wide arithmetic
    for c in (cell(a), cell(b), cell(third), 0xFFFFFF, 12345):
        assert rc.hc_hash(c) == (((c % (1 << 24)) * 0x9E3779) % (1 << 32)) // (1 << 13) % 128
    want, st = rc.expected(case)
    n = st["reads"]
    assert st["tag"] == n == want.sum()
    assert want[a] + want[b] >= 0.6 * n and abs(int(want[a]) - int(want[b])) <= n // 1000 + 1
    assert 0.2 * n <= want[third] < 0.21 * n
    assert (want > 0).sum() > 0.3 * nrows * ncols                    # the last fifth (400 reads of the block) goes anywhere
    # the two cells in turn, read by read
    seqs = case.data.split(b"\n")[1::4][:2000]
    hot = [s for s in seqs if any(s.startswith((case.barcodes[r] + case.tags[c]).encode()) for r, c in (a, b))]
    first = (case.barcodes[a[0]] + case.tags[a[1]]).encode()
    flips = sum(1 for x, y in zip(hot, hot[1:]) if x.startswith(first) != y.startswith(first))
    assert len(hot) >= 1200 and flips >= len(hot) - 1 - 2 * 2000 // 5 // 20       # (a random read may be one of them too)


def test_hc_model():
    """The restated cache on streams whose hits can be counted by hand."""
    one = [5] * (64 * 64)                                   # one cell, one consumer: the first pass takes the slot, 63 passes hit
    assert rc.hc_model(one, consumers=1) == [[63 * 64]]
    a, b, _ = rc.colliding_cells(12, 60)
    ca, cb = a[0] * 60 + a[1], b[0] * 60 + b[1]
    # two cells of one slot in turn: the slot's owner (the pass's last taker) hits 32 times a pass from the second pass on
    assert rc.hc_model([ca, cb] * (32 * 64), consumers=1) == [[63 * 32]]
    # 4 096 different cells: nothing is ever cached twice
    assert rc.hc_model(list(range(64 * 64)), consumers=1) == [[0]]
    # periods are a consumer's own: three consumers need three times the reads
    assert rc.hc_model(one * 3) == [[63 * 64]] * 3 and rc.hc_model(one * 2) == [[], [], []]


def test_hotslot_long():
    """The regime from the bytes, by the restated cache: in the uniform parts every consumer's cache has far fewer hits in
    a period than the HC_OFF_BELOW that keep it on -- whatever pass the consumers' turns begin with --, in the hot part far
    more; the first part lasts longer than one period, the rest and a few more, so that a cache goes off, rests and comes
    back inside it."""
    (case, reads) = rc.g_hotslot_long()
    assert 38 << 20 <= len(case.data) <= 44 << 20
    assert len(case.barcodes) * len(case.tags) >= 6000
    pa, pb, pc = (rc.ageing_periods(n) for n in reads)
    assert pa >= 1 + rc.HC_REST + 2 and pb >= 3 and pc >= 2
    uni, hot = rc.hot_long_blocks()
    assert case.data == uni * (reads[0] // rc.HOT_LONG_UNIFORM_READS) + hot * (reads[1] // 3000) + uni * (reads[2] // rc.HOT_LONG_UNIFORM_READS)
    cu, ch = rc.cells_of(case, uni), rc.cells_of(case, hot)
    want_uni, _ = rc.expected(case, data=uni)
    assert (np.bincount(cu, minlength=want_uni.size) == want_uni.ravel()).all()          # cells_of reads the bytes as the oracle does
    assert rc.HC_OFF_BELOW == 90
    for shift in (0, 7, 64 + 3, 128 + 11):
        per = rc.hc_model((cu * 5)[shift:])
        assert all(len(h) >= 4 and max(h) < rc.HC_OFF_BELOW // 2 for h in per), (shift, per)
    per = rc.hc_model(ch * 13)
    assert all(len(h) >= 3 and min(h) > 10 * rc.HC_OFF_BELOW for h in per), per
    # g_hotslot's 720 cells would not do: a fifth of a uniform stream's commits hit, and no cache would ever rest
    small = rc.g_hotslot()
    rnd = __import__("random").Random(3)
    anywhere = [rnd.randrange(len(small.barcodes) * len(small.tags)) for _ in range(3 * 64 * 64)]
    assert min(h[0] for h in rc.hc_model(anywhere)) > 4 * rc.HC_OFF_BELOW
    want, st = rc.expected(case)
    assert st["reads"] == sum(reads) == st["tag"]
    a, b, _ = rc.colliding_cells(len(case.barcodes), len(case.tags))
    assert want[a] + want[b] >= 0.6 * reads[1]


def test_high_byte_frames():
    """One line covers the swept span -- tile 17's last two bytes, the whole halo behind it and more --; in a header the byte
    changes nothing, in a sequence line both oracles raise."""
    t0 = rc.SWEEP_TILE * TILE
    assert rc.HI_SPAN[0] == TILE - 2 and rc.HI_SPAN[1] >= TILE + 200 and rc.HALO_MAX <= 200
    for in_sequence in (False, True):
        data, tile0 = rc._hi_frame(in_sequence)
        assert tile0 == t0 and rc.ntiles(data) in (rc.SWEEP_TILES, rc.SWEEP_TILES + 1) and data.isascii()
        ends = rc.terminator_ends(data)
        lo = max(e for e in ends if e <= t0 + rc.HI_SPAN[0])
        hi = min(e for e in ends if e > t0 + rc.HI_SPAN[0])
        assert hi - 1 > t0 + rc.HI_SPAN[1]                                  # one line: no terminator inside the span
        k = ends.index(lo) + 1                                              # the line's ordinal
        assert k % 4 == (1 if in_sequence else 0)
        base, bst = rc.expected(rc.Case("", *rc.sweep_index(), rc.CUT, data))
        assert bst["tag"] > 3000
        for off in rc.hi_offsets():
            case = rc.hi_case(in_sequence, off)
            assert case.data[t0 + off] == 0xE9 and sum(1 for x in case.data[t0:t0 + 2 * TILE] if x >= 0x80) == 1
            if in_sequence:
                with pytest.raises(orc.NonAsciiSequence):
                    rc.expected(case)
            else:
                got, st = rc.expected(case)
                assert (got == base).all() and st == bst
    case = rc.hi_case(True, TILE + 5)
    with pytest.raises(orc.NonAsciiSequence):
        orc.count_bytes(case.data, case.barcodes, case.tags, case.cutsite)


@pytest.mark.parametrize("lone_cr", [False, True], ids=["crlf", "cr"])
@pytest.mark.parametrize("boundary", sorted(rc.CRLF_BOUNDARIES))
def test_crlf_slides(boundary, lone_cr):
    t0 = rc.SWEEP_TILE * TILE
    bnd = t0 + rc.CRLF_BOUNDARIES[boundary]
    seen = set()
    for step in range(rc.CRLF_STEPS):
        case, target = rc.crlf_case(boundary, step, lone_cr)
        d = case.data
        seen.add(target - bnd)
        assert d[target] == 0x0D and rc.ntiles(d) in (rc.SWEEP_TILES, rc.SWEEP_TILES + 1)
        ends = rc.terminator_ends(d)
        k = ends.index(target + (1 if lone_cr else 2))
        assert k % 4 == 0                                                   # a header's terminator: a read starts behind it
        want, st = rc.expected(case)
        assert st["lines"] == len(ends) == line_count(d)
        seq = d[ends[k]:ends[k + 1]].rstrip(b"\r\n")
        b, t = case.barcodes[2], case.tags[2]
        assert seq == (b + t + "ACGTAC").encode() and want[2, 2] >= 1
        assert d.count(b"\r") == 4
    assert seen == set(range(-rc.CRLF_STEPS // 2 - 1, rc.CRLF_STEPS // 2 - 1)) and -1 in seen


@pytest.mark.parametrize("lone_cr", [False, True], ids=["crlf", "cr"])
def test_cr_at_quarter_ends(lone_cr):
    case = rc.g_cr_at_quarter_ends(lone_cr)
    d = case.data
    assert rc.g_cr_at_quarter_ends.__wrapped__(lone_cr) == case and 40 <= rc.ntiles(d) <= 64
    ends = set(rc.terminator_ends(d))
    for q in range(1, 4 * rc.CRQ_TILES + 1):
        at = q * rc.QUARTER
        assert d[at - 1] == 0x0D and (d[at] in b"ACGT" if lone_cr else d[at] == 0x0A)
        assert (at if lone_cr else at + 1) in ends
    assert (b"\n" in d) == (not lone_cr) and d.count(b"\r") == rc.line_count(d)
    want, st = rc.expected(case)
    assert st["lines"] == rc.line_count(d) == 4 * st["reads"] and st["tag"] > 0.5 * st["reads"] > 2000


def test_qual_high_byte_in_a_halo():
    case = rc.g_qual_high_byte_in_halo()
    d = case.data
    at = (rc.SWEEP_TILE + 1) * TILE + rc.HALO_BYTE_AT
    assert d[at] == 0xE9 and sum(1 for x in d[at - 2 * TILE:at + 2 * TILE] if x >= 0x80) == 1 and rc.HALO_BYTE_AT < 16
    ends = rc.terminator_ends(d)
    k = max(i for i, e in enumerate(ends) if e <= at)               # the line's ordinal - 1
    start = ends[k]
    assert (k + 1) % 4 == 3 and (rc.SWEEP_TILE + 1) * TILE - 100 < start < (rc.SWEEP_TILE + 1) * TILE
    line = d[start:ends[k + 1] - 1]
    bar = case.barcodes[0].encode()
    tag = next(t for t in case.tags if t.endswith("A")).encode()
    assert line.startswith(bar + tag[:-1] + b"\xe9") and start + len(bar) + len(tag) - 1 == at
    want, st = rc.expected(case)                                      # legal: the byte is in a quality line
    assert want.sum() == st["reads"] == rc.QUAL_NREC + 1
    with pytest.raises(orc.NonAsciiSequence):                         # read as a sequence it is not
        rc.expected(case, first_line=2)
