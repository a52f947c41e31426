"""tests/fused_cases.py without a GPU: from the bytes and the oracles alone, every input can catch a wrong line index.

The splitter writes the decision of line `line` (1 mod 4) to out[line >> 2].  Its line index of a tile's first line comes
from the per-tile terminator counts in front of the tile; td_count_and_split_device takes those from the count kernels'
tile records.  A count that is wrong in one tile moves the index of every line behind that tile's end.  shift_model
restates "slot = sequence-line ordinal, decision = decision of that line" and adds +1, -1, +4 and -4 to the index of
every line behind every tile boundary (24 576 and 16 384 bytes) of every input; the output, sentinels behind the last
slot included, must differ from the expected one -- else the input could not tell.  Nothing is run on a GPU for this:
a wrong index moves stores.
"""
import numpy as np
import pytest

import fused_cases as fc
import ring_cases as rc
import splitter_edge_cases as ec

ALL = list(fc.cases())


def test_the_inputs_are_all_there():
    names = set(ALL)
    assert {"edge:" + n for n, c in ec.cases().items() if c.error is None} <= names
    assert not any("nonascii" in n for n in names)
    ring = {n.split(":")[1] for n in names if n.startswith("ring:")}
    assert ring == {"dirty", "qual", "sparse", "short", "cr-quarter-ends", "cr-quarter-ends-lone", "qual-high-byte-in-halo",
                    "crlf-chunk", "crlf-lane-span", "crlf-quarter", "high-byte-header-first", "high-byte-header-last"}
    assert len(rc.CRLF_BOUNDARIES) == 3
    for c in fc.cases().values():
        assert 1 <= len(c.tags) <= fc.MAX_TAGS and max(len(t) - len(c.set.cutsite) for t in c.tags) <= 70        # W <= 3
        if c.origin != "ring":
            assert max(len(t) - len(c.set.cutsite) for t in c.tags) <= fc.TAG_BASES
        assert fc.sequence_lines_are_ascii(c.data), c.name
    # every ring case's splitter fits k_split2's compact form: the default route takes the count pass's records
    assert all(c.set.compact for c in fc.ring_cases().values())
    assert {c.set.compact for c in fc.edge_cases().values()} == {True, False}


def barcode_lines(table):
    """Indices of the sequence lines whose decision names a barcode."""
    k = np.arange(table.nlines)
    return k[((k & 3) == 1) & (table.dec[:, 0] >= 0)]


@pytest.mark.parametrize("name", ALL)
def test_a_wrong_line_index_shows(name):
    case = fc.cases()[name]
    table = fc.line_table(name)
    want = fc.expected_decisions(case)
    base = table.slots()
    # the restatement, unshifted, is the oracle's loop
    assert (base[:table.nseq] == want).all() and (base[table.nseq:] == fc.SENTINEL).all() and len(want) == table.nseq
    with_bar = barcode_lines(table)
    nothing, checked = [], 0
    for tile in fc.TILES:
        last_tile_start = (len(case.data) - 1) // tile * tile
        for b in fc.boundaries(case.data, tile):
            L = table.first_line_behind(b)
            seq_behind = any(k & 3 == 1 for k in range(L, min(L + 4, table.nlines)))
            changed = {s: not np.array_equal(table.slots(L, s), base) for s in fc.SHIFTS}
            if seq_behind:
                checked += 1
                # a slot too early or too late: the first slot behind the boundary, or the last, keeps its sentinel
                assert changed[4] and changed[-4], (name, tile, b)
            if len(with_bar) and with_bar[-1] >= L:
                # a header or a "+" line is taken for the read
                assert changed[1] and changed[-1], (name, tile, b)
            if not any(changed.values()):
                nothing.append((tile, b))
                # only where no sequence line follows at all
                assert not seq_behind and b == last_tile_start, (name, tile, b)
    if nothing:
        print(" [%s: no shift shows at %r: no sequence line behind] " % (name, nothing), end="")
    if case.origin != "ring":
        assert not nothing, (name, nothing)
    print(" [%s: %d boundaries with a sequence line behind, each shift shows at each] " % (name, checked), end="")


def tiles_of(offsets, tile):
    return sorted({o // tile for o in offsets})


@pytest.mark.parametrize("name", ALL)
def test_the_count_index_counts_where_it_matters(name):
    """The expected matrix is non-zero and the counted reads lie in at least three tiles, the last one among them -- as far
    as the buffer has sequence lines with a barcode there at all: the read cases of the splitter edge suite keep their
    reads between two header lines of one and two tiles, and the buffers cut to a length are a tile or two."""
    case = fc.cases()[name]
    m, st = fc.expected_counts(case)
    offs = fc.counted_read_offsets(case)
    assert len(offs) == int(m.sum()) == st["tag"]
    table = fc.line_table(name)
    starts = [0] + table.ends
    bar_offs = [starts[k] for k in barcode_lines(table)]
    if not bar_offs:
        assert name == "edge:length-1"
        return
    assert m.sum() > 0, name
    for tile in fc.TILES:
        have, could = tiles_of(offs, tile), tiles_of(bar_offs, tile)
        assert len(have) >= min(3, len(could)), (name, tile, have, could)
        assert have[-1] == could[-1], (name, tile)
        if case.origin != "edge":
            assert len(have) >= 3 and have[-1] == (len(case.data) - 1) // tile, (name, tile)
    if case.origin != "edge":
        d = fc.expected_decisions(case)
        assert ((d[:, 0] >= 0).sum() >= 1) and ((d[:, 0] >= 0) & (d[:, 1] != 999)).sum() >= 1, name


def test_the_tail_behind_g_dirty_leaves_its_tiles_alone():
    base = rc.g_dirty()
    case = fc.cases()["ring:dirty"]
    assert case.data.startswith(base.data) and 0 < len(case.data) - len(base.data) < 400
    a, b = rc.tile_classes(base.data), rc.tile_classes(case.data)
    assert len(a) == len(b) and a[:-1] == b[:-1] and not b[-1]["hi"] and not b[-1]["over"]
    assert 8 <= b[-1]["nstarts"] - a[-1]["nstarts"] <= 12
    # tests/test_ring.py's asserts of the generator, on the bytes with the tail
    d = case.data
    assert d.count(b"\r\n") > 1000 and d.count(b"\n") - d.count(b"\r\n") > 1000 and d.count(b"\r") - d.count(b"\r\n") > 1000
    assert max(len(x) for x in d.splitlines()) > 500
    assert sum(1 for t in rc.interior(len(b)) if b[t]["nstarts"] >= 64) >= 30
    assert 40 <= rc.ntiles(d) <= 64
    # without it no read of the last tile is counted
    plain = fc.Case("plain dirty", case.set, case.tags, base.data, None, "ring")
    assert (len(base.data) - 1) // fc.TILE2 not in tiles_of(fc.counted_read_offsets(plain), fc.TILE2)


def test_short_records_overflow_every_list_and_take_a_far_bound():
    case = fc.short_records()
    cl = rc.tile_classes(case.data)
    assert len(cl) == fc.SHORT_TILES
    q = rc.QUARTER
    for t in range(len(cl) - 1):
        for k in range(4):
            chunk = case.data[t * fc.TILE2 + k * q:t * fc.TILE2 + (k + 1) * q]
            assert chunk.count(b"\n") > rc.LIST_CAP
    reads = fc.expected_counts(case)[1]["reads"]
    far = reads * 3 // 4
    assert fc.bound_is_far(len(case.data), far) and not fc.bound_is_far(len(case.data), 3)
    m, st = fc.expected_counts(case, maxreads=far)
    assert st["reads"] == far and 0 < m.sum() < fc.expected_counts(case)[0].sum()


@pytest.mark.parametrize("name", ["ring:qual", "ring:short", "edge:geometry-24576", "edge:geometry-16384"])
def test_a_bound_inside_the_other_inputs_is_a_near_one(name):
    """Their lines are 18 bytes and longer: a bound at three quarters of the reads lies fewer than nbytes / 16 lines behind the
    start, so launch_count counts with the exact kernel and the prefix is counted from the bytes."""
    case = fc.cases()[name]
    reads = fc.expected_counts(case)[1]["reads"]
    assert not fc.bound_is_far(len(case.data), reads * 3 // 4)
    assert fc.bound_is_far(len(case.data), 10 ** 9)


# ---------------------------------------------------------------------------------------------------- more than 8 192 tiles
@pytest.mark.parametrize("tile", fc.TILES)
def test_line_prefix_big_filler(tile):
    """The filler in front of tile SCAN_ROUND: whole records that decide (-1, 999) and count nothing; the terminators inside the
    first SCAN_ROUND tiles are no multiple of 4, so a carry lost between k_scan_tiles' rounds changes the line phase
    behind it as well as the slot."""
    block = fc.big_block()
    case = fc.cases()["edge:geometry-%d" % tile]
    blk = fc.Case("big block", case.set, case.tags, block, None, "extra")
    m, st = fc.expected_counts(blk)
    assert m.sum() == 0 and st["barcut"] == 0 and st["reads"] == 3 and st["lines"] == 12
    assert (fc.expected_decisions(blk) == np.array([fc.NO_BARCODE] * 3)).all()
    assert fc.big_terminators_in_first_round(tile) % 4 != 0
    # the filler as it is built (one tile size only: 134 MB of bytes)
    if tile == fc.TILE1:
        data, nseq = fc.big_filler(tile)
        assert len(data) == fc.BIG_FILLER_TILES * tile and data.count(b"\n") == 4 * nseq and b"\r" not in data
        assert data[-1:] == b"\n" and data.count(b"\n", 0, fc.SCAN_ROUND * tile) == fc.big_terminators_in_first_round(tile)
        tail = data[-600:]
        assert fc.decide(case.set, tail.split(b"\n")[-4]) == fc.NO_BARCODE
