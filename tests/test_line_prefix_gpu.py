"""The line prefix on its own: per-tile terminator counts (k_count_lines<4> for td_count_lines_device and the streaming
modules, <6> for k_split2's tiles, k_info_counts where td_count_and_split_device takes the count pass's records) and
their scan (k_scan_tiles), directly and at scale.

  * td_count_lines_device against the bytes' own count, at lengths around a chunk, a 16, 24 and 32 KiB tile and a few tiles,
    with "\\r\\n", "\\r", "\\n" and "\\r\\r\\n" slid byte by byte across the 16-byte chunk ends of a tile's last 64 bytes, the tile's
    end and the buffer's last byte; buffers that are terminators only.
  * the same slid terminators through td_split_device (k_count_lines<6>, prefix source 1) and the fused call (k_info_counts,
    source 2) on records of the splitter edge suite's filler reads: a count that is wrong moves every later decision.
  * more than 8 192 tiles in one launch: k_scan_tiles takes 8 192 tiles a round and carries the sum into the next one.
    A filler whose every decision is (-1, 999), one tile more than a round long, with the geometry case of the tile size
    behind it (tests/test_fused.py: the terminators of the first round are no multiple of 4, so a lost carry changes the
    line phase behind it as well as the slot).  Production buffers of tens of gigabytes always take that branch.
"""
import ctypes as C
import re

import numpy as np
import pytest

import fused_cases as fc
import splitter_edge_cases as ec
from test_fused_gpu import Resident, apply, SENTINEL, SLACK

pytestmark = pytest.mark.gpu

TERMINATOR = re.compile(rb"\r\n|\n|\r")
KINDS = {"crlf": b"\r\n", "cr": b"\r", "lf": b"\n", "crcrlf": b"\r\r\n"}
LENGTHS = [1, 15, 16, 17, 16383, 16384, 16385, 24575, 24576, 24577, 32767, 32768, 32769, 5 * 16384 + 7]


@pytest.fixture(scope="module")
def eng():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    yield e
    e.close()


def count(data):
    return len(TERMINATOR.findall(data))


def filler_bytes(n):
    """Records of the filler reads, cut to n bytes."""
    reads = [ec.expand(r) for r in ec.FILLER_READS]
    block = ec.fastq_of(reads)
    return (block * (n // len(block) + 1))[:n]


def slide_points(n, tile):
    """Offsets a terminator is slid across: the 16-byte chunk ends of every tile's last 64 bytes, the tile's end, the
    buffer's end."""
    pts = {n} | {p for p in range(n - n % 16, max(0, n - 64), -16)}          # (and of the buffer's own last 64 bytes)
    for end in range(tile, n + 1, tile):
        pts.update(end - d for d in (48, 32, 16, 0))
    return sorted(p for p in pts if 0 < p <= n)


def slid(base, term, point):
    """The buffer with `term` written over its bytes so that it ends 0 .. len(term) + 1 bytes behind `point` (cut at the
    buffer's end): wholly in front of the point, split by it at every byte, wholly behind it."""
    for end in range(point, point + len(term) + 2):
        start = end - len(term)
        if start < 0:
            continue
        b = bytearray(base)
        b[start:end] = term
        yield end, bytes(b[:len(base)])


@pytest.mark.parametrize("n", LENGTHS)
def test_count_lines_device_with_slid_terminators(eng, n):
    base = filler_bytes(n)
    d = eng.dev_alloc(n + 16)
    runs = 0
    try:
        eng.h2d(d, base)
        assert eng.count_lines_device(d, n) == count(base)
        for kind, term in KINDS.items():
            for point in slide_points(n, 16384):
                for end, data in slid(base, term, point):
                    eng.h2d(d, data)
                    got = eng.count_lines_device(d, n)
                    assert got == count(data), (n, kind, point, end, got, count(data))
                    runs += 1
    finally:
        eng.dev_free(d)
    print(" [%d bytes: %d buffers] " % (n, runs), end="")


@pytest.mark.parametrize("n", [16384, 24576, 2 * 24576 + 3])
def test_count_lines_device_terminators_only(eng, n):
    d = eng.dev_alloc(n + 16)
    try:
        for data in (b"\n" * n, b"\r" * n, (b"\r\n" * n)[:n], (b"\n\r" * n)[:n], (b"\r\r\n" * n)[:n]):
            eng.h2d(d, data)
            assert eng.count_lines_device(d, n) == count(data), (n, data[:4])
    finally:
        eng.dev_free(d)


# ---------------------------------------------------------------------------------------------------- through the splitter
SPLIT_TILES = 4                         # tile 0 is the buffer's first, tiles 2 and 3 cross its end with their halo: tile 1 is a regular one


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_slid_terminators_through_the_splitter_and_the_fused_call(eng, kind):
    """k_count_lines<6> (td_split_device with k_split2) and k_info_counts (the fused call, k_fast4's records) under the same
    slid terminators, across the ends of tile 0 and of tile 1 and the buffer's last byte; expected decisions:
    splitter_edge_cases.expected."""
    n = SPLIT_TILES * fc.TILE2 - 1000
    base = filler_bytes(n)
    tags = fc.choose_tags(ec.SETS["hall"], base)
    points = [p for p in slide_points(n, fc.TILE2) if p <= 2 * fc.TILE2 or p == n]
    runs = 0
    try:
        for point in points:
            for end, data in slid(base, KINDS[kind], point):
                if not fc.sequence_lines_are_ascii(data):
                    continue
                case = fc.adhoc("slid %s %d %d" % (kind, point, end), data, tags=tags)
                want = np.array(ec.expected("hall", data), dtype=np.int32).reshape(-1, 2)
                m, st = fc.expected_counts(case)
                with Resident(eng, case) as r:
                    apply(eng, {})
                    eng.reset()
                    res, terms = r.call(False)
                    assert r.source == 1 and eng.split_kernel_in_use() == 2
                    r.check_decisions(res, terms, want, (kind, point, end, "td_split_device"))
                    r.check(want, m, st, 2, (kind, point, end, "fused"))
                    apply(eng, dict(max_grid=1))
                    r.check(want, m, st, 2, (kind, point, end, "fused, one workgroup"))
                runs += 1
    finally:
        apply(eng, {})
    print(" [%s: %d buffers, prefix sources 1 and 2] " % (kind, runs), end="")


# ---------------------------------------------------------------------------------------------------- more than 8 192 tiles
def run_big(eng, tile, fused, options, source):
    data, nfill, case = fc.big_case(tile)
    want = fc.expected_decisions(case)
    nseq = nfill + len(want)
    nterm = 4 * nfill + fc.n_terminators(case.data)
    assert len(data) // tile > fc.SCAN_ROUND and len(data) % tile == 0
    cap = (nterm + 1) // 4 + 2
    eng.set_index(list(case.set.barcodes), list(case.tags), case.set.cutsite)
    from test_splitter_edges_gpu import set_splitter
    from tagdigger_amd import _binding as B
    set_splitter(eng, case.set)
    d = eng.dev_alloc(len(data))
    d_out = eng.dev_alloc((cap + SLACK) * 8)
    try:
        eng.h2d(d, data)
        del data
        eng.h2d(d_out, np.full((cap + SLACK) * 2, SENTINEL, dtype=np.uint32).tobytes())
        apply(eng, options)
        eng.reset()
        assert eng.split_kernel_in_use() == (2 if tile == fc.TILE2 else 1)
        nbytes = fc.BIG_FILLER_TILES * tile + len(case.data)
        terms = C.c_uint64(0)
        if fused:
            B.check(eng._L.td_count_and_split_device(eng._h, C.c_void_p(d), nbytes, 0, 10 ** 12, C.c_void_p(d_out), cap, None, C.byref(terms)))
        else:
            B.check(eng._L.td_split_device(eng._h, C.c_void_p(d), nbytes, 0, C.c_void_p(d_out), cap, None, C.byref(terms)))
        assert eng.split_prefix_source() == source
        assert eng.count_lines_device(d, nbytes) == nterm              # (k_count_lines<4> and k_scan_tiles over 16 KiB tiles: more than a round as well)
        res = np.frombuffer(eng.d2h(d_out, (cap + SLACK) * 8), dtype=np.int32).reshape(-1, 2)
        assert terms.value == nterm
        head = res[:nfill]
        bad = np.flatnonzero((head != np.array(fc.NO_BARCODE, dtype=np.int32)).any(axis=1))
        assert len(bad) == 0, ("filler slots that differ", len(bad), "first", bad[:4].tolist(), head[bad[:4]].tolist())
        got = res[nfill:nseq]
        diff = np.flatnonzero((got != want).any(axis=1))
        assert len(diff) == 0, ("decisions of the case that differ", len(diff), [(int(k), case.labels[k], got[k].tolist(), want[k].tolist()) for k in diff[:8]])
        assert (res[nseq:].view(np.uint32) == SENTINEL).all()
        if fused:
            m, st = fc.expected_counts(case)
            got_m, got_st = eng.counts_numpy(), eng.stats()
            assert (got_m == m).all()
            assert got_st == dict(reads=nfill + st["reads"], barcut=st["barcut"], tag=st["tag"], lines=nterm)
    finally:
        apply(eng, {})
        eng.dev_free(d)
        eng.dev_free(d_out)
    print(" [%d tiles of %d bytes, prefix source %d] " % (nbytes // tile, tile, source), end="")


def test_more_than_a_round_of_tiles_k_split(eng):
    """8 208 tiles of 16 KiB (134 MB) through td_split_device with k_split."""
    run_big(eng, fc.TILE1, False, dict(split_kernel=1), 1)


def test_more_than_a_round_of_tiles_k_split2(eng):
    """8 208 tiles of 24 KiB (201 MB) through td_split_device with k_split2: k_count_lines<6>."""
    run_big(eng, fc.TILE2, False, dict(split_kernel=2), 1)


def test_more_than_a_round_of_tiles_fused(eng):
    """The same 201 MB through the fused call with k_fast4: the scan runs over the count pass's records."""
    run_big(eng, fc.TILE2, True, dict(kernel=4, split_kernel=2), 2)
