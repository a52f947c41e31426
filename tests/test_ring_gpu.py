"""k_fast4's ring of five LDS slots taken deep on purpose (csrc/kernel_fast4.hpp; the same inputs through k_fast2 and
k_fast): td_set_option "max_grid" caps the main pass's grid, so that with 1 one workgroup takes all 40 to 190 tiles of
a buffer -- every slot used eight times and more, run after run -- and "run" decides where the line phase is carried
and where it is voted.  The inputs are tests/ring_cases.py's (tests/test_ring.py shows without a GPU that each reaches
its regime); the buffers are resident, one launch sees the whole of each; matrix and counters are the C oracle's,
exactly.  A wave of k_fast4 that waits gives up after a bounded spin and the host reports TD_E_INTERNAL: a protocol bug
fails a test here, it does not hang one."""
import numpy as np
import pytest

import ring_cases as rc
import test_progress as tp
from helpers import DEFAULT_MODE, apply_mode
from oracle import tagdigger_oracle as orc

pytestmark = pytest.mark.gpu

TILE = rc.TILE
RESTORE = dict(max_grid=0, run=8, f4_nprod=0, hot_cache=1, progress=0)
GEOMETRIES = [(1, 1), (1, 3), (1, 4096), (2, 1), (3, 2), (2, 8)]           # (max_grid, run)
NPROD = (0, 7, 10, 13)
GENERATORS = {"dirty": rc.g_dirty, "qual": rc.g_qual, "sparse": rc.g_sparse, "short": rc.g_short}
FIXQ = 11                                                                   # debug_counters(): length of the fix-up queue


@pytest.fixture(scope="module")
def eng():
    import tagdigger_amd
    e = tagdigger_amd.Engine(0)
    yield e
    e.close()


def restore(eng):
    apply_mode(eng, RESTORE)
    apply_mode(eng, DEFAULT_MODE)


class Resident:
    """A case's index set and its bytes in device memory."""

    def __init__(self, eng, case, data=None):
        self.eng, self.case = eng, case
        self.data = case.data if data is None else data
        self.d = 0

    def __enter__(self):
        self.eng.set_index(self.case.barcodes, self.case.tags, self.case.cutsite)
        self.cap = len(self.data) + 4096               # (a slid record changes the length by a few bytes)
        self.d = self.eng.dev_alloc(self.cap)
        self.eng.h2d(self.d, self.data)
        return self

    def __exit__(self, *exc):
        self.eng.dev_free(self.d)

    def load(self, data):
        assert len(data) <= self.cap
        self.eng.h2d(self.d, data)
        self.data = data

    def count(self, nbytes=None, **kw):
        self.eng.reset()
        self.eng.count_device(self.d, len(self.data) if nbytes is None else nbytes, **kw)

    def check(self, want, wst, label, nbytes=None, **kw):
        self.count(nbytes, **kw)
        got = self.eng.counts_numpy()
        st = self.eng.stats()
        assert (got == want).all(), (label, "cells that differ", int((got != want).sum()), "sum", int(got.sum()), int(want.sum()))
        if "maxreads" in kw:                # (a bound: the oracle stops reading there, the device counts the buffer's lines)
            st, wst = dict(st, lines=0), dict(wst, lines=0)
        assert st == wst, label


_want = {}


def oracle_of(case, **kw):
    key = (case.name, len(case.data), tuple(sorted(kw.items())))
    if key not in _want:
        _want[key] = rc.expected(case, **kw)
    return _want[key]


# ---------------------------------------------------------------------------------------------------- (a) ring geometries
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "grid%d-run%d" % g)
@pytest.mark.parametrize("gen", sorted(GENERATORS))
def test_ring_geometries_k_fast4(eng, gen, geometry):
    """Every dirty generator through one, two and three workgroups with runs of 1, 2, 3, 8 and 4096 tiles, at the estimated
    and at 7, 10 and 13 producer waves."""
    case = GENERATORS[gen]()
    want, wst = oracle_of(case)
    try:
        with Resident(eng, case) as r:
            apply_mode(eng, dict(fastpath=1, kernel=4, max_grid=geometry[0], run=geometry[1]))
            for nprod in NPROD:
                eng.set_option("f4_nprod", nprod)
                r.check(want, wst, (gen, geometry, nprod))
    finally:
        restore(eng)


@pytest.mark.parametrize("gen", sorted(GENERATORS))
def test_ring_geometries_k_fast2_and_k_fast(eng, gen):
    """The cap holds for the other generations of the main pass: k_fast2 (24 KiB tiles, runs) and k_fast (32 KiB tiles, no
    runs) with one and two workgroups."""
    case = GENERATORS[gen]()
    want, wst = oracle_of(case)
    try:
        with Resident(eng, case) as r:
            for mode in (dict(fastpath=1, kernel=2, tile_kb2=24, max_grid=1, run=3), dict(fastpath=1, kernel=2, tile_kb2=24, max_grid=2, run=8),
                         dict(fastpath=1, kernel=1, tile_kb=32, max_grid=1), dict(fastpath=1, kernel=1, tile_kb=32, max_grid=2)):
                apply_mode(eng, mode)
                r.check(want, wst, (gen, mode))
    finally:
        restore(eng)


def test_every_max_grid_value_is_accepted_and_the_counts_hold(eng):
    """1, more than there are tiles, 0 and a negative value (taken as 0): the counts are the oracle's.  A cap changes
    which workgroup takes a tile, never the counts or the fix-up queue: that it took effect cannot be seen from here."""
    case = rc.g_qual()
    want, wst = oracle_of(case)
    try:
        with Resident(eng, case) as r:
            for cap in (1, 10 ** 6, 0, -5):
                eng.set_option("max_grid", cap)
                r.check(want, wst, cap)
    finally:
        restore(eng)


# ---------------------------------------------------------------------------------------------------- (b) take-back that subtracts
def reads_before(data, offset):
    return rc.line_count(data[:offset]) // 4


@pytest.mark.parametrize("shape", ["run1", "run4096-shift"])
def test_take_back_subtracts(eng, shape):
    """G_qual, one workgroup.  run = 1: every tile votes, only quality lines can be voted for, every interior tile is
    matched under the wrong phase -- its quality lines counted as reads -- and queued twice: FX_NEG takes the wrong
    counts back from the matrix (more than 100 cells of it, tests/test_ring.py), an entry at the true phase counts the
    blank-led reads.  run = 4096: tile 1 votes (for the quality lines), every later tile carries that phase; two empty lines
    inside tile 5 put the blank-led lines into the carried phase from there on, so that the take-back behind them undoes
    lines that went the raw-bytes route.  The queue must hold a tile's worth of entries and more (about two per interior
    tile) -- the path was taken --, matrix and counters are the oracle's; then the same with a maxreads bound inside an
    interior, mispredicted tile (an FX_NEG and an FX_LIMIT entry for it) and with the hot-cell cache off and never resting."""
    case = rc.g_qual(1, shape != "run1")
    nt = rc.ntiles(case.data)
    want, wst = oracle_of(case)
    bound = reads_before(case.data, 20 * TILE + TILE // 2)
    bwant, bwst = oracle_of(case, maxreads=bound)
    assert 0 < bwst["reads"] == bound < wst["reads"]
    try:
        with Resident(eng, case) as r:
            apply_mode(eng, dict(fastpath=1, kernel=4, max_grid=1, run=1 if shape == "run1" else 4096))
            for hot in (1, 0, 2):
                eng.set_option("hot_cache", hot)
                r.check(want, wst, (shape, hot))
                nfix = eng.debug_counters()[FIXQ]
                print(" [%s hot_cache=%d: %d tiles, fix-up queue %d] " % (shape, hot, nt, nfix), end="")
                assert nfix >= nt, (shape, nfix, nt)
                r.check(bwant, bwst, (shape, hot, "maxreads", bound), maxreads=bound)
                nfix = eng.debug_counters()[FIXQ]
                print(" [maxreads %d: queue %d] " % (bound, nfix), end="")
                assert nfix >= nt, (shape, nfix, nt)        # (the tiles before the bound and the bound's own twice, the tiles behind it once)
    finally:
        restore(eng)


def test_carried_phase_holds_where_every_vote_is_wrong(eng):
    """G_qual behind two tiles of clean records, one workgroup, one run: tile 1 votes -- for the sequence lines --, and every
    later tile carries that phase through records whose only votable lines are quality lines.  Nothing but the buffer's
    first tile and its last ones (they are never matched in the main pass) is queued for the fix-up pass: fewer entries
    than a quarter of the tiles, where votes would queue two per tile.  With run = 1 the same input queues them."""
    case = rc.g_qual_behind_clean_head()
    nt = rc.ntiles(case.data)
    want, wst = oracle_of(case)
    try:
        with Resident(eng, case) as r:
            for nprod in NPROD:
                apply_mode(eng, dict(fastpath=1, kernel=4, max_grid=1, run=4096, f4_nprod=nprod))
                r.check(want, wst, ("carried", nprod))
                nfix = eng.debug_counters()[FIXQ]
                print(" [carried, %d producers: %d tiles, fix-up queue %d] " % (nprod, nt, nfix), end="")
                assert nfix < nt // 4, (nprod, nfix, nt)
            apply_mode(eng, dict(run=1, f4_nprod=0))
            r.check(want, wst, "voted")
            assert eng.debug_counters()[FIXQ] >= nt - 4 * rc.QUAL_HEAD_TILES
    finally:
        restore(eng)


def test_high_byte_in_the_halo_of_a_mispredicted_tile(eng):
    """G_qual with 0xE9 for the last base of a quality line's tag, three bytes behind tile 17's end: the line begins in tile
    17, is voted for (run = 1) and would be packed from the halo by the forms for ASCII bytes, which read the byte as a
    base; the take-back looks at the bytes exactly.  The producer of the last quarter flags the halo's byte, the tile is
    left to the fix-up pass, the counts are the oracle's."""
    case = rc.g_qual_high_byte_in_halo()
    want, wst = oracle_of(case)
    try:
        with Resident(eng, case) as r:
            for run in (1, 8):
                apply_mode(eng, dict(fastpath=1, kernel=4, max_grid=1, run=run))
                for nprod in NPROD:
                    eng.set_option("f4_nprod", nprod)
                    r.check(want, wst, (run, nprod))
            apply_mode(eng, dict(fastpath=1, kernel=2, tile_kb2=24, max_grid=1, run=1, f4_nprod=0))
            r.check(want, wst, "k_fast2")
    finally:
        restore(eng)


# ---------------------------------------------------------------------------------------------------- (c) progress windows
@pytest.mark.parametrize("gen", ["short", "qual"])
def test_progress_windows_in_the_ring(eng, gen):
    """The recording instantiation with one workgroup: a consumer's 64 lines lie in up to three tiles of the ring.  G_short:
    a window ends inside an interior tile, the cumulative windows are tests/test_progress.py's boundary_stats.  G_qual has
    7 000 reads -- no boundary, boundary_stats is empty --: what it checks is its one partial window against the oracle's
    counters, with every tile's sums taken under the wrong phase (run = 1 as well): they must not reach the window."""
    case = GENERATORS[gen]()
    want, wst = oracle_of(case)
    windows = tp.boundary_stats(rc.oracle(case), case.data, wst["reads"])
    try:
        with Resident(eng, case) as r:
            for run in (8, 1):
                apply_mode(eng, dict(fastpath=1, kernel=4, max_grid=1, run=run, progress=1))
                r.check(want, wst, (gen, run))
                w = eng.progress_windows()
                assert len(w) == -(-wst["reads"] // rc.WINDOW)
                got = list(zip(np.cumsum([a for a, _ in w]).tolist(), np.cumsum([b for _, b in w]).tolist()))
                assert got[:len(windows)] == windows, (gen, run)
                assert got[-1] == (wst["barcut"], wst["tag"])
    finally:
        restore(eng)


# ---------------------------------------------------------------------------------------------------- (d) byte sweeps inside the ring
def test_high_byte_sweep_in_a_header(eng):
    """One 0xE9 at every offset from tile 17's last two bytes through the halo behind it (the slot's fourth use; the halo
    is staged with the tile and flagged by the last quarter's producer), inside a header line: the tile, or the one whose
    halo holds the byte, goes to the fix-up pass; the counts are the oracle's."""
    frame, t0 = rc._hi_frame(False)
    base = rc.Case("hi frame", *rc.sweep_index(), rc.CUT, frame)
    try:
        with Resident(eng, base) as r:
            apply_mode(eng, dict(fastpath=1, kernel=4, max_grid=1, run=8))
            r.check(*oracle_of(base), "no high byte")
            for off in rc.hi_offsets():
                case = rc.hi_case(False, off)
                r.load(case.data)
                want, wst = rc.expected(case)
                r.check(want, wst, off)
    finally:
        restore(eng)


def test_high_byte_sweep_in_a_sequence(eng):
    """The same byte inside a sequence line that covers the span: NonAsciiSequence when the counts are fetched, as the
    reference's decode raises (the Python oracle at one offset, the C oracle at every one in tests/test_ring.py)."""
    import tagdigger_amd
    frame, t0 = rc._hi_frame(True)
    base = rc.Case("hi frame seq", *rc.sweep_index(), rc.CUT, frame)
    try:
        with Resident(eng, base) as r:
            apply_mode(eng, dict(fastpath=1, kernel=4, max_grid=1, run=8))
            r.check(*oracle_of(base), "no high byte")
            for off in rc.hi_offsets():
                case = rc.hi_case(True, off)
                r.load(case.data)
                r.count()
                try:
                    eng.counts()
                    raised = False
                except tagdigger_amd.NonAsciiSequence:
                    raised = True
                assert raised, off
            case = rc.hi_case(True, TILE + 5)
            with pytest.raises(orc.NonAsciiSequence):
                orc.count_bytes(case.data, case.barcodes, case.tags, case.cutsite)
            # the engine is usable afterwards
            r.load(frame)
            r.check(*oracle_of(base), "after the sweep")
    finally:
        restore(eng)


@pytest.mark.parametrize("lone_cr", [False, True], ids=["crlf", "cr"])
@pytest.mark.parametrize("boundary", sorted(rc.CRLF_BOUNDARIES))
def test_cr_slides_inside_the_ring(eng, boundary, lone_cr):
    """A \\r\\n record, and one with lone \\r terminators (a base behind the header's), slid byte by byte across a quarter's end, a
    lane's span's end and a chunk's end inside tile 17: where the \\r is a chunk's last byte the producer looks one byte ahead,
    in LDS or -- behind its own quarter -- in global memory, where the slot still holds tile 12's bytes."""
    first, _ = rc.crlf_case(boundary, 0, lone_cr)
    try:
        with Resident(eng, first) as r:
            apply_mode(eng, dict(fastpath=1, kernel=4, max_grid=1, run=8))
            for step in range(rc.CRLF_STEPS):
                case, target = rc.crlf_case(boundary, step, lone_cr)
                r.load(case.data)
                want, wst = rc.expected(case)
                r.check(want, wst, (boundary, step, target), nbytes=len(case.data))
    finally:
        restore(eng)


@pytest.mark.parametrize("lone_cr", [False, True], ids=["crlf", "cr"])
def test_cr_at_every_quarter_end(eng, lone_cr):
    """The one-off of the slides at every quarter of every tile: a \\r as a quarter's last byte, its \\n (or the read's first
    base) the next quarter's first -- bytes of another producer, which may not have stored them yet: the slot may still hold
    the bytes of the tile five before.  k_fast4 at several geometries and producer counts, k_fast2 once."""
    case = rc.g_cr_at_quarter_ends(lone_cr)
    want, wst = oracle_of(case)
    try:
        with Resident(eng, case) as r:
            for max_grid, run in ((1, 1), (1, 8), (2, 3)):
                apply_mode(eng, dict(fastpath=1, kernel=4, max_grid=max_grid, run=run))
                for nprod in NPROD:
                    eng.set_option("f4_nprod", nprod)
                    r.check(want, wst, (max_grid, run, nprod))
            apply_mode(eng, dict(fastpath=1, kernel=2, tile_kb2=24, max_grid=1, run=8, f4_nprod=0))
            r.check(want, wst, "k_fast2")
    finally:
        restore(eng)


# ---------------------------------------------------------------------------------------------------- (e) hot-slot thrash
@pytest.mark.parametrize("max_grid", [1, 4])
def test_hot_slot_thrash(eng, max_grid):
    """Three hits in five go to two cells that share a slot of the hot-cell cache, in turn; one in five to a cell with a slot
    of its own: evictions write the loser's count out, every flush the winner's."""
    case = rc.g_hotslot()
    want, wst = oracle_of(case)
    try:
        with Resident(eng, case) as r:
            for kernel in (dict(kernel=4), dict(kernel=2, tile_kb2=24)):
                apply_mode(eng, dict(fastpath=1, max_grid=max_grid, run=8, **kernel))
                for hot in (0, 1, 2):
                    eng.set_option("hot_cache", hot)
                    r.check(want, wst, (max_grid, kernel, hot))
    finally:
        restore(eng)


def test_hot_slot_cache_rests_and_comes_back(eng):
    """40 MB through ONE workgroup with thirteen producers: its three consumers live through some 30 ageing periods each.
    96 barcodes x 200 tags: in the uniform first part a consumer's cache has some 30 hits a period where 90 keep it on
    (the cache restated: ring_cases.hc_model, asserted in tests/test_ring.py), so it is switched off after its first
    period, counts with plain atomics beside what stays in LDS for fifteen periods, and comes back inside the part; the hot
    part gives it 2 000 hits a period, the two colliding cells fighting for their slot; the last part switches it off again.
    Only the counts are asserted -- when a wave's cache goes off and on cannot be seen from outside; with the cache off and
    never resting the same bytes give the same counts."""
    case, reads = rc.g_hotslot_long()
    want, wst = oracle_of(case)
    try:
        with Resident(eng, case) as r:
            for hot in (1, 0, 2):
                apply_mode(eng, dict(fastpath=1, kernel=4, max_grid=1, run=8, f4_nprod=13, hot_cache=hot))
                r.check(want, wst, ("40 MB, one workgroup", hot))
    finally:
        restore(eng)
